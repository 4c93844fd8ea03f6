#!/usr/bin/env python3
"""Generate tests/golden/progan_critic.npz by running the REFERENCE's own ProGAN critic (stylegan.Discriminator,
stylegan.py:181-263).

Runs only where the reference checkout exists (never on the GPU box); it imports the reference exactly as
tools/make_goldens.py does.  Weights come from ``oracle.weights_recipe`` (``fill_state_dict(prefix="critic.",
wscale_convs=True)``, the aliased ``rgb_layers.8`` / ``initial_rgb`` pair sharing the ``initial_rgb`` values) and are never
stored; inputs from ``recipe_input``.  Per case (steps, alpha, B) of ``progan_critic_ref.GOLDEN_CASES`` it stores:

  {tag}.logits        D(x), [B, 1]
  {tag}.gx            d(sum D(x))/dx                 (every 4th pixel at >= 64^2)
  {tag}.gnorm         ||d(sum D(x))/dp|| per parameter, in the order of {tag}.names
  {tag}.gp            the WGAN-GP penalty (progan_critic_ref.wgan_gp, lambda 10)
  {tag}.gp_gx         d(gp)/dx_hat                   (every 4th pixel at >= 64^2)
  {tag}.gp_gnorm      ||d(gp)/dp|| per parameter, in the order of {tag}.gp_names

    python tools/make_critic_goldens.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

from make_goldens import import_reference, npf, save  # noqa: E402
import progan_critic_ref as CR  # noqa: E402


def gen_critic(ref_progan):
    d = ref_progan.Discriminator(512).eval()
    d.load_state_dict(CR.critic_recipe_state_dict(d.state_dict()))
    params = list(d.named_parameters())          # initial_rgb is listed once (as rgb_layers.8)
    out = {}
    for steps, alpha, B in CR.GOLDEN_CASES:
        tag = CR.case_tag(steps, alpha, B)
        x, fake, eps = CR.case_inputs(steps, alpha, B)
        D = lambda t: d(t, alpha, steps)          # noqa: E731
        xr = x.clone().requires_grad_(True)
        d.zero_grad()
        y = D(xr)
        y.sum().backward()
        names = [n for n, p in params if p.grad is not None]
        out[f"{tag}.names"] = np.array(names)
        out[f"{tag}.logits"] = npf(y)
        out[f"{tag}.gx"] = npf(CR.sample(xr.grad))
        out[f"{tag}.gnorm"] = np.array([p.grad.double().norm().item() for n, p in params if p.grad is not None])
        d.zero_grad()
        gp, x_hat = CR.wgan_gp(D, x, fake, eps)
        gp.backward()
        out[f"{tag}.gp_names"] = np.array([n for n, p in params if p.grad is not None])     # (a last bias never reaches gp)
        out[f"{tag}.gp"] = np.float64(gp.item())
        out[f"{tag}.gp_gx"] = npf(CR.sample(x_hat.grad))
        out[f"{tag}.gp_gnorm"] = np.array([p.grad.double().norm().item() for n, p in params if p.grad is not None])
        print(f"  {tag}: logits {y.detach().flatten().tolist()}, gp {gp.item():.6g}")
    save("progan_critic.npz", **out)


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    _, ref_progan = import_reference()
    gen_critic(ref_progan)


if __name__ == "__main__":
    main()
