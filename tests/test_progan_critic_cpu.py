"""CPU checks of the ProGAN critic: the functional restatement (tests/progan_critic_ref.py) reproduces the reference's own
outputs (tests/golden/progan_critic.npz), and the library exports the critic's entry points."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import progan_critic_ref as CR
from conftest import rel_l2


def test_restatement_matches_reference_goldens(golden):
    g = golden("progan_critic.npz")
    sd = CR.critic_recipe_state_dict()
    for steps, alpha, B in CR.GOLDEN_CASES:
        tag = CR.case_tag(steps, alpha, B)
        x, fake, eps = CR.case_inputs(steps, alpha, B)
        params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if not k.startswith("initial_rgb.")}
        params.update({"initial_rgb." + s: params[f"rgb_layers.{CR.N_BLOCKS}.{s}"] for s in ("bias", "conv.weight")})
        D = lambda t: CR.critic(t, alpha, steps, params)          # noqa: E731
        xr = x.clone().requires_grad_(True)
        y = D(xr)
        assert y.shape == (B, 1)
        assert rel_l2(y, g[f"{tag}.logits"]) <= 5e-6, tag
        y.sum().backward()
        assert rel_l2(CR.sample(xr.grad), g[f"{tag}.gx"]) <= 5e-6, tag
        for key, names in (("gnorm", "names"), ("gp_gnorm", "gp_names")):
            if key == "gp_gnorm":
                for p in params.values():
                    p.grad = None
                gp, x_hat = CR.wgan_gp(D, x, fake, eps)
                assert abs(gp.item() - float(g[f"{tag}.gp"])) <= 1e-5 * abs(float(g[f"{tag}.gp"])), tag
                gp.backward()
                assert rel_l2(CR.sample(x_hat.grad), g[f"{tag}.gp_gx"]) <= 5e-6, tag
            got = np.array([params[n].grad.double().norm().item() for n in g[f"{tag}.{names}"]])
            np.testing.assert_allclose(got, g[f"{tag}.{key}"], rtol=1e-5, err_msg=f"{tag} {key}")


def test_library_exports_the_critic_entry_points():
    import __graft_entry__ as ge
    ge.build()
    pkg = importlib.import_module("speak-hack_amd")
    h = ctypes.CDLL(pkg._lib.LIB_PATH)
    for s in ("spk_avgpool2x_blend_fwd", "spk_avgpool2x_blend_bwd", "spk_minibatch_std_workspace_bytes", "spk_minibatch_std_fwd",
              "spk_minibatch_std_bwd"):
        assert hasattr(h, s), s
        assert s in pkg._lib.exported_symbols(), s
    lib = pkg._lib.lib()
    assert lib.spk_minibatch_std_workspace_bytes(512, 16) >= (2 * 512 * 16 + 1) * 4
    assert lib.spk_minibatch_std_workspace_bytes(0, 16) < 0


def test_critic_state_dict_layout():
    prog = importlib.import_module("speak-hack_amd.progan")
    d = prog.Discriminator(512)
    assert {k: tuple(v.shape) for k, v in d.state_dict().items()} == CR.critic_param_shapes()
    assert d.rgb_layers[CR.N_BLOCKS] is d.initial_rgb
    sd = CR.critic_recipe_state_dict(d.state_dict())
    d.load_state_dict(sd)
    assert torch.equal(d.initial_rgb.conv.weight, sd["initial_rgb.conv.weight"])
