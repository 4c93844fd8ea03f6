"""The decoder plan with the x2 interpolation inside the Winograd launches (ops.WINO_FUSE_X2, SPK_WINO_FUSE_X2): no
SPK_OP_UPSAMPLE2X in the launch list, the x2 layers' descriptors carry SPK_CONV_WINOGRAD | SPK_CONV_UPSAMPLE2X and read the
low-resolution activation; with the switch off the passes are back.  Both forms against each other (5e-6, the Winograd bound) and
against the oracle (the bound of tests/test_decoder_gpu.py)."""
import importlib
import os
import sys

import pytest
import torch

from conftest import rel_l2
from oracle import decoder_ref as R
from oracle.weights_recipe import fill_state_dict, recipe_input, recipe_noises

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOL_E2E = 1e-4      # tests/test_decoder_gpu.py


def _plan_of(s):
    plans = list(s.__dict__["_plans"].values())
    assert len(plans) == 1
    return plans[0]


def test_plan_fuses_the_x2_pass_and_the_switch_restores_it(monkeypatch):
    pkg = importlib.import_module("speak-hack_amd")
    L, ops = pkg._lib, pkg.ops
    dev = torch.device("cuda:0")
    s = pkg.SynthesisNetwork(resolution=32).eval()
    sd = fill_state_dict(s.state_dict(), prefix="Gd32x2.synthesis.")
    s.load_state_dict(sd)
    s.to(dev)
    B = 2
    w = recipe_input("x2plan.w", (B, s.num_layers, 512))
    noises = recipe_noises("x2plan", B, 32)
    assert ops.WINO_FUSE_X2
    both = L.CONV_WINOGRAD | L.CONV_UPSAMPLE2X
    with torch.no_grad():
        y_f = s(w.to(dev), [n.to(dev) for n in noises])
        plan = _plan_of(s)
        assert not any(kind == L.OP_UPSAMPLE2X for kind, _ in plan.ops)
        convs = [d for kind, d in plan.ops if kind == L.OP_CONV2D]
        up = {d.H: d for d in convs if d.Hin * 2 == d.H}
        assert sorted(up) == [8, 16, 32]
        assert up[16].flags & both == both and up[32].flags & both == both
        assert not up[8].flags & L.CONV_WINOGRAD          # (8 x 8 is no whole region: the direct kernel, interpolating while staging)
        s.__dict__["_plans"].clear()
        monkeypatch.setattr(ops, "WINO_FUSE_X2", False)
        y_p = s(w.to(dev), [n.to(dev) for n in noises])
        plan = _plan_of(s)
        assert sum(kind == L.OP_UPSAMPLE2X for kind, _ in plan.ops) == 2
        assert not any(d.flags & both == both for kind, d in plan.ops if kind == L.OP_CONV2D)
        s.__dict__["_plans"].clear()
        ref = R.synthesis_network(w, sd, noises, prefix="", resolution=32)
    assert y_f.shape == (B, 3, 32, 32)
    assert rel_l2(y_f, y_p) < 5e-6, rel_l2(y_f, y_p)
    assert rel_l2(y_f, ref) < TOL_E2E and rel_l2(y_p, ref) < TOL_E2E
