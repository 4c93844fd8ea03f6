"""GPU parity of the inference entry point: ``plan.EncoderPlan`` (a BatchNorm-folded ResNet-50 trunk as one launch list) against
``oracle.resnet_ref.resnet50_trunk``, and ``IRFD.reenact`` against the composed oracle
``style_generator(cat(Ei(identity).expand(T), Ee(emotion), Ep(pose)))``.  Bounds: 2e-4 rel-L2 at the trunk features
(``TOL_TRUNK`` of test_encoder_gpu.py; folding spends none of it: 3.0e-7 folded against 2.9e-7 unfolded on the CPU), 5e-4 at the
frames (the bound test_irfd_forward_eval_vs_oracle uses for the same trunk -> 8 FC -> 12 conv chain)."""
import importlib

import pytest
import torch

from conftest import rel_l2
from oracle import decoder_ref as DR
from oracle import irfd_ref as IR
from oracle import resnet_ref as RR
from oracle.weights_recipe import fill_state_dict, recipe_input, recipe_noises, resnet_trunk_state_dict

pytestmark = pytest.mark.gpu
TOL_TRUNK = 2e-4
TOL_FRAMES = 5e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


@pytest.fixture(scope="module")
def irfd_and_sd(dev):
    import model
    m = model.IRFD()
    sd = IR.irfd_recipe_state_dict()
    sd.update({"Gd." + k: v for k, v in fill_state_dict(m.Gd.state_dict(), prefix="Gd.").items()})
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("D.") for k in missing)
    return m.to(dev).eval(), sd


def _trunk_ref(x, sd, which):
    return RR.resnet50_trunk(x.double(), {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, prefix=which + ".")


def _restore(m, sd):
    m.load_state_dict({k: v for k, v in sd.items()}, strict=False)


@pytest.mark.parametrize("B,H", [(2, 96), (2, 256), (1, 64)])
@pytest.mark.parametrize("algo", ["auto", "direct"])
def test_encoder_plan_vs_oracle(irfd_and_sd, pkg, dev, B, H, algo):
    m, sd = irfd_and_sd
    x = recipe_input(f"reenact.enc.{B}.{H}", (B, 3, H, H), "uniform")
    with pkg.ops.conv3x3_algo(algo):
        got = m.encode(x.to(dev), "Ee")
    assert got.shape == (B, 2048, 1, 1)
    err = rel_l2(got, _trunk_ref(x, sd, "Ee"))
    print(f"EncoderPlan B={B} H={H} algo={algo}: rel-L2 {err:.3e}")
    assert err < TOL_TRUNK


def test_encoder_plan_is_one_launch_list_of_55_ops(irfd_and_sd, pkg, dev, monkeypatch):
    m, _ = irfd_and_sd
    L, PL = pkg._lib, importlib.import_module("speak-hack_amd.plan")
    x = recipe_input("reenact.ops", (2, 3, 256, 256), "uniform").to(dev)
    m.encode(x, "Ep")                                   # builds (and packs) the plan
    plan = next(p for p in m.Ep.__dict__["_plans"].values() if isinstance(p, PL.EncoderPlan) and p.B == 2 and p.H == 256)
    kinds = [k for k, _ in plan.ops]
    assert len(kinds) == 55 and kinds.count(L.OP_CONV2D) == 53 and kinds.count(L.OP_MAXPOOL3X3S2) == 1 and kinds.count(L.OP_GLOBAL_AVGPOOL) == 1
    convs = [d for k, d in plan.ops if k == L.OP_CONV2D]
    assert not any(d.flags & (L.EPI_STATS | L.CONV_IN_AFFINE_RELU) for d in convs)
    assert sum(bool(d.flags & L.EPI_RESIDUAL) for d in convs) == 16
    # every 3x3 stride-1 conv sits on the kernel ops.conv3x3_route names for its shape
    for d in convs:
        if d.kh == 3 and d.stride == 1:
            assert bool(d.flags & L.CONV_WINOGRAD) == (pkg.ops.conv3x3_route(d.B, d.Cin, d.Cout, d.H, d.W, precision="f32")[0] == "wino")
    lib = L.lib()
    calls = {"list": 0, "conv": 0}
    real_list, real_conv = lib.spk_launch_list, lib.spk_conv2d_fwd

    def count_list(*a):
        calls["list"] += 1
        return real_list(*a)

    def count_conv(*a):
        calls["conv"] += 1
        return real_conv(*a)

    monkeypatch.setattr(lib, "spk_launch_list", count_list)
    monkeypatch.setattr(lib, "spk_conv2d_fwd", count_conv)
    m.encode(x, "Ep")
    monkeypatch.undo()
    assert calls == {"list": 1, "conv": 0}, calls


def test_encoder_plan_headline_batch_runs_its_3x3_as_winograd(irfd_and_sd, pkg, dev):
    """At the headline batch (8 frames of 256^2) the launches fill the chip: the 64^2 / 32^2 / 16^2 3x3 stride-1 convs are
    Winograd launches (the training-shaped path cannot: its inputs carry the producer's affine + ReLU)."""
    m, sd = irfd_and_sd
    L, PL = pkg._lib, importlib.import_module("speak-hack_amd.plan")
    x = recipe_input("reenact.b8", (8, 3, 256, 256), "uniform")
    got = m.encode(x.to(dev), "Ee")
    plan = next(p for p in m.Ee.__dict__["_plans"].values() if isinstance(p, PL.EncoderPlan) and p.B == 8 and p.H == 256)
    wino = {(d.H, d.W) for k, d in plan.ops if k == L.OP_CONV2D and d.flags & L.CONV_WINOGRAD}
    assert {(64, 64), (32, 32), (16, 16)} <= wino, wino
    err = rel_l2(got, _trunk_ref(x, sd, "Ee"))
    print(f"EncoderPlan B=8 H=256 (Winograd layers {sorted(wino)}): rel-L2 {err:.3e}")
    assert err < TOL_TRUNK


def _composed_oracle(sd, ident, pose, emo, noises):
    T = pose.size(0)
    fi = RR.resnet50_trunk(ident, sd, prefix="Ei.")
    fe, fp = RR.resnet50_trunk(emo, sd, prefix="Ee."), RR.resnet50_trunk(pose, sd, prefix="Ep.")
    gin = torch.cat([fi.expand(T, -1, -1, -1).reshape(T, -1), fe.reshape(T, -1), fp.reshape(T, -1)], 1)
    gsd = {k[3:]: v for k, v in sd.items() if k.startswith("Gd.")}
    return DR.style_generator(gin, gsd, noises)


def test_reenact_vs_composed_oracle(irfd_and_sd, dev):
    m, sd = irfd_and_sd
    T = 3
    ident = recipe_input("reenact.id", (1, 3, 256, 256), "uniform")
    pose = recipe_input("reenact.pose", (T, 3, 256, 256), "uniform")
    emo = recipe_input("reenact.emo", (T, 3, 256, 256), "uniform")
    noises = recipe_noises("reenact", T, 256)
    with torch.no_grad():
        ref = _composed_oracle(sd, ident, pose, emo, noises)
    dn = [n.to(dev) for n in noises]
    got = m.reenact(ident.to(dev), pose.to(dev), emo.to(dev), noises=dn, chunk=2)       # two plans, one ragged chunk
    assert got.shape == (T, 3, 256, 256) and got.dtype == torch.float32
    for lo, hi in ((0, 2), (2, 3)):
        err = rel_l2(got[lo:hi], ref[lo:hi])
        print(f"reenact frames [{lo}:{hi}]: rel-L2 {err:.3e}")
        assert err < TOL_FRAMES
    a = m.reenact(ident.to(dev), pose.to(dev), None, noises=dn, chunk=2)
    b = m.reenact(ident.to(dev), pose.to(dev), pose.to(dev), noises=dn, chunk=2)
    assert torch.equal(a, b)


def test_reenact_in_train_mode_is_eval_arithmetic_without_side_effects(irfd_and_sd, dev):
    m, sd = irfd_and_sd
    T = 2
    ident = recipe_input("reenact.tr.id", (1, 3, 128, 128), "uniform").to(dev)
    pose = recipe_input("reenact.tr.pose", (T, 3, 128, 128), "uniform").to(dev)
    dn = [n.to(dev) for n in recipe_noises("reenact.tr", T, 256)]
    m.eval()
    ref = m.reenact(ident, pose, noises=dn)
    m.train()
    held = m.Gd.synthesis.to_rgb
    held.eval()                           # a submodule deliberately held in eval keeps its flag
    try:
        before = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
        rng = torch.get_rng_state()
        got = m.reenact(ident, pose, noises=dn)
        assert torch.equal(torch.get_rng_state(), rng)
        assert m.training and m.Gd.training and m.Ee.training and not held.training
        after = m.state_dict()
        assert len(before) == 3 * 53 * 3
        for k, v in before.items():
            assert torch.equal(after[k], v), k
    finally:
        m.eval()
    assert torch.equal(got, ref)


def test_encoder_plan_refresh(irfd_and_sd, dev):
    m, sd = irfd_and_sd
    x = recipe_input("reenact.refresh", (2, 3, 96, 96), "uniform")
    try:
        assert rel_l2(m.encode(x.to(dev), "Ei"), _trunk_ref(x, sd, "Ei")) < TOL_TRUNK
        # a running statistic scaled in place
        sd2 = dict(sd)
        sd2["Ei.5.1.bn2.running_var"] = sd["Ei.5.1.bn2.running_var"] * 3.0
        with torch.no_grad():
            m.Ei[5][1].bn2.running_var.mul_(3.0)
        got = m.encode(x.to(dev), "Ei")
        err_new, err_old = rel_l2(got, _trunk_ref(x, sd2, "Ei")), rel_l2(got, _trunk_ref(x, sd, "Ei"))
        print(f"refresh (running_var x3): rel-L2 vs new {err_new:.3e}, vs old {err_old:.3e}")
        assert err_new < TOL_TRUNK < err_old
        # load_state_dict of another recipe prefix
        other = resnet_trunk_state_dict("Ep.")
        m.Ei.load_state_dict(other)
        sd3 = {"Ei." + k: v for k, v in other.items()}
        got = m.encode(x.to(dev), "Ei")
        err_new, err_old = rel_l2(got, _trunk_ref(x, sd3, "Ei")), rel_l2(got, _trunk_ref(x, sd, "Ei"))
        print(f"refresh (load_state_dict): rel-L2 vs new {err_new:.3e}, vs old {err_old:.3e}")
        assert err_new < TOL_TRUNK < err_old
    finally:
        _restore(m, sd)
    assert rel_l2(m.encode(x.to(dev), "Ei"), _trunk_ref(x, sd, "Ei")) < TOL_TRUNK


def test_encoder_plan_refresh_after_training_forward(irfd_and_sd, dev):
    """A train-mode forward of the trunk updates the running statistics from inside a kernel; the next ``encode`` folds the
    updated values (oracle: the same training forward on a copy of the state, then the eval trunk on what it left)."""
    m, sd = irfd_and_sd
    x = recipe_input("reenact.refresh.train", (2, 3, 96, 96), "uniform")
    try:
        assert rel_l2(m.encode(x.to(dev), "Ei"), _trunk_ref(x, sd, "Ei")) < TOL_TRUNK
        sd2 = {k: v.clone() for k, v in sd.items() if k.startswith("Ei.")}
        with torch.no_grad():
            RR.resnet50_trunk(x, sd2, prefix="Ei.", training=True, update_running_stats=True)
            m.Ei.train()
            m.Ei(x.to(dev))
            m.Ei.eval()
        assert rel_l2(m.Ei[5][1].bn2.running_var, sd2["Ei.5.1.bn2.running_var"]) < 1e-4         # the statistics did move as the oracle's
        assert rel_l2(sd["Ei.5.1.bn2.running_var"], sd2["Ei.5.1.bn2.running_var"]) > 1e-2
        got = m.encode(x.to(dev), "Ei")
        err_new, err_old = rel_l2(got, _trunk_ref(x, sd2, "Ei")), rel_l2(got, _trunk_ref(x, sd, "Ei"))
        print(f"refresh (training forward): rel-L2 vs new {err_new:.3e}, vs old {err_old:.3e}")
        assert err_new < TOL_TRUNK < err_old
    finally:
        m.eval()
        _restore(m, sd)
