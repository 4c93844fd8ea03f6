"""SPK_EPI_RESIDUAL: relu(conv1x1(x, w) + b + r) -- the residual joins BEFORE the activation -- on every tile config built for a
stride-1 1x1 conv (the tap kernel's 8-11 incl. a forced split-K whose finisher applies it, the GEMM forms 12 / 14 / 15), against
the same expression in fp64; and its rejection everywhere else.  Bound: 2e-5 rel-L2, the project's per-op bound
(test_encoder_gpu.TOL_OP: exact fp32 arithmetic, only the summation order differs)."""
import ctypes as C
import importlib

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from oracle.weights_recipe import recipe_input, recipe_tensor

pytestmark = pytest.mark.gpu
TOL_OP = 2e-5


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _launch(pkg, x, wp, Cout, cfg, ksplit, **kw):
    B, _, H, W = x.shape
    y = torch.empty((B, Cout, H, W), device=x.device, dtype=torch.float32)
    d, ws_bytes = pkg.ops.conv_desc(x, wp, Cout, 1, 1, out=y, config=cfg, ksplit=ksplit, **kw)
    pkg.ops._run_conv2d(d, ws_bytes, x.device)
    return y, ws_bytes


def _cases(pkg, cfg):
    """Shapes with a ragged last channel tile and a ragged last pixel tile that the config hosts."""
    lib = pkg._lib.lib()
    # (10 x 18: W % 4 != 0, so the tap kernel leaves its staged float4 epilogue for the per-element one)
    for (B, Cin, Cout, H, W) in [(3, 40, 72, 24, 20), (3, 40, 72, 8, 16), (3, 48, 72, 16, 16), (3, 40, 72, 10, 18)]:
        if lib.spk_conv2d_workspace_bytes(cfg, 1, 1, 1, 1, B, Cin, Cout, H, W) >= 0:
            yield B, Cin, Cout, H, W


def test_residual_before_activation_every_1x1_config(pkg, dev):
    lib = pkg._lib.lib()
    cfgs = [c for c in range(lib.spk_conv2d_num_configs()) if lib.spk_conv2d_config_valid(c, 1, 1, 1)]
    assert {12, 14, 15} <= set(cfgs) and len(cfgs) >= 7, cfgs
    ran, split_ran = set(), 0
    for cfg in cfgs:
        for (B, Cin, Cout, H, W) in _cases(pkg, cfg):
            tag = f"res.{B}.{Cin}.{Cout}.{H}.{W}"
            x, w = recipe_input(tag + ".x", (B, Cin, H, W)), recipe_tensor(tag + ".weight", (Cout, Cin, 1, 1))
            b, r = recipe_tensor(tag + ".bias", (Cout,)), recipe_input(tag + ".r", (B, Cout, H, W))
            pre = F.conv2d(x.double(), w.double()) + b.double().view(1, -1, 1, 1) + r.double()
            wp = pkg.ops.pack_conv_weight(w.to(dev), cfg)
            for ksplit in (1, 2):
                for relu in (True, False):
                    # (ksplit = 2 is honoured by the tap kernel, configs 8-11; the GEMM forms never split K and run whole)
                    y, ws = _launch(pkg, x.to(dev), wp, Cout, cfg, ksplit, bias=b.to(dev), residual=r.to(dev),
                                    lrelu_slope=0.0 if relu else None)
                    err = rel_l2(y, torch.relu(pre) if relu else pre)
                    print(f"cfg {cfg} {tag} ksplit {ksplit} (workspace {ws} B) relu {relu}: rel-L2 {err:.3e}")
                    assert err < TOL_OP, (cfg, tag, ksplit, relu, err)
                    split_ran += ws > 0
            ran.add(cfg)
    assert ran == set(cfgs), (ran, cfgs)
    assert split_ran >= 2          # a forced split-K ran: the finisher applied the residual


def test_residual_leaky_slope_and_accumulate(pkg, dev):
    """The stage order: lrelu(v + bias + residual), then SPK_EPI_ACCUM adds the old y after the activation."""
    B, Cin, Cout, H, W = 2, 64, 72, 8, 16
    x, w = recipe_input("res2.x", (B, Cin, H, W)), recipe_tensor("res2.weight", (Cout, Cin, 1, 1))
    b, r, old = recipe_tensor("res2.bias", (Cout,)), recipe_input("res2.r", (B, Cout, H, W)), recipe_input("res2.old", (B, Cout, H, W))
    ref = F.leaky_relu(F.conv2d(x.double(), w.double()) + b.double().view(1, -1, 1, 1) + r.double(), 0.2) + old.double()
    for cfg in (10, 12, 15):
        wp = pkg.ops.pack_conv_weight(w.to(dev), cfg)
        y = old.to(dev).clone()
        d, ws = pkg.ops.conv_desc(x.to(dev), wp, Cout, 1, 1, out=y, config=cfg, ksplit=1, bias=b.to(dev), residual=r.to(dev),
                                  lrelu_slope=0.2, accumulate=True)
        pkg.ops._run_conv2d(d, ws, dev)
        err = rel_l2(y, ref)
        print(f"cfg {cfg} lrelu 0.2 + accumulate: rel-L2 {err:.3e}")
        assert err < TOL_OP, (cfg, err)


def test_residual_flag_rejected_elsewhere(pkg, dev):
    L, lib = pkg._lib, pkg._lib.lib()
    B, Cc, H = 2, 64, 32
    x = torch.zeros(B, Cc, H, H, device=dev)
    r = torch.zeros(B, Cc, H, H, device=dev)
    y = torch.empty_like(r)
    w3 = torch.zeros(Cc, Cc, 3, 3, device=dev)

    def rejected(d):
        code = lib.spk_conv2d_fwd(C.byref(d), L.stream_ptr())
        msg = lib.spk_last_error().decode()
        assert code < 0 and msg, (code, msg)
        return msg

    # 3x3 on the direct kernel
    cfg = pkg.ops.conv2d_pick_config(3, 1, B, Cc, Cc, H, H)
    d, _ = pkg.ops.conv_desc(x, pkg.ops.pack_conv_weight(w3, cfg), Cc, 3, 1, out=y, config=cfg, ksplit=1)
    d.flags |= L.EPI_RESIDUAL
    d.residual = r.data_ptr()
    assert "RESIDUAL" in rejected(d)
    # Winograd
    assert pkg.ops.wino_supported(B, Cc, Cc, H, H)
    d, _ = pkg.ops.conv_desc(x, pkg.ops.pack_conv_weight_wino(w3), Cc, 3, 1, flags=L.CONV_WINOGRAD, out=y, ksplit=1)
    d.flags |= L.EPI_RESIDUAL
    d.residual = r.data_ptr()
    rejected(d)
    # a 1x1 with BatchNorm statistics, a strided 1x1, and a missing residual pointer
    w1 = torch.zeros(Cc, Cc, 1, 1, device=dev)
    cfg = pkg.ops.conv2d_pick_config(1, 1, B, Cc, Cc, H, H)
    stats = torch.zeros(pkg.ops.stats_slots(cfg, 1, 1, B, Cc, Cc, H, H) * 2 * Cc, device=dev, dtype=torch.float64)
    d, _ = pkg.ops.conv_desc(x, pkg.ops.pack_conv_weight(w1, cfg), Cc, 1, 1, out=y, config=cfg, ksplit=1, stats=stats)
    d.flags |= L.EPI_RESIDUAL
    d.residual = r.data_ptr()
    assert "RESIDUAL" in rejected(d)
    d, _ = pkg.ops.conv_desc(x, pkg.ops.pack_conv_weight(w1, cfg), Cc, 1, 1, out=y, config=cfg, ksplit=1)
    d.flags |= L.EPI_RESIDUAL
    assert "residual" in rejected(d)
    cfg2 = pkg.ops.conv2d_pick_config(1, 2, B, Cc, Cc, H // 2, H // 2)
    y2 = torch.empty(B, Cc, H // 2, H // 2, device=dev)
    d, _ = pkg.ops.conv_desc(x, pkg.ops.pack_conv_weight(w1, cfg2), Cc, 1, 2, out=y2, config=cfg2, ksplit=1)
    d.flags |= L.EPI_RESIDUAL
    d.residual = r.data_ptr()
    assert "RESIDUAL" in rejected(d)
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,Hin,Win", [(2, 64, 64), (1, 50, 72)])
def test_stem_bias_relu_epilogue(pkg, dev, B, Hin, Win):
    """The 7x7 stride-2 stem form (tile config 16) with SPK_EPI_BIAS | SPK_EPI_LRELU -- a BatchNorm-folded stem: bn1 + ReLU --
    against relu(conv + b) in fp64, whole and partial tiles; and with a leaky slope."""
    tag = f"stemepi.{B}.{Hin}.{Win}"
    x, w = recipe_input(tag + ".x", (B, 3, Hin, Win), "uniform"), recipe_tensor(tag + ".weight", (64, 3, 7, 7))
    b = recipe_tensor(tag + ".bias", (64,))
    pre = F.conv2d(x.double(), w.double(), stride=2, padding=3) + b.double().view(1, -1, 1, 1)
    Ho, Wo = pre.shape[-2:]
    cfg = pkg.ops.conv2d_pick_config(7, 2, B, 3, 64, Ho, Wo)
    assert cfg == 16
    wp = pkg.ops.pack_conv_weight(w.to(dev), cfg)
    for slope in (0.0, 0.2):
        y = torch.empty((B, 64, Ho, Wo), device=dev, dtype=torch.float32)
        d, ws = pkg.ops.conv_desc(x.to(dev), wp, 64, 7, 2, out=y, config=cfg, bias=b.to(dev), lrelu_slope=slope)
        pkg.ops._run_conv2d(d, ws, dev)
        err = rel_l2(y, F.leaky_relu(pre, slope))
        print(f"stem bias + lrelu({slope}) {tag}: rel-L2 {err:.3e}")
        assert err < TOL_OP
