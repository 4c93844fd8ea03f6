"""Direct fp64 tests of the small forward / backward kernels of the training path that the module tests only reach through
whole-network gradients: the plain toRGB 1x1 (``conv1x1_small``: csrc/pointwise.hip) and its backward (``conv1x1_small_bwd``:
csrc/decoder_bwd.hip), the grouped FC backward (``fc_grouped_bwd``) and the decoder prologue (``bias_noise_style`` /
``const_prologue``).  Shapes are chosen per dispatch branch; the criterion is rounding level element by element (see
``assert_rounding`` in test_sg2_backward_kernels_gpu.py)."""
import importlib
import math

import pytest
import torch

from oracle.weights_recipe import recipe_input, recipe_tensor
from test_sg2_backward_kernels_gpu import assert_rounding, place, rtol_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd.ops")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("speak-hack_amd._lib")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ---- conv1x1_small (plain toRGB forward) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,O,H,W,has_bias,misaligned", [
    (2, 64, 3, 2, 2, True, False),       # csplit, n4 = 1 (Q = 1)
    (1, 96, 2, 2, 4, True, False),       # csplit, n4 = 2 (Q = 2)
    (2, 128, 4, 4, 4, False, False),     # csplit, n4 = 4, bias None
    (1, 64, 1, 4, 8, True, False),       # csplit, n4 = 8, O = 1
    (2, 100, 3, 12, 12, True, False),    # csplit, n4 = 36 >= 16: Q = 16 with a ragged last workgroup; C % 16 != 0
    (8, 512, 3, 4, 4, True, False),      # realistic: the 4^2 toRGB
    (2, 32, 3, 16, 16, True, False),     # C < 64: the one-thread-per-quad kernel <true>
    (2, 64, 3, 16, 16, False, True),     # x / y 4 bytes off: kernel <false>
    (2, 70, 4, 7, 9, True, False),       # HW % 4 != 0: kernel <false>
    (2, 16, 3, 256, 256, True, False),   # realistic: a 16-channel toRGB at 256^2, <true> over many workgroups
])
def test_conv1x1_small(ops, dev, B, C, O, H, W, has_bias, misaligned):
    key = f"smk.c1s.{B}.{C}.{O}.{H}.{W}"
    x = recipe_input(key + ".x", (B, C, H, W))
    w = recipe_tensor(key + ".w", (O, C, 1, 1), 1.0)
    bias = recipe_tensor(key + ".bias", (O,), 0.3) if has_bias else None
    in_scale = 1 / math.sqrt(C)
    y = ops.conv1x1_small(place(x, dev, misaligned), w.to(dev), bias.to(dev) if has_bias else None, in_scale)
    x64, w64 = x.double().flatten(2), in_scale * w.double().reshape(O, C)
    ref = torch.einsum("oc,bcp->bop", w64, x64)
    ref_abs = torch.einsum("oc,bcp->bop", w64.abs(), x64.abs())
    if has_bias:
        ref, ref_abs = ref + bias.double()[None, :, None], ref_abs + bias.double().abs()[None, :, None]
    assert_rounding(y, ref.view(B, O, H, W), ref_abs.view(B, O, H, W), rtol_for(C + 1), 1e-5, what="y")


# ---- conv1x1_small_bwd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,O,H,W,in_scale,misaligned", [
    (2, 16, 3, 12, 12, 1.0, False),      # the old single shape: vector data kernel, one tile per image
    (2, 100, 3, 12, 12, 1.0, False),     # C % 64 != 0: a ragged second channel group (dword staging)
    (1, 64, 2, 10, 15, 0.5, False),      # HW = 150: not a multiple of 128 (ragged last tile), HW % 4 != 0: dword data kernel
    (2, 64, 4, 48, 48, 0.25, False),     # 2304 px: five blocks per image, the last with a ragged tile
    (2, 64, 3, 16, 16, 1.0, True),       # x / dy 4 bytes off: the weight kernel's vec_ok off, dword data kernel
    (4, 128, 1, 32, 32, 0.125, False),   # O = 1, two channel groups, full vector tiles
    (2, 64, 3, 256, 256, 1.0, False),    # realistic: 128 blocks per image
])
@pytest.mark.parametrize("need_dx", [True, False])
def test_conv1x1_small_bwd(ops, dev, B, C, O, H, W, in_scale, misaligned, need_dx):
    key = f"smk.c1b.{B}.{C}.{O}.{H}.{W}"
    x = recipe_input(key + ".x", (B, C, H, W))
    w = recipe_tensor(key + ".w", (O, C, 1, 1), 1.0)
    dy = recipe_input(key + ".dy", (B, O, H, W))
    dx, dw, db = ops.conv1x1_small_bwd(place(x, dev, misaligned), w.to(dev), place(dy, dev, misaligned), need_dx, in_scale)
    x64, w64, dy64 = x.double().flatten(2), w.double().reshape(O, C), dy.double().flatten(2)
    assert_rounding(dw, in_scale * torch.einsum("bop,bcp->oc", dy64, x64).view(O, C, 1, 1),
                    in_scale * torch.einsum("bop,bcp->oc", dy64.abs(), x64.abs()).view(O, C, 1, 1), rtol_for(B * H * W), 1e-5, what="dw")
    assert_rounding(db, dy64.sum((0, 2)), dy64.abs().sum((0, 2)), rtol_for(B * H * W), 1e-5, what="db")
    if need_dx:
        assert_rounding(dx, in_scale * torch.einsum("oc,bop->bcp", w64, dy64).view(B, C, H, W),
                        in_scale * torch.einsum("oc,bop->bcp", w64.abs(), dy64.abs()).view(B, C, H, W), rtol_for(O), what="dx")
    else:
        assert dx is None


def test_conv1x1_small_refusals(ops, L, dev):
    for O, C in ((5, 8), (4, 3073)):                                 # more than 4 outputs; [O][C] weights beyond 48 KiB of LDS
        x = torch.zeros((1, C, 4, 4), device=dev)
        w = torch.zeros((O, C, 1, 1), device=dev)
        with pytest.raises(L.SpkError):
            ops.conv1x1_small(x, w)
        with pytest.raises(L.SpkError):
            ops.conv1x1_small_bwd(x, w, torch.zeros((1, O, 4, 4), device=dev))


# ---- fc_grouped_bwd ---------------------------------------------------------------------------------------------------------
def _fc_ref(dout, out, x, w, wmul, bmul, slope):
    dz = dout.double() * torch.where(out > 0, 1.0, slope).double()
    w64, x64 = w.double(), x.double()
    return ((wmul * dz @ w64, wmul * dz.abs() @ w64.abs()),
            (wmul * dz.t() @ x64, wmul * dz.abs().t() @ x64.abs()),
            (bmul * dz.sum(0), bmul * dz.abs().sum(0)))


# (I, O) per group: O = 40 runs the 8-row unrolled loop once plus a remainder, O = 7 only the remainder, O = 128 only the loop
GROUPS = [(64, 40), (100, 7), (512, 128), (37, 64)]


@pytest.mark.parametrize("B", [3, 8, 11, 16])       # one partial batch tile; exactly one; a ragged second; two (the batch-16 config)
def test_fc_grouped_bwd(ops, dev, B):
    """Groups of different I / O in one launch; dx written into column views of ONE tensor; group 1 reads a row-strided dout;
    group 2 has no dw, group 3 no bias; slopes 0.2 (with about half the saved outputs negative) and 1."""
    key = f"smk.fcb.{B}"
    Itot = sum(I for I, _ in GROUPS)
    dx_all = torch.full((B, Itot + 5), 7.0, device=dev)          # sentinel columns past the groups' stay untouched
    x_all = recipe_input(key + ".x", (B, Itot + 3))
    dout_wide = recipe_input(key + ".dout_wide", (B, 100 + 9))
    items, refs, j, jx = [], [], 0, 0
    for gi, (I, O) in enumerate(GROUPS):
        w = recipe_tensor(f"{key}.{gi}.w", (O, I), 1.0)
        out = recipe_input(f"{key}.{gi}.out", (B, O))
        dout = dout_wide[:, 9:9 + O] if gi == 1 else recipe_input(f"{key}.{gi}.dout", (B, O))
        x = x_all[:, jx:jx + I]
        need_dw, has_bias = gi != 2, gi != 3
        wmul, bmul, slope = 1 / math.sqrt(I), 0.5, (0.2 if gi % 2 == 0 else 1.0)
        dx = dx_all[:, j:j + I]
        items.append(((dout_wide.to(dev)[:, 9:9 + O] if gi == 1 else dout.to(dev)), out.to(dev), x_all.to(dev)[:, jx:jx + I], w.to(dev), dx,
                      need_dw, has_bias, wmul, bmul, slope))
        refs.append((_fc_ref(dout, out, x, w, wmul, bmul, slope), need_dw, has_bias, j, I))
        j, jx = j + I, jx + I
    assert items[1][0].stride(0) == 109
    res = ops.fc_grouped_bwd(items, B)
    dx_host = dx_all.cpu()
    for (((rdx, rdx_abs), (rdw, rdw_abs), (rdb, rdb_abs)), need_dw, has_bias, j, I), (dw, db), (_, O) in zip(refs, res, GROUPS):
        assert_rounding(dx_host[:, j:j + I], rdx, rdx_abs, rtol_for(O), 1e-5, what=f"dx [{I}x{O}]")
        if need_dw:
            assert_rounding(dw, rdw, rdw_abs, rtol_for(B), 1e-5, what=f"dw [{I}x{O}]")
        else:
            assert dw is None
        if need_dw and has_bias:
            assert_rounding(db, rdb, rdb_abs, rtol_for(B), 1e-5, what=f"db [{I}x{O}]")
        else:
            assert db is None
    assert torch.equal(dx_host[:, Itot:], torch.full((B, 5), 7.0))


def test_fc_grouped_bwd_without_dx(ops, dev):
    """dx None for every group: only the weight kernel runs."""
    B, I, O = 16, 48, 20
    w, x = recipe_tensor("smk.fcb.nodx.w", (O, I), 1.0), recipe_input("smk.fcb.nodx.x", (B, I))
    out, dout = recipe_input("smk.fcb.nodx.out", (B, O)), recipe_input("smk.fcb.nodx.dout", (B, O))
    (dw, db), = ops.fc_grouped_bwd([(dout.to(dev), out.to(dev), x.to(dev), w.to(dev), None, True, True, 0.25, 2.0, 0.2)], B)
    _, (rdw, rdw_abs), (rdb, rdb_abs) = _fc_ref(dout, out, x, w, 0.25, 2.0, 0.2)
    assert_rounding(dw, rdw, rdw_abs, rtol_for(B), 1e-5, what="dw")
    assert_rounding(db, rdb, rdb_abs, rtol_for(B), 1e-5, what="db")


def test_fc_grouped_bwd_refuses_too_many_groups(ops, L, dev):
    B, I, O = 2, 8, 4
    t = lambda *s: torch.zeros(s, device=dev)
    items = [(t(B, O), t(B, O), t(B, I), t(O, I), t(B, I), True, True, 1.0, 1.0, 1.0) for _ in range(L.FC_MAX_GROUPS + 1)]
    with pytest.raises(L.SpkError):
        ops.fc_grouped_bwd(items, B)


# ---- bias_noise_style / const_prologue --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W,broadcast", [
    (2, 5, 7, 9, False),
    (3, 300, 4, 4, True),      # a [1,C,H,W] constant broadcast over the batch (const_prologue)
    (8, 512, 4, 4, True),      # realistic: the 4^2 prologue at B = 8
])
@pytest.mark.parametrize("has_bias,has_noise,has_style", [
    (a, b, c) for a in (True, False) for b in (True, False) for c in (True, False)])
def test_bias_noise_style(ops, dev, B, C, H, W, broadcast, has_bias, has_noise, has_style):
    """Every subset of bias / noise / style None; the style rows are a column block of a wider buffer (row stride 2C + 7)."""
    key = f"smk.bns.{B}.{C}.{H}"
    x = recipe_input(key + ".x", (1 if broadcast else B, C, H, W))
    bias = recipe_tensor(key + ".bias", (C,), 0.3) if has_bias else None
    nw = recipe_tensor(key + ".nw", (C,), 0.3) if has_noise else None
    noise = recipe_input(key + ".noise", (B, 1, H, W)) if has_noise else None
    style_buf = recipe_input(key + ".style", (B, 2 * C + 10))
    style = style_buf[:, 3:3 + 2 * C] if has_style else None
    dv = lambda t: t.to(dev) if t is not None else None
    style_d = style_buf.to(dev)[:, 3:3 + 2 * C] if has_style else None
    if broadcast and has_bias and has_noise and has_style:
        y = ops.const_prologue(x.to(dev), dv(bias), dv(nw), dv(noise), style_d, B)
    else:
        y = ops.bias_noise_style(x.to(dev), B, dv(bias), dv(nw), dv(noise), style_d)
    v = x.double().expand(B, C, H, W)
    v_abs = v.abs()
    if has_bias:
        v, v_abs = v + bias.double()[None, :, None, None], v_abs + bias.double().abs()[None, :, None, None]
    if has_noise:
        t = nw.double()[None, :, None, None] * noise.double()
        v, v_abs = v + t, v_abs + t.abs()
    if has_style:
        s0, s1 = (style.double()[:, :C] + 1)[:, :, None, None], style.double()[:, C:][:, :, None, None]
        v, v_abs = v * s0 + s1, v_abs * (s0 - 1).abs().add(1) + s1.abs()      # (|s0| + 1: the kernel forms s0 + 1 first)
    assert_rounding(y, v, v_abs, rtol_for(4), what="y")
