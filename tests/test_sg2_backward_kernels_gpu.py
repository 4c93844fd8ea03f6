"""Direct fp64 tests of the small backward kernels of the StyleGAN2 variant (csrc/stylegan2_bwd.hip and the plane-sum reduction
of csrc/decoder_bwd.hip): ``modconv_dx_finish``, ``modconv_demod_bwd``, ``modconv_epi_finish``, ``torgb_mod_bwd`` and
``plane_sums_reduce``, at shapes that reach every dispatch branch.

These ops have no ReLU, so they are held to rounding level ELEMENT BY ELEMENT (``assert_rounding``): for every output element
|got - ref64| <= rtol * ref_abs + atol, where ``ref_abs`` is the same float64 contraction evaluated on absolute values (immune to
cancellation), plus a rel-L2 bound.  One wrong element -- a tail block, a second batch tile, the last channel chunk -- fails."""
import importlib
import math

import pytest
import torch

from oracle import modconv_ref as M
from oracle.weights_recipe import recipe_input, recipe_tensor

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24                     # unit roundoff of float32


def rtol_for(terms):
    """8 u sqrt(terms): the element-wise bound for a sum of ``terms`` products (at least 4 terms' worth)."""
    return 8 * U32 * math.sqrt(max(terms, 4))


def assert_rounding(got, ref, ref_abs, rtol, l2=2e-6, atol=1e-30, what=""):
    """|got - ref| <= rtol * ref_abs + atol for every element, and rel-L2(got, ref) <= l2; ``ref`` / ``ref_abs`` are float64."""
    g = got.detach().cpu().double()
    ref, ref_abs = ref.double(), ref_abs.double()
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} != {tuple(ref.shape)}"
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    err = (g - ref).abs()
    bound = rtol * ref_abs + atol
    bad = err > bound
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        idx = tuple(int(k) for k in torch.unravel_index(torch.tensor(i), g.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements outside rounding; first at {idx}: got "
                             f"{float(g.flatten()[i]):.9g}, ref {float(ref.flatten()[i]):.9g}, |err| {float(err.flatten()[i]):.3g} > "
                             f"bound {float(bound.flatten()[i]):.3g}")
    rel = float((g - ref).norm() / ref.norm().clamp_min(1e-300))
    assert rel <= l2, f"{what}: rel-L2 {rel:.3e} > {l2:.0e}"


def offset_copy(t, dev):
    """``t`` on ``dev`` as a contiguous view 4 bytes past a 16-byte boundary."""
    v = torch.empty(t.numel() + 1, device=dev, dtype=torch.float32)[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def place(t, dev, misaligned=False):
    return offset_copy(t, dev) if misaligned else t.to(dev)


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


# ---- modconv_dx_finish ------------------------------------------------------------------------------------------------------
def _up_adjoint(g):
    """up^T(g) for oracle.modconv_ref.upsample2x, by float64 autograd."""
    B, C, H, W = g.shape
    x = torch.zeros((B, C, H // 2, W // 2), dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad((M.upsample2x(x) * g).sum(), x)
    return gx


@pytest.mark.parametrize("B,C,Hs,Ws", [
    (2, 3, 4, 4),        # 8 items per plane: most threads idle
    (1, 2, 5, 6),        # odd low-res height, Ws % 4 == 2 (the halo of the last column pair)
    (2, 3, 32, 32),      # 512 items per plane: two trips of the item loop
    (1, 2, 23, 46),      # 529 items, a ragged last trip
    (8, 16, 8, 8),       # realistic: the 8^2 -> 16^2 layer of the variant at B = 8
])
@pytest.mark.parametrize("need_dx", [True, False])
def test_modconv_dx_finish_x2(ops, dev, B, C, Hs, Ws, need_dx):
    key = f"sg2k.dxf2.{B}.{C}.{Hs}.{Ws}"
    g = recipe_input(key + ".g", (B, C, 2 * Hs, 2 * Ws))
    x = recipe_input(key + ".x", (B, C, Hs, Ws))
    s = recipe_input(key + ".s", (B, C))
    dx, ds = ops.modconv_dx_finish(g.to(dev), x.to(dev), s.to(dev), True, need_dx=need_dx)
    g64, x64, s64 = g.double(), x.double(), s.double()
    ut, ut_abs = _up_adjoint(g64), _up_adjoint(g64.abs())
    assert_rounding(ds, (ut * x64).sum((2, 3)), (ut_abs * x64.abs()).sum((2, 3)), rtol_for(16 * Hs * Ws), 1e-5, what="ds")
    if need_dx:
        sv = s64[:, :, None, None]
        assert_rounding(dx, ut * sv, ut_abs * sv.abs(), rtol_for(16), what="dx")
    else:
        assert dx is None


def test_modconv_dx_finish_x2_refusals(ops, L, dev):
    g = recipe_input("sg2k.dxf2r.g", (1, 2, 8, 10)).to(dev)
    x = recipe_input("sg2k.dxf2r.x", (1, 2, 4, 5)).to(dev)
    s = recipe_input("sg2k.dxf2r.s", (1, 2)).to(dev)
    with pytest.raises(L.SpkError):                                  # odd low-resolution width
        ops.modconv_dx_finish(g, x, s, True)
    g = recipe_input("sg2k.dxf2r.g4", (1, 2, 8, 8))
    x = recipe_input("sg2k.dxf2r.x4", (1, 2, 4, 4))
    with pytest.raises(L.SpkError):                                  # gradient not 16-byte aligned
        ops.modconv_dx_finish(offset_copy(g, dev), x.to(dev), s, True)
    with pytest.raises(L.SpkError):                                  # input not 8-byte aligned
        ops.modconv_dx_finish(g.to(dev), offset_copy(x, dev), s, True)


@pytest.mark.parametrize("B,C,H,W,misaligned", [
    (2, 3, 4, 4, False),       # vec: HW % 4 == 0, aligned
    (2, 3, 32, 32, False),     # vec, 256 quads per plane: one full trip
    (1, 2, 37, 29, False),     # dword: HW % 4 != 0 (1073 px, > 4 trips)
    (2, 3, 16, 16, True),      # dword: HW % 4 == 0 but every tensor 4 bytes off a 16-byte boundary
    (8, 64, 16, 16, False),    # realistic: a 16^2 same-resolution layer at B = 8
])
@pytest.mark.parametrize("need_dx", [True, False])
def test_modconv_dx_finish_same_res(ops, dev, B, C, H, W, misaligned, need_dx):
    """The same-resolution form scales the gradient IN PLACE (dx is dxt); need_dx=False must leave it untouched."""
    key = f"sg2k.dxf1.{B}.{C}.{H}.{W}"
    g = recipe_input(key + ".g", (B, C, H, W))
    x = recipe_input(key + ".x", (B, C, H, W))
    s = recipe_input(key + ".s", (B, C))
    gd = place(g, dev, misaligned)
    dx, ds = ops.modconv_dx_finish(gd, place(x, dev, misaligned), place(s, dev, misaligned), False, need_dx=need_dx)
    g64, x64, s64 = g.double(), x.double(), s.double()
    assert_rounding(ds, (g64 * x64).sum((2, 3)), (g64 * x64).abs().sum((2, 3)), rtol_for(H * W), 1e-5, what="ds")
    if need_dx:
        assert dx is gd
        sv = s64[:, :, None, None]
        assert_rounding(dx, g64 * sv, (g64 * sv).abs(), rtol_for(1), what="dx")
    else:
        assert dx is None
        assert torch.equal(gd.cpu(), g)


# ---- modconv_demod_bwd ------------------------------------------------------------------------------------------------------
def _demod_inputs(key, B, Cin, Cout, k):
    w = recipe_tensor(key + ".w", (Cout, Cin, k, k), 1.0)
    s = 1.0 + recipe_tensor(key + ".s", (B, Cin), 0.3)
    dd = recipe_input(key + ".dd", (B, Cout))
    scale = 1 / math.sqrt(Cin * k * k)
    d64 = torch.rsqrt(scale ** 2 * torch.einsum("oik,bi->bo", w.double().pow(2).flatten(2), s.double().pow(2)) + 1e-8)
    return w, s, d64.float().contiguous(), dd, scale


def _demod_ref(w, s, dd, scale):
    """(ds, dw) of <dd, d> with d = rsqrt(scale^2 sum s^2 w^2 + eps), float64 autograd; and the abs-contractions."""
    w64 = w.double().requires_grad_(True)
    s64 = s.double().requires_grad_(True)
    d = torch.rsqrt(scale ** 2 * torch.einsum("oik,bi->bo", w64.pow(2).flatten(2), s64.pow(2)) + 1e-8)
    ds, dw = torch.autograd.grad((d * dd.double()).sum(), (s64, w64))
    e_abs = (dd.double() * d.detach().pow(3)).abs() * scale ** 2                     # |e[b,co]|
    w2 = w.double().pow(2).flatten(2).sum(2)                                          # [Cout, Cin]
    ds_abs = s.double().abs() * (e_abs @ w2)
    dw_abs = w.double().abs() * torch.einsum("bo,bi->oi", e_abs, s.double().pow(2))[:, :, None, None]
    return ds, dw, ds_abs, dw_abs


@pytest.mark.parametrize("B,Cin,Cout,k", [
    (2, 16, 24, 3),        # one ci block, one co chunk with a tail (24 of 32)
    (17, 40, 33, 3),       # B > 16: two batch tiles, the second with one image; Cout % 32 == 1: a 1-channel last chunk
    (33, 64, 64, 1),       # three batch tiles, taps = 1
    (3, 130, 70, 3),       # Cin % 64 == 2: a 2-lane last ci block; three co chunks
    (8, 512, 512, 3),      # realistic: a 512-channel 3x3 layer at B = 8
])
@pytest.mark.parametrize("want", ["ds", "dw", "both"])
def test_modconv_demod_bwd(ops, dev, B, Cin, Cout, k, want):
    """Accumulating op: ds / dw hold recipe values before the call and are checked against old + ref."""
    key = f"sg2k.dbw.{B}.{Cin}.{Cout}.{k}"
    w, s, d, dd, scale = _demod_inputs(key, B, Cin, Cout, k)
    ds0 = recipe_input(key + ".ds0", (B, Cin))
    dw0 = recipe_tensor(key + ".dw0", (Cout, Cin, k, k), 0.01)
    ds = ds0.to(dev) if want in ("ds", "both") else None
    dw = dw0.to(dev) if want in ("dw", "both") else None
    ops.modconv_demod_bwd(w.to(dev), s.to(dev), d.to(dev), dd.to(dev), scale, ds=ds, dw=dw)
    rds, rdw, ds_abs, dw_abs = _demod_ref(w, s, dd, scale)
    if ds is not None:
        assert_rounding(ds, ds0.double() + rds, ds0.double().abs() + ds_abs, rtol_for(Cout * k * k), 1e-5, what="ds")
    if dw is not None:
        assert_rounding(dw, dw0.double() + rdw, dw0.double().abs() + dw_abs, rtol_for(B), 1e-5, what="dw")


def test_modconv_demod_bwd_is_bitwise_reproducible(ops, dev):
    """demod_bwd claims a fixed summation order (no atomics): two calls give bitwise equal ds and dw."""
    w, s, d, dd, scale = _demod_inputs("sg2k.dbw.rep", 20, 96, 80, 3)
    args = [t.to(dev) for t in (w, s, d, dd)]
    res = []
    for _ in range(2):
        ds = torch.zeros((20, 96), device=dev)
        dw = torch.zeros_like(args[0])
        ops.modconv_demod_bwd(*args, scale, ds=ds, dw=dw)
        res.append((ds.cpu(), dw.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ---- modconv_epi_finish -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C", [(2, 24), (3, 300), (8, 512)])      # one partial block; C > 256 with a 44-channel tail; realistic
@pytest.mark.parametrize("has_d,has_bias,has_nw", [
    (True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)])
def test_modconv_epi_finish(ops, dev, B, C, has_d, has_bias, has_nw):
    key = f"sg2k.epi.{B}.{C}"
    sums = recipe_input(key + ".sums", (B, 4, C))
    d = (0.5 + recipe_tensor(key + ".d", (B, C), 0.1).abs()) if has_d else None
    bias = recipe_tensor(key + ".bias", (C,), 0.3) if has_bias else None
    nw = recipe_tensor(key + ".nw", (C,), 0.3) if has_nw else None
    gain = math.sqrt(2)
    dd, dprime, dbias, dnw = ops.modconv_epi_finish(sums.to(dev), *(t.to(dev) if t is not None else None for t in (d, bias, nw)), gain)
    s64 = sums.double()
    d64 = d.double() if has_d else torch.ones((B, C), dtype=torch.float64)
    b64 = bias.double() if has_bias else torch.zeros(C, dtype=torch.float64)
    n64 = nw.double() if has_nw else torch.zeros(C, dtype=torch.float64)
    assert_rounding(dprime, d64 * gain, d64.abs() * gain, rtol_for(1), what="dprime")
    if has_d:
        terms = (s64[:, 0], -gain * n64 * s64[:, 3], -gain * b64 * s64[:, 2])
        assert_rounding(dd, sum(terms) / d64, sum(t.abs() for t in terms) / d64.abs(), rtol_for(3), what="dd")
    else:
        assert dd is None
    for got, present, row in ((dbias, has_bias, 2), (dnw, has_nw, 3)):
        if present:
            assert_rounding(got, gain * s64[:, row].sum(0), gain * s64[:, row].abs().sum(0), rtol_for(B), what="dbias/dnw")
        else:
            assert got is None


# ---- plane_sums_reduce ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C", [(1, 7), (5, 300), (8, 512)])       # one image; C > 256 with a tail; realistic
@pytest.mark.parametrize("row", [0, 1, 2, 3])
@pytest.mark.parametrize("accumulate", [False, True])
def test_plane_sums_reduce(ops, dev, B, C, row, accumulate):
    key = f"sg2k.psr.{B}.{C}"
    sums = recipe_input(key + ".sums", (B, 4, C))
    old = recipe_input(key + f".old{row}", (C,))
    out = old.to(dev) if accumulate else None
    got = ops.plane_sums_reduce(sums.to(dev), row, out=out)
    if accumulate:
        assert got is out
    ref = sums.double()[:, row].sum(0)
    ref_abs = sums.double()[:, row].abs().sum(0)
    if accumulate:
        ref, ref_abs = ref + old.double(), ref_abs + old.double().abs()
    assert_rounding(got, ref, ref_abs, rtol_for(B + 1), 1e-5, what="plane sums")


# ---- torgb_mod_bwd ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,O,H,W,misaligned", [
    (2, 8, 1, 8, 8, False),         # O = 1, vec data kernel, one 64-pixel tile
    (2, 70, 2, 5, 5, False),        # O = 2, HW % 4 != 0: dword data kernel; C % 64 == 6: a ragged channel group
    (1, 64, 3, 16, 16, True),       # O = 3, HW % 4 == 0 but dy and x 4 bytes off: dword data kernel, weight kernel's vec_ok off
    (2, 3072, 4, 2, 2, False),      # O = 4, C at the LDS limit (4 x 3072 floats = 48 KiB)
    (2, 33, 3, 40, 40, False),      # 1600 px: four blocks per image, the last tile ragged
    (8, 512, 3, 4, 4, False),       # realistic: the 4^2 toRGB
    (2, 64, 3, 256, 256, False),    # realistic: the 256^2 toRGB (128 blocks per image, full vector tiles)
])
@pytest.mark.parametrize("need_dx", [True, False])
def test_torgb_mod_bwd(ops, dev, B, C, O, H, W, misaligned, need_dx):
    key = f"sg2k.trgb.{B}.{C}.{O}.{H}"
    x = recipe_input(key + ".x", (B, C, H, W))
    w = recipe_tensor(key + ".w", (O, C, 1, 1), 1.0)
    mod = recipe_input(key + ".mod", (B, C))
    dy = recipe_input(key + ".dy", (B, O, H, W))
    in_scale = 1 / math.sqrt(C)
    dx, P, db = ops.torgb_mod_bwd(place(x, dev, misaligned), w.to(dev), mod.to(dev), place(dy, dev, misaligned), in_scale, need_dx)
    x64, w64, m64, dy64 = x.double().flatten(2), w.double().reshape(O, C), mod.double(), dy.double().flatten(2)
    assert_rounding(P, in_scale * torch.einsum("bop,bcp->boc", dy64, x64), in_scale * torch.einsum("bop,bcp->boc", dy64.abs(), x64.abs()),
                    rtol_for(H * W), 1e-5, what="P")
    assert_rounding(db, dy64.sum((0, 2)), dy64.abs().sum((0, 2)), rtol_for(B * H * W), 1e-5, what="db")
    if need_dx:
        wm = in_scale * w64[None] * m64[:, None, :]                                   # [B, O, C]
        ref = torch.einsum("boc,bop->bcp", wm, dy64).view(B, C, H, W)
        ref_abs = torch.einsum("boc,bop->bcp", wm.abs(), dy64.abs()).view(B, C, H, W)
        assert_rounding(dx, ref, ref_abs, rtol_for(O), what="dx")
    else:
        assert dx is None


def test_torgb_mod_bwd_refusals(ops, L, dev):
    for O, C in ((5, 8), (4, 3073)):                                 # more than 4 outputs; [O][C] weights beyond 48 KiB of LDS
        x = torch.zeros((1, C, 4, 4), device=dev)
        with pytest.raises(L.SpkError):
            ops.torgb_mod_bwd(x, torch.zeros((O, C, 1, 1), device=dev), torch.zeros((1, C), device=dev),
                              torch.zeros((1, O, 4, 4), device=dev))
