"""GPU checks of the aligned NV12 edge (csrc/frame_sim_nv12.hip): ``ops.frames_from_nv12_aligned``, ``ops.frames_paste_nv12_aligned``
and ``ops.paste_colour_match_nv12`` against the numpy fp64 model tests/nv12_sim_ref.py (written from the definitions in
include/spk.h on top of sim_ref, blend_ref and nv12_ref), against the axis-aligned NV12 launchers where a box makes the two forms
one, and the clip-level composition of INTEGRATION.md in slices against one call.  The cases are those of tests/nv12_sim_cases.py;
tests/test_nv12_align_cpu.py asserts their margins, partial chroma blocks and variances.

Bounds.  Way in: 5e-7 absolute on (-1, 1) outputs, the bound of tests/test_align_gpu.py -- the arithmetic is fp64 up to the one
rounding to fp32, and the clamp is 1-Lipschitz.  Whole frame at s = 2 against ``ops.frames_from_nv12``: 2e-6 (that file's bound for
the same comparison) times the gain ``sum_j |to_rgb[c][j]|`` of the channel's row, as ``in_bounds`` of tests/test_nv12_gpu.py has
it.  Way out: ``|got - z| <= 0.5 + 1e-4`` on every Y, U and V byte without colour rows and ``0.5 + 2e-4`` with rows of gain <= 2,
the two bounds of tests/test_blend_gpu.py (no row of ``from_rgb`` has an absolute sum above 1, so the conversion adds no gain).
Colour rows: ``|g - g_ref| <= 2^-22 g_ref`` and ``|o - o_ref| <= 2^-15``, that file's bounds.  Every test prints what it measures."""
import importlib

import numpy as np
import pytest
import torch

import blend_ref as B
import nv12_sim_cases as NC
import nv12_sim_ref as M
import sim_ref as R
from oracle import irfd_ref as IR
from oracle.weights_recipe import fill_state_dict, recipe_noises

pytestmark = pytest.mark.gpu
H, W = NC.H, NC.W
TOL_IN, TOL_TABLE, TOL_OUT, TOL_COLOUR, TOL_G, TOL_O = 5e-7, 2e-6, 0.5 + 1e-4, 0.5 + 2e-4, 2.0 ** -22, 2.0 ** -15


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


def packed(y, uv):
    """The two planes as one surface tensor [N, 3H/2, W]"""
    return torch.cat([y, uv.reshape(y.size(0), y.size(1) // 2, y.size(2))], 1).contiguous()


def on(c, dev):
    """A case where the kernels want it: -> (x, pitched surfaces between guard bytes, device rows, matte, keywords of the way out)"""
    kw = dict(feather=c["feather"], **c["colour"])
    return c["x"].to(dev), NC.Pitched(c["y"], c["uv"], dev), c["rows"].to(dev), None if c["matte"] is None else c["matte"].to(dev), kw


# ---- in -----------------------------------------------------------------------------------------------------------------------------
def check_in(got, y, uv, rows, net, colour, bgr, what):
    to_rgb, _ = NC.coeffs(**colour)
    want, hit = M.warp_in(y.numpy(), uv.numpy(), np.asarray(rows), net[0], net[1], to_rgb, swap_rb=bgr)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    g = got.cpu().numpy()
    err = float(np.abs(g.astype(np.float64) - want).max())
    clamped = float(((want[hit[:, None].repeat(3, 1)] == -1) | (want[hit[:, None].repeat(3, 1)] == 1)).mean()) if hit.any() else 0.0
    print(f"way in, {what}: largest |got - model| = {err:.3e} (bound {TOL_IN}); {int((~hit).sum())} of {hit.size} outputs by rule, "
          f"{100 * clamped:.1f}% of the rest at a clamp")
    assert err <= TOL_IN
    assert (g[(~hit)[:, None].repeat(3, 1)] == -1.0).all()                  # shift_c exactly
    return hit


@pytest.mark.parametrize("name,bgr", [("generic 601", False), ("wide 709", True), ("full range", False), ("matte frames 709", True),
                                      ("raw bytes", False)])
def test_way_in_against_the_model(pkg, dev, name, bgr):
    """BT.601 limited, BT.709 limited, both full ranges, rgb and bgr, in-gamut surfaces and raw bytes; rotation, s < 1, s > 2 and the
    identity; pitched planes between guard bytes."""
    c = NC.case(name)
    surf = NC.Pitched(c["y"], c["uv"], dev)
    order = "bgr" if bgr else "rgb"
    got = pkg.ops.frames_from_nv12_aligned(surf.planes, c["net"], c["rows"].to(dev), channel_order=order, **c["colour"])
    torch.cuda.synchronize()
    check_in(got, c["y"], c["uv"], c["rows"], c["net"], c["colour"], bgr, f"{name}, {order}")
    assert surf.intact()
    # host rows, the packed tensor form and the planes apart: the same bits; bgr is rgb with the planes in the other order
    f = pkg.ops.frames_from_nv12_aligned
    assert torch.equal(f(surf.planes, c["net"], c["rows"], channel_order=order, **c["colour"]), got)
    assert torch.equal(f(packed(c["y"], c["uv"]).to(dev), c["net"], c["rows"], channel_order=order, **c["colour"]), got)
    assert torch.equal(f((c["y"].to(dev), c["uv"].to(dev)), c["net"], c["rows"], channel_order="rgb" if bgr else "bgr", **c["colour"]), got.flip(1))
    one = f((surf.y[1], surf.uv[1]), c["net"], c["rows"][1:2], channel_order=order, **c["colour"])                 # one frame, [H,W] planes
    assert torch.equal(one, got[1:2])


def test_way_in_outputs_by_rule_are_the_shift_exactly(pkg, dev):
    """A footprint over the frame's corner, one wholly outside, a NaN row and a scale beyond 16, with a mean and std per channel:
    every output whose footprint misses the frame, and every output of an invalid row, is ``-mean / std`` to the bit."""
    net, N = (16, 16), 4
    y, uv = NC.surface_from_rgb(41, N, H, W)
    rows = torch.tensor([R.rows((35.1, 50.3), 1.3 * 16, 2.0, net), R.rows((20.2, 190.4), 16.0, 0.3, net), [float("nan"), 0, 0, 0], [0.0, 100.0, 3.0, 4.0]],
                        dtype=torch.float64).float()
    mean, std = (0.4, 0.5, 0.6), (0.2, 0.25, 0.3)
    surf = NC.Pitched(y, uv, dev)
    got = pkg.ops.frames_from_nv12_aligned(surf.planes, net, rows.to(dev), mean=mean, std=std).cpu()
    shift = torch.tensor([-m / s for m, s in zip(mean, std)], dtype=torch.float64).float()
    scale = [float(np.float32(1.0 / (255.0 * s))) for s in std]
    want, hit = M.warp_in(y.numpy(), uv.numpy(), rows.numpy(), 16, 16, NC.coeffs()[0], scale=scale, shift=[float(v) for v in shift])
    err = float(np.abs(got.numpy().astype(np.float64) - want).max())
    print(f"way in, outputs by rule: {int((~hit[0]).sum())} of 256 outputs of the corner frame miss it; largest |got - model| = {err:.3e} (bound {TOL_IN}) on "
          f"outputs in ({want.min():.2f}, {want.max():.2f})")
    assert 0 < (~hit[0]).sum() < 256 and not hit[1:].any()
    assert err <= TOL_IN
    miss = torch.from_numpy(~hit)
    for ch in range(3):
        assert (got[:, ch][miss] == shift[ch]).all()
    assert surf.intact()


def test_way_in_grey_surface_has_no_colour(pkg, dev):
    """U = V = 128: R = G = B, spread 0."""
    net = (16, 16)
    y = NC.BC.frames(42, 3, H, W)
    uv = torch.full((3, H // 2, W // 2, 2), 128, dtype=torch.uint8)
    rows = NC.BC.rows_for((0, 1, 2), net)
    for colour in (dict(standard="bt601", full_range=False), dict(standard="bt709", full_range=True)):
        got = pkg.ops.frames_from_nv12_aligned((y.to(dev), uv.to(dev)), net, rows, **colour).cpu()
        spread = float((got.amax(1) - got.amin(1)).max())
        print(f"way in, grey surface, {colour}: largest spread of R, G, B = {spread:.3e}")
        check_in(got, y, uv, rows, net, colour, False, f"grey surface, {colour['standard']}")
        assert spread == 0.0


def test_way_in_whole_frame_is_the_table_form(pkg, dev):
    """c = 0, s = 2, the whole frame: ``ops.frames_from_nv12``, per channel within 2e-6 times the gain of the channel's row."""
    for name in ("generic 601", "matte frames 709"):
        c = NC.case(name)
        planes = (c["y"].to(dev), c["uv"].to(dev))
        N = c["y"].size(0)
        got = pkg.ops.frames_from_nv12_aligned(planes, (H // 2, W // 2), [[2, 0, 0, 0]] * N, **c["colour"])
        want = pkg.ops.frames_from_nv12(planes, (H // 2, W // 2), **c["colour"])
        to_rgb = torch.from_numpy(NC.coeffs(**c["colour"])[0])
        gain = torch.tensor([255 * (2 / 255) * float(to_rgb[ch, :3].abs().sum()) / 2 for ch in range(3)], dtype=torch.float64)
        err = (got.double() - want.double()).abs().amax((0, 2, 3)).cpu()
        print(f"way in, whole frame at s = 2 against frames_from_nv12, {name}: per channel {[f'{float(e):.3e}' for e in err]}, "
              f"bounds {[f'{TOL_TABLE * float(g):.3e}' for g in gain]}")
        assert torch.all(err <= TOL_TABLE * gain)


# ---- out ----------------------------------------------------------------------------------------------------------------------------
def check_out(gy, guv, ref, y0, uv0, tol, what):
    """The bytes of both planes against the model; every byte the model leaves alone is the background, bit for bit."""
    gy, guv, y0, uv0 = (t.cpu().numpy() for t in (gy, guv, y0, uv0))
    ey, euv = float(np.abs(gy - ref["z_y"]).max()), float(np.abs(guv - ref["z_uv"]).max())
    region, touched = ref["region"], ref["touched_uv"]
    zero_y = region & (ref["m"] == 0)
    zero_uv = touched & (M.blocks(ref["m"]).sum(3) == 0)
    print(f"way out, {what}: largest |got - z| = {ey:.6f} (Y), {euv:.6f} (UV) (bound {tol}); region pixels {int(region.sum())}, blocks "
          f"{int(touched.sum())} with {[int((ref['count'] == k).sum()) for k in (1, 2, 3, 4)]} of 1..4 pixels; m = 0 at {int(zero_y.sum())} pixels, "
          f"S = 0 at {int(zero_uv.sum())} blocks")
    assert ref["margin"] >= NC.MARGIN and ey <= tol and euv <= tol
    assert np.array_equal(gy[~region], y0[~region]) and np.array_equal(guv[~touched], uv0[~touched])
    assert np.array_equal(gy[zero_y], y0[zero_y]) and np.array_equal(guv[zero_uv], uv0[zero_uv])
    for n in np.flatnonzero(~ref["valid"]):
        assert np.array_equal(gy[n], y0[n]) and np.array_equal(guv[n], uv0[n])
    assert int((gy != y0).sum()) > 0.2 * int((region & (ref["m"] > 0.1)).sum())          # the region was written
    return zero_y, zero_uv


@pytest.mark.parametrize("name", sorted(NC.SPECS))
def test_way_out_against_the_model(pkg, dev, name):
    """Without colour rows: feathers 0 and 2.5, shared and per-frame mattes with their NaN and out-of-range samples, a NaN row, every
    colour; in place on pitched planes between guard bytes."""
    c, ref = NC.case(name), NC.reference(name)
    x, surf, rows, matte, kw = on(c, dev)
    f = pkg.ops.frames_paste_nv12_aligned
    assert f(x, surf.planes, rows, matte=matte, out=surf.planes, **kw) is surf.planes
    torch.cuda.synchronize()
    zero_y, zero_uv = check_out(surf.y, surf.uv, ref, c["y"], c["uv"], TOL_OUT, name)
    assert surf.intact()
    if c["matte"] is not None:
        assert zero_y.any()
    # bit for bit: host rows (all valid) = device rows; out=None on the packed tensor = in place on pitched planes = another out=;
    # the tensor form = the pair form; a shared matte is that matte for every frame
    whole = packed(c["y"], c["uv"]).to(dev)
    keep = whole.clone()
    got = f(x, whole, rows, matte=matte, **kw)
    gy, guv = pkg.ops.nv12_planes(got)
    assert got.data_ptr() != whole.data_ptr() and torch.equal(whole, keep) and torch.equal(gy, surf.y) and torch.equal(guv, surf.uv)
    if not c["by_rule"]:
        assert torch.equal(f(x, whole, c["rows"], matte=matte, **kw), got)
    pair = (c["y"].to(dev), c["uv"].to(dev))
    other = (torch.zeros_like(pair[0]), torch.zeros_like(pair[1]))
    assert f(x, pair, rows, matte=matte, out=other, **kw) is other and torch.equal(other[0], surf.y) and torch.equal(other[1], surf.uv)
    assert torch.equal(pair[0].cpu(), c["y"]) and torch.equal(pair[1].cpu(), c["uv"])
    if matte is not None and matte.dim() == 2:
        assert torch.equal(f(x, whole, rows, matte=matte.expand(x.size(0), -1, -1).contiguous(), **kw), got)


def test_way_out_regions_over_the_frames_edge(pkg, dev):
    """Regions cut by two edges of the frame and one wholly outside it, a NaN row and a scale beyond 16, matte and feather."""
    net, N = (16, 16), 5
    rows = torch.tensor([R.rows((35.1, 50.3), 1.3 * 16, 2.0, net), R.rows((2.2, 3.9), 2.3 * 16, -0.4, net), R.rows((20.2, 90.4), 16.0, 0.3, net),
                         R.rows((20.3, 27.6), 20.0, 0.3, net), R.rows((20.3, 27.6), 20.0, 0.3, net)], dtype=torch.float64).float()
    rows[3, 0] = float("nan")
    rows[4, :2] = torch.tensor([0.0, 100.0])
    x, matte = NC.BC.source(13, N, *net), NC.BC.matte_for(15, N, *net)
    y, uv = NC.surface_from_rgb(14, N, H, W, "bt709", True)
    to_rgb, from_rgb = NC.coeffs("bt709", True)
    ref = M.paste_out(x.numpy(), y.numpy(), uv.numpy(), rows.numpy(), from_rgb, to_rgb, feather=2.5, matte=matte.numpy(), sums=False)
    surf = NC.Pitched(y, uv, dev)
    pkg.ops.frames_paste_nv12_aligned(x.to(dev), surf.planes, rows.to(dev), feather=2.5, matte=matte.to(dev), standard="bt709", full_range=True,
                                      out=surf.planes)
    torch.cuda.synchronize()
    check_out(surf.y, surf.uv, ref, y, uv, TOL_OUT, "regions over the edge")
    assert surf.intact()
    assert 0 < ref["region"][0].sum() and 0 < ref["region"][1].sum() and not ref["region"][2:].any() and ref["valid"].tolist() == [True] * 3 + [False] * 2
    assert torch.equal(surf.y[2:].cpu(), y[2:]) and torch.equal(surf.uv[2:].cpu(), uv[2:])


@pytest.mark.parametrize("feather", [0, 2.5])
@pytest.mark.parametrize("origin", [(4, 6), (5, 7)])
def test_way_out_integer_box_is_the_table_form(pkg, dev, feather, origin):
    """c = 0, s = 1.5, an even and an odd origin: ``ops.frames_paste_nv12``.  No byte differs by more than one level (the table form
    sums with fp32 weights and fp32 ramps, so a value near a rounding tie may fall to the other side)."""
    S, h = 16, 24
    x = NC.BC.source(18, 3, S, S).to(dev)
    y, uv = NC.surface_from_rgb(19, 3, H, W)
    whole = packed(y, uv).to(dev)
    rows = torch.tensor([[h / S, 0, origin[1], origin[0]]] * 3)
    got = pkg.ops.frames_paste_nv12_aligned(x, whole, rows, feather=feather)
    want = pkg.ops.frames_paste_nv12(x, whole, (*origin, h, h), feather=feather)
    diff = (got.int() - want.int()).abs()
    print(f"way out, integer box at {origin}, feather {feather}: {int((diff > 0).sum())} of {diff.numel()} bytes differ from frames_paste_nv12, "
          f"largest difference {int(diff.max())}; {int((got != whole).sum())} bytes written")
    assert int(diff.max()) <= 1 and int((got != whole).sum()) > 0.5 * 1.5 * h * h * 3


def test_way_out_second_trip_of_the_stride_loop(pkg, dev):
    """An 18 x 18 image at s = 16 into a 288 x 288 surface: 144 x 144 = 20736 chroma blocks against 64 x 256 threads per frame, so
    the end of the frame is pasted in the second trip."""
    S, Hh = 18, 288
    assert (Hh // 2) ** 2 > 64 * 256
    x = NC.BC.source(51, 1, S, S)
    y, uv = NC.surface_from_rgb(52, 1, Hh, Hh)
    rows = torch.tensor([[16.0, 0.0, 0.0, 0.0]])
    to_rgb, from_rgb = NC.coeffs()
    ref = M.paste_out(x.numpy(), y.numpy(), uv.numpy(), rows.numpy(), from_rgb, to_rgb, feather=2.5, sums=False)
    surf = NC.Pitched(y, uv, dev, pitch=320)
    pkg.ops.frames_paste_nv12_aligned(x.to(dev), surf.planes, rows.to(dev), feather=2.5, out=surf.planes)
    torch.cuda.synchronize()
    check_out(surf.y, surf.uv, ref, y, uv, TOL_OUT, "second trip")
    assert surf.intact() and ref["region"].all()
    last = slice(Hh - 32, Hh)                                              # the rows of the second trip
    assert int((surf.y[0, last].cpu() != y[0, last]).sum()) > 0.9 * 32 * Hh


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def check_rows(got, ref, c, what):
    got = got.cpu().numpy().astype(np.float64)
    want = ref["rows"]
    eg = np.abs(got[:, :, 0] - want[:, :, 0]) / want[:, :, 0]
    eo = np.abs(got[:, :, 1] - want[:, :, 1])
    print(f"colour rows, {what}: largest |g - g_ref| / g_ref = {eg.max():.3e} (bound {TOL_G:.3e}), largest |o - o_ref| = {eo.max():.3e} "
          f"(bound {TOL_O:.3e}); gains {want[:, :, 0].min():.3f} .. {want[:, :, 0].max():.3f}")
    assert eg.max() <= TOL_G and eo.max() <= TOL_O
    for n in c["by_rule"]:                                                  # (1, 0) exactly
        assert got[n].tolist() == [[1.0, 0.0]] * 3
    if c["kind"] == "small":                                                # the gain meets max_gain exactly
        assert (got[:, :, 0] == NC.MAX_GAIN).all()
    if c["kind"] == "constant":                                             # var_q = 0: g == 1 exactly
        assert (got[:, :, 0] == 1.0).all()


@pytest.mark.parametrize("name", sorted(NC.SPECS))
def test_colour_rows_against_the_model(pkg, dev, name):
    c, ref = NC.case(name), NC.reference(name)
    x, surf, rows, matte, kw = on(c, dev)
    f = pkg.ops.paste_colour_match_nv12
    got = f(x, surf.planes, rows, matte=matte, **kw)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (x.size(0), 3, 2) and got.is_cuda
    check_rows(got, ref, c, name)
    assert surf.intact() and torch.equal(surf.y.cpu(), c["y"]) and torch.equal(surf.uv.cpu(), c["uv"])      # it reads the surfaces, writes none
    # two calls on the same inputs: the same bits; out= is written and returned
    out = torch.full_like(got, 7.0)
    assert f(x, surf.planes, rows, matte=matte, out=out, **kw) is out and torch.equal(out, got)
    # pitched planes = the packed tensor = the planes apart; host rows (all valid) = device rows
    assert torch.equal(f(x, packed(c["y"], c["uv"]).to(dev), rows, matte=matte, **kw), got)
    assert torch.equal(f(x, (c["y"].to(dev), c["uv"].to(dev)), rows, matte=matte, **kw), got)
    if not c["by_rule"]:
        assert torch.equal(f(x, surf.planes, c["rows"], matte=matte, **kw), got)
    # a frame's row depends on that frame alone
    assert torch.equal(f(x[1:2], (surf.y[1:2], surf.uv[1:2]), rows[1:2], matte=matte if matte is None or matte.dim() == 2 else matte[1:2], **kw),
                       got[1:2])


def test_colour_rows_workspace_guards(pkg, dev):
    """The statistics through the C entry point with a workspace of exactly the size it asks for, between guard bytes; ``colour_out``
    between guard bytes too."""
    lib, L = pkg._lib.lib(), pkg._lib
    c = NC.case("invalid and zero")
    x, surf, rows, matte, kw = on(c, dev)
    N = x.size(0)
    need = lib.spk_paste_colour_match_workspace_bytes(N)
    raw_w = torch.full((256 + need + 256,), 0xA5, dtype=torch.uint8, device=dev)
    raw_c = torch.full((256 + N * 24 + 256,), 0xA5, dtype=torch.uint8, device=dev)
    ws, colour = raw_w[256:256 + need], raw_c[256:256 + N * 24].view(torch.float32).view(N, 3, 2)
    assert ws.data_ptr() % 8 == 0
    L.check(lib.spk_paste_colour_match_nv12_sim(x.data_ptr(), N, *c["net"], surf.y.data_ptr(), surf.y.stride(0), surf.y.stride(1), surf.uv.data_ptr(),
                                                surf.uv.stride(0), surf.uv.stride(1), H, W, rows.data_ptr(), 601, 0, 0.0, -1.0, 127.5,
                                                matte.data_ptr(), N, 2.0, 1.0, 16.0, colour.data_ptr(), ws.data_ptr(), need, L.stream_ptr()),
            "spk_paste_colour_match_nv12_sim")
    torch.cuda.synchronize()
    for raw, n in ((raw_w, need), (raw_c, N * 24)):
        assert bool(torch.all(raw[:256] == 0xA5)) and bool(torch.all(raw[256 + n:] == 0xA5))
    assert surf.intact() and torch.equal(colour, pkg.ops.paste_colour_match_nv12(x, surf.planes, rows, matte=matte, **kw))
    part = ws.view(torch.float64).view(N, -1, 13).cpu()
    assert part.shape[1] == 64 and bool((part[2] == 0).all()) and bool((part[1] == 0).all()) and bool((part[0, :, 0] > 0).any())


@pytest.mark.parametrize("name", ["generic 601", "wide 709", "full range", "gain cap"])
def test_way_out_with_colour_rows_against_the_model(pkg, dev, name):
    """The model is fed the rows the device produced, read back, so this test does not inherit the ulp of the rows."""
    c = NC.case(name)
    x, surf, rows, matte, kw = on(c, dev)
    colour = pkg.ops.paste_colour_match_nv12(x, surf.planes, rows, matte=matte, **kw)
    assert float(colour[:, :, 0].max()) <= 2.0
    pkg.ops.frames_paste_nv12_aligned(x, surf.planes, rows, matte=matte, colour=colour, out=surf.planes, **kw)
    torch.cuda.synchronize()
    ref, plain = NC.model(c, colour.cpu().numpy()), NC.reference(name)
    check_out(surf.y, surf.uv, ref, c["y"], c["uv"], TOL_COLOUR, f"{name}, with colour rows")
    moved = float(np.abs(ref["z_y"] - plain["z_y"]).max())
    print(f"way out with colour rows, {name}: the rows move z_y by up to {moved:.1f}")
    assert surf.intact() and moved > 2.0                                    # the rows did something
    # identity rows and NaN rows change nothing
    whole = packed(c["y"], c["uv"]).to(dev)
    ident = torch.tensor([1.0, 0.0], device=dev).repeat(x.size(0), 3, 1)
    want = pkg.ops.frames_paste_nv12_aligned(x, whole, rows, matte=matte, **kw)
    assert torch.equal(pkg.ops.frames_paste_nv12_aligned(x, whole, rows, matte=matte, colour=ident, **kw), want)
    assert torch.equal(pkg.ops.frames_paste_nv12_aligned(x, whole, rows, matte=matte, colour=ident * float("nan"), **kw), want)


# ---- the clip-level composition of INTEGRATION.md ---------------------------------------------------------------------------------------
SIZE, RES = 128, 32          # encoder input; a 32^2 decoder keeps the case quick, as tests/test_nv12_gpu.py
TEMPLATE5 = [(44.0, 52.0), (84.0, 52.0), (64.0, 74.0), (48.0, 96.0), (80.0, 96.0)]


@pytest.fixture(scope="module")
def irfd(pkg, dev):
    import model
    m = model.IRFD()
    m.Gd.synthesis = pkg.SynthesisNetwork(resolution=RES)
    sd = {k: v for k, v in IR.irfd_recipe_state_dict().items() if not k.startswith("Gd.")}
    sd.update({"Gd." + k: v for k, v in fill_state_dict(m.Gd.state_dict(), prefix="Gd.").items()})
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("D.") for k in missing)
    return m.to(dev).eval()


def test_clip_composition_in_slices_is_one_call(irfd, pkg, dev):
    """Landmarks -> rows -> aligned crops from NV12 -> reenact -> rows scaled to the generated size -> statistics -> paste, for a clip
    of T = 4 surfaces of 48 x 64 with pitch 72: pasting frames [0:2] and [2:4] is pasting the clip, statistics included."""
    ops, T, Hc, Wc = pkg.ops, 4, 48, 64
    true = ops.similarity_rows([(22.3, 31.6), (25.9, 30.2), (23.4, 34.1), (24.1, 29.7)], [30.0, 34.0, 27.0, 31.0], [0.2, -0.3, 0.1, 0.0], SIZE).double()
    t = torch.tensor(TEMPLATE5, dtype=torch.float64)
    lm = torch.stack([torch.stack([r[0] * t[:, 0] - r[1] * t[:, 1] + r[2], r[1] * t[:, 0] + r[0] * t[:, 1] + r[3]], 1) for r in true])
    lm = (lm + 0.3 * torch.randn(lm.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)).float().to(dev)
    rows = ops.smooth_similarity_rows(ops.similarity_from_landmarks(lm, TEMPLATE5), 1)
    y, uv = NC.surface_from_rgb(61, T, Hc, Wc)
    pose = NC.Pitched(y, uv, dev, pitch=72)
    ident = ops.frames_from_u8(NC.BC.frames(62, 56, 72, 3).to(dev), SIZE, channel_order="bgr")
    net = ops.frames_from_nv12_aligned(pose.planes, SIZE, rows)
    assert float(net.std()) > 0.1
    f32 = irfd.reenact(ident, net, net, noises=[n.to(dev) for n in recipe_noises("nv12", T, RES)], chunk=2)
    assert f32.shape == (T, 3, RES, RES)
    gen = rows * torch.tensor([SIZE / RES, SIZE / RES, 1.0, 1.0], device=dev)             # the generated image has 32 pixels where the network's has 128
    matte = ops.ellipse_matte((RES, RES), device=dev)
    colour = ops.paste_colour_match_nv12(f32, pose.planes, gen, matte=matte, feather=2)
    whole = ops.frames_paste_nv12_aligned(f32, pose.planes, gen, matte=matte, colour=colour, feather=2)
    wy, wuv = ops.nv12_planes(whole)
    changed = int((wy.cpu() != y).sum())
    print(f"clip composition: rows {[round(v, 3) for v in rows[0].tolist()]} ...; gains {float(colour[:, :, 0].min()):.3f} .. "
          f"{float(colour[:, :, 0].max()):.3f}; {changed} of {y.numel()} Y bytes pasted")
    assert changed > 0.1 * T * 30 * 30 and pose.intact() and torch.equal(pose.y.cpu(), y)
    for t0 in (0, 2):
        part = (pose.y[t0:t0 + 2], pose.uv[t0:t0 + 2])
        rows_part = ops.paste_colour_match_nv12(f32[t0:t0 + 2], part, gen[t0:t0 + 2], matte=matte, feather=2)
        assert torch.equal(rows_part, colour[t0:t0 + 2])
        assert ops.frames_paste_nv12_aligned(f32[t0:t0 + 2], part, gen[t0:t0 + 2], matte=matte, colour=rows_part, feather=2, out=part) is part
    torch.cuda.synchronize()
    assert torch.equal(pose.y, wy) and torch.equal(pose.uv, wuv) and pose.intact()
