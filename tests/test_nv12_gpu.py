"""GPU checks of the NV12 video edge (csrc/frame_nv12.hip) against the fp64 CPU compositions of tests/nv12_ref.py (written from
the definitions in include/spk.h and checked against a loop per pixel by tests/test_nv12_cpu.py), and of the plan / ``IRFD`` paths
built on it against their hand compositions, bit for bit.

Bounds.  In: per output channel the input bound of tests/test_frame_io_gpu.py, ``(taps_x + taps_y + 8) * 2^-23``, times the gain
``255 |scale_c| sum_j |to_rgb[c][j]| / 2`` over the three linear coefficients of the row (the offset multiplies 1, not a byte that
carries an error; the clamp is 1-Lipschitz): that test's bound is this one for a map of gain 1 into a range of width 2.  Out:
``|got - val| - 0.5 <= 255 * 16 * 2^-23`` on every byte of both planes (the paste bound with identity taps; no row of ``from_rgb``
has an absolute sum above 1, so no gain).  Paste: ``|got - val| - 0.5 <= 255 * (taps_y + taps_x + 16) * 2^-23``.  Every test prints
what it measures.  Measured (MI355X): in, 0.55 - 2.34 x 2^-23 per channel against bounds of 23.7 - 66.8; out, between -3.4e-1 and
-1.1e-4 (eps 4.86e-4); paste, between -1.8e-2 and +4.7e-6 (eps 5.5e-4 .. 9.1e-4); per case in DESIGN.md 4.2c."""
import importlib

import pytest
import torch

import nv12_ref as R
from oracle import irfd_ref as IR
from oracle.weights_recipe import fill_state_dict, recipe_noises

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


def rand_u8(seed, *shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def surface(seed, N, H, W, pitch=None):
    """Random NV12 surfaces on the CPU: [N, 3H/2, W] inside rows of ``pitch`` bytes."""
    return rand_u8(seed, N, 3 * H // 2, pitch or W)[:, :, :W]


def planes(pkg, surf):
    y, uv = pkg.ops.nv12_planes(surf)
    return y.contiguous(), uv.contiguous()


def source(seed, N, S, rng=(-1, 1)):
    x = torch.randn(N, 3, S, S, generator=torch.Generator().manual_seed(seed)) * 0.7
    return x if rng == (-1, 1) else x * 0.5 + 0.5


def taps(pkg, a, b, c, d):
    return pkg.ops.resize_tables(a, c)[2].shape[1] + pkg.ops.resize_tables(b, d)[2].shape[1]


def in_bounds(pkg, h, w, Ho, Wo, to_rgb, scale=(2 / 255,) * 3):
    """Per output channel (R, G, B): the bound of the module docstring."""
    base = (taps(pkg, h, w, Ho, Wo) + 8) * ULP
    return torch.tensor([base * 255 * abs(scale[c]) * float(to_rgb[c, :3].abs().sum()) / 2 for c in range(3)], dtype=torch.float64)


def check_in(pkg, got, ref, h, w, to_rgb, what, size=None):
    Ho, Wo = size or got.shape[2:]
    err = (got.cpu().double() - ref).abs().amax((0, 2, 3))
    bound = in_bounds(pkg, h, w, Ho, Wo, to_rgb)
    print(f"{what}: max-abs error per channel {[round(float(e) / ULP, 2) for e in err]} x 2^-23, bounds {[round(float(b) / ULP, 1) for b in bound]}")
    assert torch.all(err <= bound), (err / ULP, bound / ULP)


# ---- in ---------------------------------------------------------------------------------------------------------------------------
IN_CASES = [(2, 48, 64, 16), (1, 38, 54, 32), (1, 16, 16, 16), (2, 8, 8, 24), (1, 2, 2, 4)]


@pytest.mark.parametrize("N,H,W,size", IN_CASES)
def test_frames_from_nv12_vs_fp64(pkg, dev, N, H, W, size):
    surf = surface(H * 100 + W + N, N, H, W)                             # random bytes: many triples out of gamut, the clamp is active
    to_rgb, _ = pkg.ops.yuv_coeffs()
    got = pkg.ops.frames_from_nv12(surf.to(dev), size)
    assert got.shape == (N, 3, size, size) and got.dtype == torch.float32
    y, uv = planes(pkg, surf)
    ref = R.from_nv12_ref(pkg.ops, y, uv, [(0, 0)] * N, H, W, size, to_rgb)
    clamped = float((ref.abs() == 1).double().mean())
    print(f"  outputs at the clamp: {100 * clamped:.1f} %")
    if size >= min(H, W):                                                # (no averaging: a fifth and more of random triples are out of gamut)
        assert clamped > 0.05
    check_in(pkg, got, ref, H, W, to_rgb, f"frames_from_nv12 {N}x{H}x{W} -> {size}^2")
    assert torch.equal(pkg.ops.frames_from_nv12((y.to(dev), uv.to(dev)), (size, size)), got)        # planes that live apart
    assert torch.equal(pkg.ops.frames_from_nv12(surf.to(dev), size, channel_order="bgr"), got.flip(1))


@pytest.mark.parametrize("standard,full", [("bt709", False), ("bt601", True)])
def test_frames_from_nv12_other_colour(pkg, dev, standard, full):
    N, H, W, size = 1, 38, 54, 32
    surf = surface(7, N, H, W)
    to_rgb, _ = pkg.ops.yuv_coeffs(standard, full)
    got = pkg.ops.frames_from_nv12(surf.to(dev), size, standard=standard, full_range=full)
    y, uv = planes(pkg, surf)
    check_in(pkg, got, R.from_nv12_ref(pkg.ops, y, uv, [(0, 0)], H, W, size, to_rgb), H, W, to_rgb, f"{standard} full={full}")
    assert not torch.equal(got, pkg.ops.frames_from_nv12(surf.to(dev), size))


def test_frames_from_nv12_boxes_and_pitch(pkg, dev):
    """Fixed boxes at odd origins and the far corner of a surface whose pitch exceeds W; tracked origins of mixed parity from a
    host list, a CPU tensor and a device array against single-box calls."""
    N, H, W, h, w, size = 3, 48, 64, 37, 53, 16
    host = surface(11, N, H, W)
    _, dpitched = pitched(dev, host, 72)
    assert dpitched.stride(1) == 72 and not dpitched.is_contiguous()
    y, uv = planes(pkg, host)
    to_rgb, _ = pkg.ops.yuv_coeffs()
    origins = [(1, 1), (0, 3), (H - h, W - w)]
    f = pkg.ops.frames_from_nv12
    for o in origins:
        got = f(dpitched, size, crop=(*o, h, w))
        check_in(pkg, got, R.from_nv12_ref(pkg.ops, y, uv, [o] * N, h, w, size, to_rgb), h, w, to_rgb, f"box at {o}, pitch 72")
        assert torch.equal(got, f(dpitched.contiguous(), size, crop=(*o, h, w)))            # the pitch changes nothing
    singles = torch.cat([f(dpitched[n:n + 1], size, crop=(*origins[n], h, w)) for n in range(N)])
    assert not torch.equal(singles[0], singles[1])
    assert torch.equal(f(dpitched, size, crop=[(*o, h, w) for o in origins]), singles)
    assert torch.equal(f(dpitched, size, crop=torch.tensor([(*o, h, w) for o in origins])), singles)
    yx = torch.tensor(origins, dtype=torch.int32, device=dev)
    assert torch.equal(f(dpitched, size, crop=(yx, h, w)), singles)
    # device origins outside the frame give the result of the clamped origin
    wild = torch.tensor([(-4, W - w + 9), (H - h + 6, -7), (-3, -2)], dtype=torch.int32, device=dev)
    clamped = [(0, W - w), (H - h, 0), (0, 0)]
    assert torch.equal(f(dpitched, size, crop=(wild, h, w)), torch.cat([f(dpitched[n:n + 1], size, crop=(*clamped[n], h, w)) for n in range(N)]))


@pytest.mark.parametrize("H,W,size", [(38, 54, 32), (8, 8, 24)])
def test_constant_and_grey_surfaces(pkg, dev, H, W, size):
    to_rgb, _ = pkg.ops.yuv_coeffs()
    bound = in_bounds(pkg, H, W, size, size, to_rgb)
    const = torch.empty(1, 3 * H // 2, W, dtype=torch.uint8)
    const[:, :H] = 120
    const[:, H:, 0::2], const[:, H:, 1::2] = 100, 150                   # an in-gamut colour: R, G, B = 156.2, 114.3, 64.6
    got = pkg.ops.frames_from_nv12(const.to(dev), size).cpu()
    rgb = to_rgb @ torch.tensor([120.0, 100, 150, 1], dtype=torch.float64)
    assert float(rgb.min()) > 1 and float(rgb.max()) < 254
    for c in range(3):                                                   # the rows of the tables sum to exactly 1: constant in, constant out
        assert float(got[:, c].min()) == float(got[:, c].max())
        assert abs(float(got[0, c, 0, 0]) - (float(rgb[c]) * 2 / 255 - 1)) <= float(bound[c])
    grey = surface(21, 1, H, W).clone()
    grey[:, H:] = 128
    got = pkg.ops.frames_from_nv12(grey.to(dev), size).cpu().double()
    spread = float((got.amax(1) - got.amin(1)).max())
    print(f"grey {H}x{W} -> {size}^2: largest spread of R, G, B {spread / ULP:.2f} x 2^-23, bound {float(bound.min()) / ULP:.1f}")
    assert spread <= float(bound.min())
    y, uv = planes(pkg, grey)
    check_in(pkg, got.float(), R.from_nv12_ref(pkg.ops, y, uv, [(0, 0)], H, W, size, to_rgb), H, W, to_rgb, "grey surface")


def test_frames_from_nv12_second_grid_stride_trip(pkg, dev):
    """2 frames of 192 strips x 1536 columns are 589824 work items against 2048 x 256 threads: the end of the last frame runs in
    the second trip."""
    N, H, W, size = 2, 32, 32, 1536
    assert N * ((size + 7) // 8) * size > 2048 * 256
    surf = surface(31, N, H, W)
    to_rgb, _ = pkg.ops.yuv_coeffs()
    got = pkg.ops.frames_from_nv12(surf.to(dev), size)[-1:].cpu()
    y, uv = planes(pkg, surf)
    ref = R.from_nv12_ref(pkg.ops, y[-1:], uv[-1:], [(0, 0)], H, W, size, to_rgb)
    check_in(pkg, got, ref, H, W, to_rgb, "grid-stride case, last frame")
    check_in(pkg, got[:, :, -8:], ref[:, :, -8:], H, W, to_rgb, "grid-stride case, last rows", (size, size))
    assert float(got[:, :, -8:].std()) > 0.1


# ---- out --------------------------------------------------------------------------------------------------------------------------
def check_out(got_y, got_uv, val_y, val_uv, eps, what):
    over_y = float((got_y.cpu().double() - val_y).abs().max()) - 0.5
    over_uv = float((got_uv.cpu().double() - val_uv).abs().max()) - 0.5
    print(f"{what}: largest |got - val| - 0.5: Y {over_y:+.3e}, UV {over_uv:+.3e}, eps {eps:.3e}")
    assert over_y <= eps and over_uv <= eps


@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (1, 3, 2, 2)])
@pytest.mark.parametrize("rng,standard,full", [((-1, 1), "bt601", False), ((0, 1), "bt601", False), ((-1, 1), "bt709", True)])
def test_frames_to_nv12_vs_fp64(pkg, dev, shape, rng, standard, full):
    x = source(shape[2] + 5, shape[0], shape[2], rng)
    x.view(-1)[0], x.view(-1)[1], x.view(-1)[2] = 5.0, -5.0, float("nan")       # past both range ends, and NaN -> 0
    assert float(x[~x.isnan()].max()) > rng[1] and float(x[~x.isnan()].min()) < rng[0]
    _, from_rgb = pkg.ops.yuv_coeffs(standard, full)
    got = pkg.ops.frames_to_nv12(x.to(dev), value_range=rng, standard=standard, full_range=full)
    N, _, H, W = shape
    assert got.dtype == torch.uint8 and got.shape == (N, 3 * H // 2, W)
    gy, guv = pkg.ops.nv12_planes(got)
    check_out(gy, guv, *R.to_nv12_ref(pkg.ops, x, from_rgb, rng), 255 * 16 * ULP, f"frames_to_nv12 {shape} {rng} {standard} full={full}")


def test_frames_to_nv12_into_a_pitched_surface_and_a_pair(pkg, dev):
    x = source(3, 2, 16).to(dev)
    want = pkg.ops.frames_to_nv12(x)
    raw = torch.full((2, 24, 40), 0xA5, dtype=torch.uint8, device=dev)
    out = raw[:, :, :16]
    assert pkg.ops.frames_to_nv12(x, out=out) is out and torch.equal(out, want)
    assert torch.all(raw[:, :, 16:] == 0xA5)                              # nothing written into the pitch
    py, puv = torch.zeros(2, 16, 16, dtype=torch.uint8, device=dev), torch.zeros(2, 8, 8, 2, dtype=torch.uint8, device=dev)
    pkg.ops.frames_to_nv12(x, out=(py, puv))
    wy, wuv = pkg.ops.nv12_planes(want)
    assert torch.equal(py, wy) and torch.equal(puv, wuv)


# ---- paste ------------------------------------------------------------------------------------------------------------------------
H, W, PITCH = 64, 96, 128


def eps_bytes(pkg, S, h, w):
    return 255.0 * (taps(pkg, S, S, h, w) + 16) * ULP


def pitched(dev, surf, pitch=PITCH, fill=0xA5):
    raw = torch.full((surf.size(0), surf.size(1), pitch), fill, dtype=torch.uint8, device=dev)
    raw[:, :, :surf.size(2)] = surf.to(dev)
    return raw, raw[:, :, :surf.size(2)]


def outside_masks(N, boxes, h, w, Hh=H, Ww=W):
    """Luma pixels outside every box, and chroma samples none of whose four pixels is in the box."""
    my = torch.ones(N, Hh, Ww, dtype=torch.bool)
    for n, (y0, x0) in enumerate(boxes):
        my[n, max(y0, 0):max(min(y0 + h, Hh), 0), max(x0, 0):max(min(x0 + w, Ww), 0)] = False
    muv = my.view(N, Hh // 2, 2, Ww // 2, 2).all(4).all(2)
    return my, muv


@pytest.mark.parametrize("S,h,w", [(16, 37, 53), (32, 9, 11), (32, 32, 32)])
@pytest.mark.parametrize("origin", ["0,0", "1,1", "2,5", "corner"])
def test_paste_nv12_vs_fp64(pkg, dev, S, h, w, origin):
    o = (H - h, W - w) if origin == "corner" else tuple(int(v) for v in origin.split(","))
    N = 2
    x, bg = source(S + h, N, S), surface(h + w, N, H, W)
    by, buv = planes(pkg, bg)
    _, from_rgb = pkg.ops.yuv_coeffs()
    eps = eps_bytes(pkg, S, h, w)
    my, muv = outside_masks(N, [o] * N, h, w)
    for feather in (0, 3, 40):
        raw, dbg = pitched(dev, bg)
        got = pkg.ops.frames_paste_nv12(x.to(dev), dbg, (*o, h, w), feather=feather)
        assert got.dtype == torch.uint8 and got.shape == (N, 3 * H // 2, W) and got.is_contiguous()
        assert torch.equal(dbg.cpu(), bg)                                # without out the input is unchanged
        gy, guv = (t.cpu() for t in pkg.ops.nv12_planes(got))
        check_out(gy, guv, *R.paste_nv12_ref(pkg.ops, x, by, buv, [o] * N, h, w, from_rgb, feather), eps,
                  f"paste {S}^2 -> {h}x{w} at {o}, feather {feather}")
        assert torch.equal(gy[my], by[my]) and torch.equal(guv[muv], buv[muv])          # every byte outside the box is the background
        if feather < 40:
            assert int((gy != by).sum()) > 0.5 * N * h * w
        # in place through the pitch equals the clone, bit for bit; nothing lands in the pitch
        assert pkg.ops.frames_paste_nv12(x.to(dev), dbg, (*o, h, w), feather=feather, out=dbg) is dbg
        assert torch.equal(dbg, got) and torch.all(raw[:, :, W:] == 0xA5)


def test_paste_nv12_whole_frame_is_frames_to_nv12_bit_for_bit(pkg, dev):
    k = torch.arange(255, dtype=torch.float64)
    mid = ((k + 0.5) / 127.5 - 1).float()                                # the rounding ties of the quantiser and their neighbours
    v = torch.cat([mid, torch.nextafter(mid, torch.full_like(mid, 2.0)), torch.nextafter(mid, torch.full_like(mid, -2.0)),
                   torch.tensor([1.0, -1.0, 3.0, -3.0, float("inf"), float("-inf"), -0.0, float("nan")])])
    n = 3 * 4 * 16
    x = torch.cat([v, torch.zeros(-v.numel() % n)]).view(-1, 3, 4, 16).to(dev)
    N = x.size(0)
    for kw in (dict(), dict(value_range=(-2, 2), standard="bt709", full_range=True)):
        want = pkg.ops.frames_to_nv12(x, **kw)
        for seed in (1, 2):                                              # whatever the background holds
            bg = surface(seed, N, 4, 16).to(dev)
            assert torch.equal(pkg.ops.frames_paste_nv12(x, bg, (0, 0, 4, 16), **kw), want)
    x2 = source(5, 1, 2).to(dev)                                        # one chroma block
    assert torch.equal(pkg.ops.frames_paste_nv12(x2, surface(3, 1, 2, 2).to(dev), (0, 0, 2, 2)), pkg.ops.frames_to_nv12(x2))


ORIGINS = [(5, 7), (0, 27), (H - 37, 0)]


def test_paste_nv12_per_frame_origins_and_out(pkg, dev):
    N, S, h, w = 3, 16, 37, 53
    x, bg = source(41, N, S).to(dev), surface(42, N, H, W).to(dev)
    f = pkg.ops.frames_paste_nv12
    singles = torch.cat([f(x[n:n + 1], bg[n:n + 1], (*ORIGINS[n], h, w), feather=3) for n in range(N)])
    assert not torch.equal(singles[0], singles[1])
    assert torch.equal(f(x, bg, [(*o, h, w) for o in ORIGINS], feather=3), singles)
    assert torch.equal(f(x, bg, torch.tensor([(*o, h, w) for o in ORIGINS]), feather=3), singles)
    yx = torch.tensor(ORIGINS, dtype=torch.int32, device=dev)
    assert torch.equal(f(x, bg, (yx, h, w), feather=3), singles)
    keep = bg.clone()
    other = torch.empty_like(bg)
    assert f(x, bg, (yx, h, w), feather=3, out=other) is other and torch.equal(other, singles) and torch.equal(bg, keep)
    pair = tuple(t.clone() for t in pkg.ops.nv12_planes(bg))            # planes that live apart, in place
    assert f(x, pair, (yx, h, w), feather=3, out=pair) is pair
    sy, suv = pkg.ops.nv12_planes(singles)
    assert torch.equal(pair[0], sy) and torch.equal(pair[1], suv)
    assert f(x, bg, (yx, h, w), feather=3, out=bg) is bg and torch.equal(bg, singles)


def test_paste_nv12_skip_rule(pkg, dev):
    """Device boxes over each frame edge, over two at a corner, and wholly outside, the surfaces inside a buffer of sentinel bytes
    whose guards are larger than any overshoot: the visible part equals the clipped reference, a chroma sample with one in-box
    pixel moves by that pixel's quarter weight only, and no other byte changes."""
    S, h, w = 16, 37, 53
    boxes = [(-10, 7), (5, -13), (5, W - 30), (H - 20, 7), (-9, -11), (H - 5, W - 6), (-h, 3), (3, W), (H - 1, W - 1)]
    N = len(boxes)
    rows = 3 * H // 2
    guard = (h + 2) * PITCH + 2 * w + 64
    raw = torch.full((guard + N * rows * PITCH + guard,), 0xA5, dtype=torch.uint8, device=dev)
    view = raw[guard:guard + N * rows * PITCH].view(N, rows, PITCH)[:, :, :W]
    bg = surface(43, N, H, W)
    view.copy_(bg.to(dev))
    x = source(44, N, S)
    yx = torch.tensor(boxes, dtype=torch.int32, device=dev)
    assert pkg.ops.frames_paste_nv12(x.to(dev), view, (yx, h, w), feather=3, out=view) is view
    by, buv = planes(pkg, bg)
    _, from_rgb = pkg.ops.yuv_coeffs()
    gy, guv = planes(pkg, view.cpu())
    val_y, val_uv = R.paste_nv12_ref(pkg.ops, x, by, buv, boxes, h, w, from_rgb, 3)
    check_out(gy, guv, val_y, val_uv, eps_bytes(pkg, S, h, w), "boxes over the frame edges")
    my, muv = outside_masks(N, boxes, h, w)
    assert torch.equal(gy[my], by[my]) and torch.equal(guv[muv], buv[muv])
    assert torch.equal(gy[6], by[6]) and torch.equal(gy[7], by[7]) and torch.equal(guv[6], buv[6]) and torch.equal(guv[7], buv[7])
    for n in (0, 1, 2, 3, 4, 5):
        assert not torch.equal(gy[n], by[n]) and not torch.equal(guv[n], buv[n])
    # frame 8: the box's first pixel alone is in the frame, the last pixel of the last chroma block
    m00 = float(pkg.ops.feather_tables(h, 3)[0] * pkg.ops.feather_tables(w, 3)[0])
    assert int((gy[8] != by[8]).sum()) <= 1 and int((guv[8] != buv[8]).sum()) <= 2
    assert float((guv[8, -1, -1].double() - buv[8, -1, -1].double()).abs().max()) <= 0.25 * m00 * 255 + 0.5
    pad = raw[guard:guard + N * rows * PITCH].view(N, rows, PITCH)[:, :, W:]
    assert torch.all(raw[:guard] == 0xA5) and torch.all(raw[guard + N * rows * PITCH:] == 0xA5) and torch.all(pad == 0xA5)


def test_paste_nv12_second_grid_stride_trip(pkg, dev):
    """3 frames of 421 x 421 chroma blocks are 531723 work items against 2048 x 256 threads: the end of the last frame's box runs
    in the second trip."""
    N, S, h, w, Hh = 3, 16, 840, 840, 848
    assert N * (h // 2 + 1) * (w // 2 + 1) > 2048 * 256
    x, bg = source(49, N, S), surface(50, N, Hh, Hh)
    got = pkg.ops.frames_paste_nv12(x.to(dev), bg.to(dev), (5, 3, h, w), feather=3).cpu()
    by, buv = planes(pkg, bg)
    _, from_rgb = pkg.ops.yuv_coeffs()
    gy, guv = planes(pkg, got)
    val_y, val_uv = R.paste_nv12_ref(pkg.ops, x, by, buv, [(5, 3)] * N, h, w, from_rgb, 3)
    eps = eps_bytes(pkg, S, h, w)
    check_out(gy, guv, val_y, val_uv, eps, "grid-stride case")
    check_out(gy[-1, -64:], guv[-1, -32:], val_y[-1, -64:], val_uv[-1, -32:], eps, "grid-stride case, last rows")
    assert int((gy[-1, -64:-3] != by[-1, -64:-3]).sum()) > 0.9 * 61 * w
    assert torch.equal(gy[:, :5], by[:, :5]) and torch.equal(gy[:, :, :3], by[:, :, :3]) and torch.equal(gy[:, 845:], by[:, 845:])


# ---- plans and the public interface ---------------------------------------------------------------------------------------------
SIZE, RES = 128, 32          # encoder input of the model-level cases; a 32^2 decoder keeps them quick


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


@pytest.fixture(scope="module")
def clip(dev):
    """Identity photo (BGR), T = 3 NV12 surfaces of 48 x 64 with pitch 72, a fixed box at an odd origin, tracked boxes of mixed
    parity, and explicit noise."""
    T = 3
    _, pose = pitched(dev, surface(32, T, 48, 64), 72)
    _, emo = pitched(dev, surface(33, T, 48, 64), 72)
    return dict(T=T, ident_u8=rand_u8(31, 56, 72, 3).to(dev), pose=pose, emo=emo, crop=(3, 5, 40, 44),
                tracked=[(3, 5, 40, 44), (0, 20, 40, 44), (8, 1, 40, 44)], noises=[n.to(dev) for n in recipe_noises("nv12", T, RES)])


def nets(irfd, pkg, c, crop, **colour):
    f = pkg.ops.frames_from_nv12
    return pkg.ops.frames_from_u8(c["ident_u8"], SIZE, channel_order="bgr"), f(c["pose"], SIZE, crop=crop, **colour), \
        f(c["emo"], SIZE, crop=crop, **colour)


def test_reenact_nv12_is_frames_to_nv12_of_reenact(irfd, pkg, clip, dev):
    c = clip
    ident, pose, emo = nets(irfd, pkg, c, c["crop"])
    f32 = irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2)                 # T = 3: one ragged chunk
    assert f32.shape == (c["T"], 3, RES, RES)
    nv = irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2, output="nv12")
    assert nv.dtype == torch.uint8 and nv.shape == (c["T"], 3 * RES // 2, RES) and torch.equal(nv, pkg.ops.frames_to_nv12(f32))
    print(f"nv12 frames: Y mean {float(nv[:, :RES].float().mean()):.1f}, UV mean {float(nv[:, RES:].float().mean()):.1f}, "
          f"{nv.unique().numel()} distinct values")
    nv709 = irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2, output="nv12", standard="bt709", full_range=True)
    assert torch.equal(nv709, pkg.ops.frames_to_nv12(f32, standard="bt709", full_range=True)) and not torch.equal(nv709, nv)
    assert torch.equal(irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2), f32)              # the fp32 plans are as they were
    assert torch.equal(irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2, output="uint8"), pkg.ops.frames_to_u8(f32))


def test_nv12_decoder_plan_is_the_fp32_plan_plus_one_op(irfd, pkg, dev, monkeypatch):
    L = pkg._lib
    Gd = irfd.Gd
    Gd.__dict__.pop("_plans", None)
    feats = torch.randn(2, 6144, generator=torch.Generator().manual_seed(3)).to(dev)
    noises = [n.to(dev) for n in recipe_noises("nv12.plan", 2, RES)]
    y32 = Gd.plan_forward(feats, noises)
    y8 = Gd.plan_forward(feats, noises, output="uint8")
    ys = Gd.plan_forward(feats, seed=5)
    before = [[k for k, _ in p.ops] for p in Gd.__dict__["_plans"].values()]
    ynv = Gd.plan_forward(feats, noises, output="nv12")
    plans = list(Gd.__dict__["_plans"].values())
    assert len(plans) == 4                                                  # side by side
    p32, p8, ps, pnv = plans
    assert (p32.output, p8.output, ps.output, pnv.output) == ("f32", "uint8", "f32", "nv12") and ps.seeded and not pnv.seeded
    k32, k8, ks, knv = ([k for k, _ in p.ops] for p in plans)
    assert [k32, k8, ks] == before                                          # the f32 / uint8 / seeded plans keep their ops
    assert L.OP_FRAMES_TO_NV12 not in k32 + k8 + ks and knv == k32 + [L.OP_FRAMES_TO_NV12] and L.OP_FRAMES_TO_NV12 == 13
    assert k8 == k32 + [L.OP_FRAMES_TO_U8] and ks == [L.OP_NOISE_FILL] + k32
    assert p32.to_nv12 is None and p8.to_nv12 is None and pnv.to_u8 is None
    for (ka, da), (kb, db) in zip(p32.ops, pnv.ops):                        # the same launches: kinds, and for the convs flags and shapes
        if ka == L.OP_CONV2D:
            assert (da.flags, da.B, da.Cin, da.Cout, da.H, da.W, da.config, da.ksplit) == (db.flags, db.B, db.Cin, db.Cout, db.H, db.W, db.config, db.ksplit)
    assert ynv.shape == (2, 3 * RES // 2, RES) and torch.equal(ynv, pkg.ops.frames_to_nv12(y32))
    lib = L.lib()
    names = ("spk_launch_list", "spk_frames_f32_to_nv12", "spk_conv2d_fwd")
    real = {n: getattr(lib, n) for n in names}
    calls = dict.fromkeys(names, 0)

    def counting(name):
        def f(*a):
            calls[name] += 1
            return real[name](*a)
        return f

    for n in names:
        monkeypatch.setattr(lib, n, counting(n))
    again = Gd.plan_forward(feats, noises, output="nv12")
    monkeypatch.undo()
    assert calls == {"spk_launch_list": 1, "spk_frames_f32_to_nv12": 0, "spk_conv2d_fwd": 0}, calls
    assert torch.equal(again, ynv)
    assert torch.equal(Gd.plan_forward(feats, noises), y32) and torch.equal(Gd.plan_forward(feats, noises, output="uint8"), y8)
    assert torch.equal(Gd.plan_forward(feats, seed=5), ys) and len(Gd.__dict__["_plans"]) == 4
    # range and colour are part of the key: a plan of its own each (the cache keeps the four used last)
    y01 = Gd.plan_forward(feats, noises, output="nv12", value_range=(0, 1), standard="bt709")
    p01 = list(Gd.__dict__["_plans"].values())[-1]
    assert p01 is not pnv and p01.output == "nv12" and torch.equal(y01, pkg.ops.frames_to_nv12(y32, value_range=(0, 1), standard="bt709"))
    yfull = Gd.plan_forward(feats, noises, output="nv12", full_range=True)
    pfull = list(Gd.__dict__["_plans"].values())[-1]
    assert pfull is not pnv and pfull is not p01 and torch.equal(yfull, pkg.ops.frames_to_nv12(y32, full_range=True))
    snv = Gd.plan_forward(feats, seed=5, output="nv12")                       # a seeded nv12 plan: the draw first, the conversion last
    assert torch.equal(snv, pkg.ops.frames_to_nv12(ys))


def test_reenact_video_nv12_is_frames_from_nv12_then_reenact(irfd, pkg, clip, dev):
    c = clip
    ident, pose, emo = nets(irfd, pkg, c, c["crop"])
    want = irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2, output="nv12")
    kw = dict(size=SIZE, crop=c["crop"], channel_order="bgr", noises=c["noises"], chunk=2, pixel_format="nv12")
    got = irfd.reenact_video(c["ident_u8"], c["pose"], c["emo"], **kw)
    assert got.dtype == torch.uint8 and got.shape == (c["T"], 3 * RES // 2, RES) and torch.equal(got, want)
    a = irfd.reenact_video(c["ident_u8"], c["pose"], None, **kw)
    b = irfd.reenact_video(c["ident_u8"], c["pose"], c["pose"], **kw)
    assert torch.equal(a, b)
    pair = tuple(t.contiguous() for t in pkg.ops.nv12_planes(c["pose"]))   # planes that live apart
    assert torch.equal(irfd.reenact_video(c["ident_u8"], pair, None, **kw), a)
    colour = dict(standard="bt709", full_range=True)
    i9, p9, e9 = nets(irfd, pkg, c, c["crop"], **colour)
    assert torch.equal(irfd.reenact_video(c["ident_u8"], c["pose"], c["emo"], **kw, **colour),
                       irfd.reenact(i9, p9, e9, noises=c["noises"], chunk=2, output="nv12", **colour))


@pytest.mark.parametrize("which", ["crop", "tracked"])
def test_reenact_video_nv12_paste_is_paste_of_reenact(irfd, pkg, clip, dev, which):
    c = clip
    crop = c[which]
    keep = c["pose"].clone()
    ident, pose, emo = nets(irfd, pkg, c, crop)
    f32 = irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2)
    want = pkg.ops.frames_paste_nv12(f32, c["pose"], crop, feather=4)
    kw = dict(size=SIZE, channel_order="bgr", noises=c["noises"], chunk=2, paste=True, feather=4, pixel_format="nv12")
    got = irfd.reenact_video(c["ident_u8"], c["pose"], c["emo"], crop=crop, **kw)
    assert got.dtype == torch.uint8 and got.shape == (c["T"], 72, 64) and got.is_contiguous() and torch.equal(got, want)
    assert torch.equal(c["pose"], keep) and not torch.equal(got, keep)
    if which == "tracked":                                                  # the same origins from the device
        yx = torch.tensor([b[:2] for b in crop], dtype=torch.int32, device=dev)
        assert torch.equal(irfd.reenact_video(c["ident_u8"], c["pose"], c["emo"], crop=(yx, 40, 44), **kw), want)
    # in place: the pose surfaces, pitch and all, become the result
    raw, video = pitched(dev, keep.cpu(), 72)
    back = irfd.reenact_video(c["ident_u8"], video, c["emo"], crop=crop, inplace=True, **kw)
    assert back is video and torch.equal(video, want) and torch.all(raw[:, :, 64:] == 0xA5)


def test_reenact_video_nv12_paste_chunk_invariance_and_launches(irfd, pkg, clip, dev, monkeypatch):
    """Chunk-invariant under a seed; one ``spk_launch_list`` per encoder / decoder plan plus exactly one ``spk_frames_paste_nv12``
    per chunk, and none of the RGB edge's launches."""
    c, L = clip, pkg._lib
    kw = dict(size=SIZE, channel_order="bgr", paste=True, seed=7, crop=c["tracked"], feather=4, pixel_format="nv12")
    a = irfd.reenact_video(c["ident_u8"], c["pose"], chunk=2, **kw)
    b = irfd.reenact_video(c["ident_u8"], c["pose"], chunk=3, **kw)
    one = irfd.reenact_video(c["ident_u8"], c["pose"], chunk=1, **kw)
    assert torch.equal(a, b) and torch.equal(a, one)
    # crop=None: the box is the whole frame
    whole = irfd.reenact_video(c["ident_u8"], c["pose"], chunk=2, size=SIZE, channel_order="bgr", paste=True, seed=7, pixel_format="nv12")
    f32 = irfd.reenact(pkg.ops.frames_from_u8(c["ident_u8"], SIZE, channel_order="bgr"), pkg.ops.frames_from_nv12(c["pose"], SIZE), chunk=3, seed=7)
    assert torch.equal(whole, pkg.ops.frames_paste_nv12(f32, c["pose"], (0, 0, 48, 64)))
    lib = L.lib()
    names = ("spk_launch_list", "spk_frames_paste_nv12", "spk_frames_f32_to_nv12", "spk_frames_nv12_to_f32", "spk_frames_paste_u8",
             "spk_frames_u8_to_f32_boxes", "spk_conv2d_fwd")
    real = {n: getattr(lib, n) for n in names}
    calls = dict.fromkeys(names, 0)

    def counting(name):
        def f(*args):
            calls[name] += 1
            return real[name](*args)
        return f

    for n in names:
        monkeypatch.setattr(lib, n, counting(n))
    again = irfd.reenact_video(c["ident_u8"], c["pose"], c["emo"], chunk=2, **kw)
    monkeypatch.undo()
    # Ei once, then Ee + Ep + Gd per chunk of T = 3 at chunk 2; the pose and the emotion surfaces through one launch each
    assert calls == {"spk_launch_list": 1 + 2 * 3, "spk_frames_paste_nv12": 2, "spk_frames_f32_to_nv12": 0, "spk_frames_nv12_to_f32": 2,
                     "spk_frames_paste_u8": 0, "spk_frames_u8_to_f32_boxes": 0, "spk_conv2d_fwd": 0}, calls
    assert again.shape == a.shape
    plans = [p for p in irfd.Gd.__dict__["_plans"].values() if p.output == "f32"]
    assert plans and all(L.OP_FRAMES_TO_NV12 not in [k for k, _ in p.ops] and p.to_nv12 is None for p in plans)
