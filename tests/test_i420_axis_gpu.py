"""GPU checks of the axis-aligned I420 edge (csrc/frame_i420.hip: ``ops.frames_from_i420``, ``ops.frames_to_i420``,
``ops.frames_paste_i420``), of ``DecoderPlan(output="i420")`` and of ``IRFD.reenact(output="i420")`` /
``IRFD.reenact_video(pixel_format="i420")``.

The chain of trust: NV12 against fp64 is tests/test_nv12_gpu.py, unchanged; I420 against NV12 is this file.  An I420 surface and the
NV12 surface with the same Y bytes and ``UV[cy][cx] = (U[cy][cx], V[cy][cx])`` go through the same kernel templates, so the criterion
is ``torch.equal`` -- of the fp32 tensors on the way in, of the Y, U and V bytes on the way out -- and needs no tolerance.  One anchor
per direction also checks I420 against tests/nv12_ref.py on the interleaved planes, within the bounds of tests/test_nv12_gpu.py (its
``check_in`` / ``check_out``), so the suite does not rest on sibling equality alone.

The surfaces come packed (one contiguous ``[N,3H/2,W]`` tensor) and as a triple of pitched planes between 0xA5 guards
(tests/i420_cases.py: ``Layout``): Y at pitch ``W + 8``; V FIRST and U behind it in one allocation; U at an ODD pitch from an ODD
offset; ``u_row_stride != v_row_stride``.  Every byte that belongs to no plane must stay what it was.  Shapes, boxes, origins, the
model set-up, seeds and the clip are those of tests/test_nv12_gpu.py, imported from it."""
import pytest
import torch

import nv12_ref as R
from i420_cases import GUARD, Layout, Plane, interleave, split
from test_nv12_gpu import (H, IN_CASES, ORIGINS, RES, SIZE, W, check_in, check_out, clip, dev, eps_bytes, irfd, pkg, rand_u8,  # noqa: F401
                           source)

pytestmark = pytest.mark.gpu


def layout_of(N, Hh, Ww):
    """Y at pitch W + 8; V first, U behind it in the same allocation at an odd pitch from an odd offset, its frames an odd number of
    bytes apart; the two chroma pitches differ"""
    ch, cw = Hh // 2, Ww // 2
    up, vp = (cw + 3) | 1, cw + 6
    vplane = Plane(1, GUARD, ch, cw, vp, N, ch * vp)
    uplane = Plane(1, (vplane.end + GUARD) | 1, ch, cw, up, N, (ch * up + 2) | 1)
    lay = Layout([(Plane(0, GUARD, Hh, Ww, Ww + 8, N, Hh * (Ww + 8)), uplane, vplane)])
    assert uplane.offset % 2 == 1 and up % 2 == 1 and up != vp and vplane.offset < uplane.offset
    return lay


class Case:
    """Random surfaces in every form: ``y``, ``u``, ``v`` (CPU, contiguous); ``nv12``: the interleaved pair on the device; ``packed``:
    the contiguous I420 tensor on the device; ``triple()``: fresh pitched planes on the device with their flats"""

    def __init__(self, dev, seed, N, Hh, Ww):
        self.dev, self.N, self.H, self.W = dev, N, Hh, Ww
        self.y, self.u, self.v = rand_u8(seed, N, Hh, Ww), rand_u8(seed + 1, N, Hh // 2, Ww // 2), rand_u8(seed + 2, N, Hh // 2, Ww // 2)
        self.layout = layout_of(N, Hh, Ww)
        self.flats = self.layout.fill([(self.y, self.u, self.v)])

    @property
    def nv12(self):
        return self.y.to(self.dev), interleave(self.u, self.v).to(self.dev)

    @property
    def packed(self):
        return pack((self.y, self.u, self.v)).to(self.dev)

    def triple(self):
        flats = [f.to(self.dev) for f in self.flats]
        return self.layout.planes(flats, 0), flats

    def intact(self, flats):
        return self.layout.rest_intact(flats, self.flats)


def pack(t):
    y, u, v = t
    return torch.cat([p.flatten(1) for p in (y, u, v)], 1).view(y.size(0), 3 * y.size(1) // 2, y.size(2))


def same_bytes(pkg, i420, nv12):
    """An I420 result and an NV12 result hold the same Y, U and V bytes"""
    (y, u, v), (ny, nuv) = pkg.ops.i420_planes(i420), pkg.ops.nv12_planes(nv12)
    return torch.equal(y, ny) and torch.equal(u, nuv[..., 0]) and torch.equal(v, nuv[..., 1])


# ---- in ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Hh,Ww,size", IN_CASES)
def test_frames_from_i420_is_frames_from_nv12(pkg, dev, N, Hh, Ww, size):
    c = Case(dev, Hh * 100 + Ww + N, N, Hh, Ww)
    if (Hh, Ww) == (38, 54):
        assert pkg.ops.i420_planes(c.packed)[1].stride(1) == 27              # a packed plane of an odd width: an odd pitch
    f, g = pkg.ops.frames_from_i420, pkg.ops.frames_from_nv12
    planes, flats = c.triple()
    for kw in (dict(), dict(channel_order="bgr"), dict(standard="bt709", full_range=True), dict(mean=(0.4, 0.5, 0.6), std=(0.2, 0.3, 0.4))):
        want = g(c.nv12, size, **kw)
        got = f(c.packed, size, **kw)
        assert got.shape == (N, 3, size, size) and got.dtype == torch.float32 and torch.equal(got, want), kw
        assert torch.equal(f(planes, size, **kw), want), kw
    assert not torch.equal(g(c.nv12, size, standard="bt709", full_range=True), g(c.nv12, size))
    assert c.intact(flats)
    to_rgb, _ = pkg.ops.yuv_coeffs()                                         # the anchor: I420 against fp64 on the interleaved planes
    ref = R.from_nv12_ref(pkg.ops, c.y, interleave(c.u, c.v), [(0, 0)] * N, Hh, Ww, size, to_rgb)
    check_in(pkg, f(planes, size), ref, Hh, Ww, to_rgb, f"frames_from_i420 {N}x{Hh}x{Ww} -> {size}^2, pitched triple")


def test_frames_from_i420_boxes(pkg, dev):
    """Fixed boxes at odd origins and the far corner; tracked origins of mixed parity from a host list, a CPU tensor and a device
    array; device origins outside the frame, which the kernel clamps"""
    N, Hh, Ww, h, w, size = 3, 48, 64, 37, 53, 16
    c = Case(dev, 11, N, Hh, Ww)
    f, g = pkg.ops.frames_from_i420, pkg.ops.frames_from_nv12
    planes, _ = c.triple()
    origins = [(1, 1), (0, 3), (Hh - h, Ww - w)]
    forms = [(*o, h, w) for o in origins] + [[(*o, h, w) for o in origins], torch.tensor([(*o, h, w) for o in origins]),
                                             (torch.tensor(origins, dtype=torch.int32, device=dev), h, w),
                                             (torch.tensor([(-4, Ww - w + 9), (Hh - h + 6, -7), (-3, -2)], dtype=torch.int32, device=dev), h, w)]
    results = []
    for crop in forms:
        want = g(c.nv12, size, crop=crop)
        assert torch.equal(f(c.packed, size, crop=crop), want) and torch.equal(f(planes, size, crop=crop), want)
        results.append(want)
    assert not torch.equal(results[0], results[1]) and torch.equal(results[3], results[4]) and torch.equal(results[3], results[5])
    assert torch.equal(results[6], torch.cat([g(tuple(t[n:n + 1] for t in c.nv12), size, crop=(*o, h, w))
                                              for n, o in enumerate([(0, Ww - w), (Hh - h, 0), (0, 0)])]))


# ---- out --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (1, 3, 2, 2)])
@pytest.mark.parametrize("rng,standard,full", [((-1, 1), "bt601", False), ((0, 1), "bt601", False), ((-1, 1), "bt709", True)])
def test_frames_to_i420_is_the_split_of_frames_to_nv12(pkg, dev, shape, rng, standard, full):
    x = source(shape[2] + 5, shape[0], shape[2], rng)
    x.view(-1)[0], x.view(-1)[1], x.view(-1)[2] = 5.0, -5.0, float("nan")
    kw = dict(value_range=rng, standard=standard, full_range=full)
    N, _, Hh, Ww = shape
    got = pkg.ops.frames_to_i420(x.to(dev), **kw)
    assert got.dtype == torch.uint8 and got.shape == (N, 3 * Hh // 2, Ww) and got.is_contiguous()
    assert same_bytes(pkg, got, pkg.ops.frames_to_nv12(x.to(dev), **kw))
    c = Case(dev, 3, N, Hh, Ww)                                              # into a pitched triple: guards and pitch bytes intact
    planes, flats = c.triple()
    assert pkg.ops.frames_to_i420(x.to(dev), out=planes, **kw) is planes
    assert torch.equal(pack(planes), got) and c.intact(flats)
    _, from_rgb = pkg.ops.yuv_coeffs(standard, full)                         # the anchor
    gy, gu, gv = pkg.ops.i420_planes(got)
    check_out(gy, interleave(gu, gv), *R.to_nv12_ref(pkg.ops, x, from_rgb, rng), 255 * 16 * 2.0 ** -23, f"frames_to_i420 {shape} {rng} {standard}")


def tie_vector(dev):
    k = torch.arange(255, dtype=torch.float64)
    mid = ((k + 0.5) / 127.5 - 1).float()                                    # the rounding ties of the quantiser and their neighbours
    v = torch.cat([mid, torch.nextafter(mid, torch.full_like(mid, 2.0)), torch.nextafter(mid, torch.full_like(mid, -2.0)),
                   torch.tensor([1.0, -1.0, 3.0, -3.0, float("inf"), float("-inf"), -0.0, float("nan")])])
    n = 3 * 4 * 16
    return torch.cat([v, torch.zeros(-v.numel() % n)]).view(-1, 3, 4, 16).to(dev)


def test_rounding_ties_and_whole_frame_paste_is_frames_to_i420(pkg, dev):
    x = tie_vector(dev)
    N = x.size(0)
    for kw in (dict(), dict(value_range=(-2, 2), standard="bt709", full_range=True)):
        want = pkg.ops.frames_to_i420(x, **kw)
        assert same_bytes(pkg, want, pkg.ops.frames_to_nv12(x, **kw))
        for seed in (1, 2):                                                  # whatever the background holds
            assert torch.equal(pkg.ops.frames_paste_i420(x, Case(dev, seed, N, 4, 16).packed, (0, 0, 4, 16), **kw), want)
    x2 = source(5, 1, 2).to(dev)                                             # one chroma block
    assert torch.equal(pkg.ops.frames_paste_i420(x2, Case(dev, 3, 1, 2, 2).packed, (0, 0, 2, 2)), pkg.ops.frames_to_i420(x2))


# ---- paste ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,h,w", [(16, 37, 53), (32, 9, 11), (32, 32, 32)])
@pytest.mark.parametrize("origin", ["0,0", "1,1", "2,5", "corner"])
def test_paste_i420_is_paste_nv12(pkg, dev, S, h, w, origin):
    o = (H - h, W - w) if origin == "corner" else tuple(int(v) for v in origin.split(","))
    N = 2
    c = Case(dev, h + w, N, H, W)
    x = source(S + h, N, S).to(dev)
    for feather in (0, 3, 40):
        want = pkg.ops.frames_paste_nv12(x, c.nv12, (*o, h, w), feather=feather)
        packed = c.packed
        got = pkg.ops.frames_paste_i420(x, packed, (*o, h, w), feather=feather)
        assert got.dtype == torch.uint8 and got.shape == (N, 3 * H // 2, W) and got.is_contiguous() and same_bytes(pkg, got, want)
        assert torch.equal(packed, c.packed)                                 # without out the input is unchanged
        if feather < 40:
            assert int((pkg.ops.i420_planes(got)[0] != pkg.ops.i420_planes(packed)[0]).sum()) > 0.5 * N * h * w
        planes, flats = c.triple()
        assert torch.equal(pkg.ops.frames_paste_i420(x, planes, (*o, h, w), feather=feather), got)       # one packed clone of a triple
        assert all(torch.equal(a.cpu(), b) for a, b in zip(planes, (c.y, c.u, c.v)))
        assert pkg.ops.frames_paste_i420(x, planes, (*o, h, w), feather=feather, out=planes) is planes   # in place through the pitches
        assert torch.equal(pack(planes), got) and c.intact(flats)
    if (S, h, w) == (16, 37, 53) and origin == "1,1":                        # the anchor: I420 against fp64 on the interleaved planes
        _, from_rgb = pkg.ops.yuv_coeffs()
        gy, gu, gv = (t.cpu() for t in pkg.ops.i420_planes(got))
        val = R.paste_nv12_ref(pkg.ops, x.cpu(), c.y, interleave(c.u, c.v), [o] * N, h, w, from_rgb, 40)
        check_out(gy, interleave(gu, gv), *val, eps_bytes(pkg, S, h, w), f"paste_i420 {S}^2 -> {h}x{w} at {o}, feather 40")


def test_paste_i420_per_frame_origins_and_out(pkg, dev):
    N, S, h, w = 3, 16, 37, 53
    c = Case(dev, 42, N, H, W)
    x = source(41, N, S).to(dev)
    f = pkg.ops.frames_paste_i420
    yx = torch.tensor(ORIGINS, dtype=torch.int32, device=dev)
    want = pkg.ops.frames_paste_nv12(x, c.nv12, (yx, h, w), feather=3)
    bg = c.packed
    for box in ([(*o, h, w) for o in ORIGINS], torch.tensor([(*o, h, w) for o in ORIGINS]), (yx, h, w)):
        assert same_bytes(pkg, f(x, bg, box, feather=3), want)
    assert not torch.equal(f(x, bg, (yx, h, w), feather=3)[0], f(x, bg, (*ORIGINS[1], h, w), feather=3)[0])
    other = torch.empty_like(bg)
    assert f(x, bg, (yx, h, w), feather=3, out=other) is other and same_bytes(pkg, other, want) and torch.equal(bg, c.packed)
    planes, flats = c.triple()                                               # out= a pitched triple: it first receives a copy
    assert f(x, bg, (yx, h, w), feather=3, out=planes) is planes and same_bytes(pkg, planes, want) and c.intact(flats)
    assert f(x, bg, (yx, h, w), feather=3, out=bg) is bg and same_bytes(pkg, bg, want)


def test_paste_i420_skip_rule(pkg, dev):
    """The nine edge-crossing boxes of ``test_paste_nv12_skip_rule`` -- over each frame edge, over two at a corner, wholly outside --
    give chroma blocks with 1 to 4 in-box pixels: the same bytes as the NV12 paste, and no byte outside the planes changes"""
    S, h, w = 16, 37, 53
    boxes = [(-10, 7), (5, -13), (5, W - 30), (H - 20, 7), (-9, -11), (H - 5, W - 6), (-h, 3), (3, W), (H - 1, W - 1)]
    N = len(boxes)
    c = Case(dev, 43, N, H, W)
    x = source(44, N, S).to(dev)
    yx = torch.tensor(boxes, dtype=torch.int32, device=dev)
    want = pkg.ops.frames_paste_nv12(x, c.nv12, (yx, h, w), feather=3)
    planes, flats = c.triple()
    assert pkg.ops.frames_paste_i420(x, planes, (yx, h, w), feather=3, out=planes) is planes
    assert same_bytes(pkg, planes, want) and c.intact(flats)
    assert same_bytes(pkg, pkg.ops.frames_paste_i420(x, c.packed, (yx, h, w), feather=3), want)
    for n in (6, 7):                                                         # wholly outside: untouched
        assert all(torch.equal(p[n].cpu(), q[n]) for p, q in zip(planes, (c.y, c.u, c.v)))
    for n in range(6):
        assert not torch.equal(planes[0][n].cpu(), c.y[n]) and not torch.equal(planes[1][n].cpu(), c.u[n])
    assert int((planes[0][8].cpu() != c.y[8]).sum()) <= 1 and int((planes[1][8].cpu() != c.u[8]).sum()) <= 1      # one pixel in the frame


def test_paste_i420_second_grid_stride_trip(pkg, dev):
    """3 frames of 421 x 421 chroma blocks are 531723 work items against 2048 x 256 threads: the end of the last frame's box runs in
    the second trip.  The reference is the NV12 launcher on the GPU."""
    N, S, h, w, Hh = 3, 16, 840, 840, 848
    assert N * (h // 2 + 1) * (w // 2 + 1) > 2048 * 256
    c = Case(dev, 50, N, Hh, Hh)
    x = source(49, N, S).to(dev)
    want = pkg.ops.frames_paste_nv12(x, c.nv12, (5, 3, h, w), feather=3)
    got = pkg.ops.frames_paste_i420(x, c.packed, (5, 3, h, w), feather=3)
    assert same_bytes(pkg, got, want)
    gy = pkg.ops.i420_planes(got)[0]
    assert int((gy[-1, -64:-3].cpu() != c.y[-1, -64:-3]).sum()) > 0.9 * 61 * w


# ---- YV12 -------------------------------------------------------------------------------------------------------------------------
def test_yv12_is_the_same_call_with_the_planes_swapped(pkg, dev):
    """A YV12 buffer holds V where I420 holds U: its planes given as ``(y, second, first)`` are the I420 surface"""
    N, S, h, w = 2, 16, 37, 53
    c = Case(dev, 61, N, H, W)
    x = source(62, N, S).to(dev)
    y, first, second = pkg.ops.i420_planes(pack((c.y, c.v, c.u)).to(dev))    # V in front of U in memory
    assert first.data_ptr() < second.data_ptr() and torch.equal(first.cpu(), c.v)
    yv12 = (y, second, first)
    assert torch.equal(pkg.ops.frames_from_i420(yv12, 16, crop=(1, 3, h, w)), pkg.ops.frames_from_i420(c.packed, 16, crop=(1, 3, h, w)))
    want = pkg.ops.frames_paste_i420(x, c.packed, (1, 3, h, w), feather=3)
    assert pkg.ops.frames_paste_i420(x, yv12, (1, 3, h, w), feather=3, out=yv12) is yv12
    wy, wu, wv = pkg.ops.i420_planes(want)
    assert torch.equal(y, wy) and torch.equal(second, wu) and torch.equal(first, wv)
    out = torch.empty(N, 3 * H // 2, W, dtype=torch.uint8, device=dev)
    oy, ofirst, osecond = pkg.ops.i420_planes(out)
    x3 = source(63, N, W)[:, :, :H].contiguous().to(dev)                     # [N,3,H,W]
    pkg.ops.frames_to_i420(x3, out=(oy, osecond, ofirst))
    ty, tu, tv = pkg.ops.i420_planes(pkg.ops.frames_to_i420(x3))
    assert torch.equal(oy, ty) and torch.equal(osecond, tu) and torch.equal(ofirst, tv)


# ---- plans and the public interface ---------------------------------------------------------------------------------------------
def test_i420_decoder_plan_is_the_fp32_plan_plus_one_op(irfd, pkg, dev, monkeypatch):
    from oracle.weights_recipe import recipe_noises
    L = pkg._lib
    Gd = irfd.Gd
    Gd.__dict__.pop("_plans", None)
    feats = torch.randn(2, 6144, generator=torch.Generator().manual_seed(3)).to(dev)
    noises = [n.to(dev) for n in recipe_noises("nv12.plan", 2, RES)]
    y32 = Gd.plan_forward(feats, noises)
    ys = Gd.plan_forward(feats, seed=5)
    ynv = Gd.plan_forward(feats, noises, output="nv12")
    before = [[k for k, _ in p.ops] for p in Gd.__dict__["_plans"].values()]
    yi = Gd.plan_forward(feats, noises, output="i420")
    plans = list(Gd.__dict__["_plans"].values())
    assert len(plans) == 4
    p32, ps, pnv, pi = plans
    assert (p32.output, ps.output, pnv.output, pi.output) == ("f32", "f32", "nv12", "i420") and ps.seeded and not pi.seeded
    k32, ks, knv, ki = ([k for k, _ in p.ops] for p in plans)
    assert [k32, ks, knv] == before                                          # the f32 / seeded / nv12 plans keep their ops
    assert L.OP_FRAMES_TO_I420 == 15 and L.OP_FRAMES_TO_I420 not in k32 + ks + knv and ki == k32 + [L.OP_FRAMES_TO_I420]
    assert p32.to_i420 is None and pnv.to_i420 is None and pi.to_nv12 is None and pi.to_u8 is None
    assert yi.shape == (2, 3 * RES // 2, RES) and yi.dtype == torch.uint8 and torch.equal(yi, pkg.ops.frames_to_i420(y32))
    assert same_bytes(pkg, yi, ynv)
    lib = L.lib()
    names = ("spk_launch_list", "spk_frames_f32_to_i420", "spk_frames_f32_to_nv12", "spk_conv2d_fwd")
    real = {n: getattr(lib, n) for n in names}
    calls = dict.fromkeys(names, 0)

    def counting(name):
        def f(*a):
            calls[name] += 1
            return real[name](*a)
        return f

    for n in names:
        monkeypatch.setattr(lib, n, counting(n))
    again = Gd.plan_forward(feats, noises, output="i420")
    monkeypatch.undo()
    assert calls == {"spk_launch_list": 1, "spk_frames_f32_to_i420": 0, "spk_frames_f32_to_nv12": 0, "spk_conv2d_fwd": 0}, calls
    assert torch.equal(again, yi) and len(Gd.__dict__["_plans"]) == 4
    assert torch.equal(Gd.plan_forward(feats, noises), y32) and torch.equal(Gd.plan_forward(feats, seed=5), ys)      # their bits too
    assert torch.equal(Gd.plan_forward(feats, noises, output="nv12"), ynv)
    assert torch.equal(Gd.plan_forward(feats, noises, output="uint8"), pkg.ops.frames_to_u8(y32))
    # range and colour are part of the key: a plan of its own each
    y01 = Gd.plan_forward(feats, noises, output="i420", value_range=(0, 1), standard="bt709")
    p01 = list(Gd.__dict__["_plans"].values())[-1]
    assert p01 is not pi and p01.output == "i420" and torch.equal(y01, pkg.ops.frames_to_i420(y32, value_range=(0, 1), standard="bt709"))
    yfull = Gd.plan_forward(feats, noises, output="i420", full_range=True)
    pfull = list(Gd.__dict__["_plans"].values())[-1]
    assert pfull is not pi and pfull is not p01 and torch.equal(yfull, pkg.ops.frames_to_i420(y32, full_range=True))
    assert torch.equal(Gd.plan_forward(feats, seed=5, output="i420"), pkg.ops.frames_to_i420(ys))      # seeded: the draw first, the conversion last
    seeds, frames = torch.tensor([5, 9], device=dev), torch.tensor([0, 4], device=dev)
    rows32 = Gd.plan_forward(feats, seed_rows=seeds, frame_rows=frames)
    assert torch.equal(Gd.plan_forward(feats, seed_rows=seeds, frame_rows=frames, output="i420"), pkg.ops.frames_to_i420(rows32))


def as_i420(pkg, nv12):
    """The NV12 clip of tests/test_nv12_gpu.py as a contiguous packed I420 tensor"""
    y, uv = pkg.ops.nv12_planes(nv12)
    return pack((y, *split(uv)))


def clip_triple(pkg, dev, packed):
    """A packed clip as a triple of pitched planes between guards -> (planes, flats, layout, the CPU flats before)"""
    y, u, v = (t.cpu() for t in pkg.ops.i420_planes(packed))
    lay = layout_of(*y.shape)
    before = lay.fill([(y, u, v)])
    flats = [f.to(dev) for f in before]
    return lay.planes(flats, 0), flats, lay, before


def test_reenact_i420_is_frames_to_i420_of_reenact(irfd, pkg, clip, dev):
    c = clip
    f = pkg.ops.frames_from_nv12
    ident, pose, emo = pkg.ops.frames_from_u8(c["ident_u8"], SIZE, channel_order="bgr"), f(c["pose"], SIZE, crop=c["crop"]), f(c["emo"], SIZE, crop=c["crop"])
    f32 = irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2)
    got = irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2, output="i420")
    assert got.dtype == torch.uint8 and got.shape == (c["T"], 3 * RES // 2, RES) and torch.equal(got, pkg.ops.frames_to_i420(f32))
    assert same_bytes(pkg, got, irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2, output="nv12"))
    colour = dict(standard="bt709", full_range=True)
    got709 = irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2, output="i420", **colour)
    assert torch.equal(got709, pkg.ops.frames_to_i420(f32, **colour)) and not torch.equal(got709, got)


@pytest.mark.parametrize("which", ["crop", "tracked"])
def test_reenact_video_i420_is_the_split_of_the_nv12_result(irfd, pkg, clip, dev, which):
    c = clip
    pose, emo = as_i420(pkg, c["pose"]), as_i420(pkg, c["emo"])
    triple = clip_triple(pkg, dev, pose)[0]
    for extra in (dict(), dict(standard="bt709", full_range=True)):
        kw = dict(size=SIZE, crop=c[which], channel_order="bgr", noises=c["noises"], chunk=2, **extra)
        want = irfd.reenact_video(c["ident_u8"], c["pose"], c["emo"], pixel_format="nv12", **kw)
        got = irfd.reenact_video(c["ident_u8"], pose, emo, pixel_format="i420", **kw)
        assert got.dtype == torch.uint8 and got.shape == (c["T"], 3 * RES // 2, RES) and same_bytes(pkg, got, want)
        assert torch.equal(irfd.reenact_video(c["ident_u8"], triple, emo, pixel_format="i420", **kw), got)
        none = irfd.reenact_video(c["ident_u8"], pose, None, pixel_format="i420", **kw)                  # emotion_u8=None: the pose frames
        assert torch.equal(none, irfd.reenact_video(c["ident_u8"], pose, pose, pixel_format="i420", **kw))
        assert same_bytes(pkg, none, irfd.reenact_video(c["ident_u8"], c["pose"], None, pixel_format="nv12", **kw))


@pytest.mark.parametrize("which", ["crop", "tracked"])
def test_reenact_video_i420_paste_is_paste_of_reenact(irfd, pkg, clip, dev, which):
    c = clip
    crop = c[which]
    pose, emo = as_i420(pkg, c["pose"]), as_i420(pkg, c["emo"])
    keep = pose.clone()
    g = pkg.ops.frames_from_i420
    ident = pkg.ops.frames_from_u8(c["ident_u8"], SIZE, channel_order="bgr")
    f32 = irfd.reenact(ident, g(pose, SIZE, crop=crop), g(emo, SIZE, crop=crop), noises=c["noises"], chunk=2)
    want = pkg.ops.frames_paste_i420(f32, pose, crop, feather=4)
    kw = dict(size=SIZE, channel_order="bgr", noises=c["noises"], chunk=2, paste=True, feather=4)
    got = irfd.reenact_video(c["ident_u8"], pose, emo, crop=crop, pixel_format="i420", **kw)
    assert got.dtype == torch.uint8 and got.shape == (c["T"], 72, 64) and got.is_contiguous() and torch.equal(got, want)
    assert torch.equal(pose, keep) and not torch.equal(got, keep)
    assert same_bytes(pkg, got, irfd.reenact_video(c["ident_u8"], c["pose"], c["emo"], crop=crop, pixel_format="nv12", **kw))
    if which == "tracked":                                                   # the same origins from the device
        yx = torch.tensor([b[:2] for b in crop], dtype=torch.int32, device=dev)
        assert torch.equal(irfd.reenact_video(c["ident_u8"], pose, emo, crop=(yx, 40, 44), pixel_format="i420", **kw), want)
    # in place: a packed tensor, then the decoder's own pitched planes, become the result
    video = keep.clone()
    assert irfd.reenact_video(c["ident_u8"], video, emo, crop=crop, inplace=True, pixel_format="i420", **kw) is video and torch.equal(video, want)
    planes, flats, lay, before = clip_triple(pkg, dev, keep)
    back = irfd.reenact_video(c["ident_u8"], planes, emo, crop=crop, inplace=True, pixel_format="i420", **kw)
    assert back is planes and torch.equal(pack(planes), want) and lay.rest_intact(flats, before)


def test_reenact_video_i420_paste_chunk_invariance_and_launches(irfd, pkg, clip, dev, monkeypatch):
    """Chunk-invariant under a seed; ``crop=None`` is the whole frame; exactly one ``spk_frames_paste_i420`` per chunk and none of the
    NV12 or RGB edge's launches"""
    c, L = clip, pkg._lib
    pose, emo = as_i420(pkg, c["pose"]), as_i420(pkg, c["emo"])
    kw = dict(size=SIZE, channel_order="bgr", paste=True, seed=7, crop=c["tracked"], feather=4, pixel_format="i420")
    a = irfd.reenact_video(c["ident_u8"], pose, chunk=2, **kw)
    assert torch.equal(a, irfd.reenact_video(c["ident_u8"], pose, chunk=3, **kw)) and torch.equal(a, irfd.reenact_video(c["ident_u8"], pose, chunk=1, **kw))
    whole = irfd.reenact_video(c["ident_u8"], pose, chunk=2, size=SIZE, channel_order="bgr", paste=True, seed=7, pixel_format="i420")
    f32 = irfd.reenact(pkg.ops.frames_from_u8(c["ident_u8"], SIZE, channel_order="bgr"), pkg.ops.frames_from_i420(pose, SIZE), chunk=3, seed=7)
    assert torch.equal(whole, pkg.ops.frames_paste_i420(f32, pose, (0, 0, 48, 64)))
    lib = L.lib()
    names = [n for n in L._PROTOTYPES if "frames_" in n] + ["spk_launch_list", "spk_conv2d_fwd"]        # every launch of the video edge
    assert "spk_frames_paste_nv12" in names and "spk_frames_paste_u8" in names and "spk_frames_u8_to_f32_boxes" in names
    real = {n: getattr(lib, n) for n in names}
    calls = dict.fromkeys(names, 0)

    def counting(name):
        def f(*args):
            calls[name] += 1
            return real[name](*args)
        return f

    for n in names:
        monkeypatch.setattr(lib, n, counting(n))
    again = irfd.reenact_video(c["ident_u8"], pose, emo, chunk=2, **kw)
    monkeypatch.undo()
    used = {n: k for n, k in calls.items() if k}
    # the identity photo is packed RGB; the pose and the emotion surfaces through one launch each; Ei once, then Ee + Ep + Gd per chunk
    assert used == {"spk_frames_u8_to_f32": 1, "spk_frames_i420_to_f32": 2, "spk_frames_paste_i420": 2, "spk_launch_list": 1 + 2 * 3}, used
    assert again.shape == a.shape
