"""GPU checks of the axis-aligned RGB32 edge (csrc/frame_rgb32.hip: ``ops.frames_from_rgb32``, ``ops.frames_to_rgb32``,
``ops.frames_paste_rgb32``), of ``DecoderPlan(output="rgb32")`` and of ``IRFD.reenact(output="rgb32")`` /
``IRFD.reenact_video(pixel_format="rgb32")``.

The chain of trust: rgb24 against fp64 is tests/test_frame_io_gpu.py and tests/test_paste_gpu.py, unchanged; RGB32 against rgb24 is
this file.  An RGB32 frame and the packed frame with the same colour bytes give sums of the same byte values in the same order, so the
criterion is ``torch.equal`` -- of the fp32 BITS (compared as int32) on the way in, of the colour bytes on the way out and in the
paste, against the packed launcher on ``rgb32_cases.packed(frames, order)`` -- and needs no tolerance.  On top of that EVERY fourth
byte, pitch byte and guard byte is what it was, or is ``alpha`` where the way out fills.  One anchor per direction also checks RGB32
against the fp64 references the rgb24 tests use (``resize_ref``, ``quant_ref``, ``paste_ref``), within their bounds, so the suite does
not rest on sibling equality alone.

The frames come from tests/rgb32_cases.py (``Surface``: pitch ``4 W + 16``, 64 guard bytes of 0xA5, fourth bytes random and never
255), which is imported and not edited.  The two forms of the way out and the shapes that reach each: the vector form
(float4 loads, the four words as dword accesses) -- ``(2,3,16,16)`` contiguous and pitched from a 16-aligned base, and a 32 x 44 view
at pixel offset (3, 5) of a 40 x 60 surface (4-aligned, not 16-aligned, W % 4 == 0); the tail form -- ``(1,3,5,7)``, ``(1,3,2,2)``, the
33 x 47 view at (3, 5), and a source one float into a larger buffer."""
import pytest
import torch

import rgb32_cases as RC
from test_frame_io_gpu import ULP, quant_ref, resize_ref, taps
from test_i420_axis_gpu import tie_vector
from test_nv12_gpu import IN_CASES, RES, SIZE, dev, irfd, pkg, rand_u8, source  # noqa: F401
from test_paste_gpu import ORIGINS, H, W, eps_bytes, paste_ref

pytestmark = pytest.mark.gpu
GRID_THREADS = 2048 * 256                                                   # GRID_CAP workgroups of 256 threads: one grid-stride trip


def bits(t):
    return t.view(torch.int32)


class Frames:
    """Random RGB32 frames in ``order`` inside a ``Surface``: ``before`` (the flat CPU buffer), ``flat`` (its copy on the device),
    ``frames`` (the views of ``flat``), ``packed`` (the colour bytes [N,h,w,3] on the device, the rgb24 launchers' input) and
    ``order24``"""

    def __init__(self, dev, seed, order, N, bh, bw, y0=0, x0=0, h=None, w=None):
        self.s, self.order, self.dev = RC.Surface(N, bh, bw, y0, x0, h, w), order, dev
        self.order24 = RC.colour_of(order)[0]
        self.before = self.s.fill(rand_u8(seed, N, bh, bw, 3), order, seed + 1)
        self.fresh()

    def fresh(self):
        self.flat = self.before.to(self.dev)
        self.frames = self.s.view(self.flat)
        return self

    @property
    def packed(self):
        return RC.packed(self.s.view(self.before), self.order).to(self.dev)

    @property
    def alpha(self):
        return RC.fourth(self.s.view(self.before), self.order).to(self.dev)

    def untouched(self):
        return torch.equal(self.flat.cpu(), self.before)

    def outside_intact(self):
        return self.s.outside_intact(self.flat, self.before)


def roi(dev, seed, order, h=33, w=47):
    """The ``h x w`` view at pixel offset (3, 5) of a 40 x 60 surface: its first pixel is 4-aligned and not 16-aligned"""
    f = Frames(dev, seed, order, 1, 40, 60, 3, 5, h, w)
    assert f.frames.data_ptr() % 4 == 0 and f.frames.data_ptr() % 16 != 0 and f.frames.stride(1) == 4 * 60 + 16
    return f


# ---- in ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", RC.ORDERS)
@pytest.mark.parametrize("N,Hh,Ww,size", IN_CASES)
def test_frames_from_rgb32_is_frames_from_u8(pkg, dev, N, Hh, Ww, size, order):
    c = Frames(dev, Hh * 100 + Ww + N, order, N, Hh, Ww)
    f, g = pkg.ops.frames_from_rgb32, pkg.ops.frames_from_u8
    assert c.frames.stride(1) == 4 * Ww + 16 and not c.frames.is_contiguous()            # pitched
    for kw in (dict(), dict(mean=(0.4, 0.5, 0.6), std=(0.2, 0.3, 0.4))):
        want = g(c.packed, size, channel_order=c.order24, **kw)
        got = f(c.frames, size, channel_order=order, **kw)
        assert got.shape == (N, 3, size, size) and got.dtype == torch.float32 and torch.equal(bits(got), bits(want)), kw
    want = g(c.packed, size, channel_order=c.order24)
    assert torch.equal(bits(f(c.frames.contiguous(), size, channel_order=order)), bits(want))        # a contiguous copy
    assert torch.equal(bits(f(c.frames[0], size, channel_order=order)), bits(want[:1]))  # one frame given as [H,W,4]
    wide = torch.zeros(N, Hh, 2 * Ww, 4, dtype=torch.uint8, device=dev)
    wide[:, :, ::2] = c.frames
    strided = wide[:, :, ::2]                                                # a pixel stride of 8: read through a copy
    assert strided.stride(2) == 8 and torch.equal(bits(f(strided, size, channel_order=order)), bits(want))
    swapped = {"rgba": "bgra", "bgra": "rgba", "argb": "abgr", "abgr": "argb"}[order]
    moved = {"rgba": "argb", "bgra": "abgr", "argb": "rgba", "abgr": "bgra"}[order]
    if Hh * Ww >= 64:                                                        # (a 2 x 2 frame may look the same from both ends)
        assert not torch.equal(f(c.frames, size, channel_order=swapped), want) and not torch.equal(f(c.frames, size, channel_order=moved), want)
    assert c.untouched()
    if order in ("bgra", "argb"):                                            # the anchor: RGB32 against the fp64 reference of tests/test_frame_io_gpu.py
        ref = resize_ref(c.packed.cpu(), size, size, bgr=c.order24 == "bgr")
        err = float((f(c.frames, size, channel_order=order).cpu().double() - ref).abs().max())
        t = taps(pkg, Hh, Ww, size, size)
        print(f"frames_from_rgb32 {order} {N}x{Hh}x{Ww} -> {size}^2: max-abs error {err / ULP:.2f} x 2^-23, bound {t + 8} x 2^-23")
        assert err <= (t + 8) * ULP


@pytest.mark.parametrize("order", RC.ORDERS)
def test_frames_from_rgb32_region_of_interest_view(pkg, dev, order):
    c = roi(dev, 21, order)
    want = pkg.ops.frames_from_u8(c.packed, 16, channel_order=c.order24)
    assert torch.equal(bits(pkg.ops.frames_from_rgb32(c.frames, 16, channel_order=order)), bits(want))
    whole = c.s.view(c.flat, whole=True)                                     # the same pixels as a crop of the whole surface
    assert torch.equal(bits(pkg.ops.frames_from_rgb32(whole, 16, crop=(3, 5, 33, 47), channel_order=order)), bits(want))
    assert c.untouched()


@pytest.mark.parametrize("order", ["bgra", "argb"])
def test_frames_from_rgb32_boxes(pkg, dev, order):
    """One box at odd origins and the far corner; per-frame host boxes as a list and as a CPU tensor; device origins; device origins
    outside the frame, which the kernel clamps"""
    N, Hh, Ww, h, w, size = 3, 48, 64, 37, 53, 16
    c = Frames(dev, 11, order, N, Hh, Ww)
    f, g = pkg.ops.frames_from_rgb32, pkg.ops.frames_from_u8
    origins = [(1, 1), (0, 3), (Hh - h, Ww - w)]
    forms = [(*o, h, w) for o in origins] + [[(*o, h, w) for o in origins], torch.tensor([(*o, h, w) for o in origins]),
                                             (torch.tensor(origins, dtype=torch.int32, device=dev), h, w),
                                             (torch.tensor([(-4, Ww - w + 9), (Hh - h + 6, -7), (-3, -2)], dtype=torch.int32, device=dev), h, w)]
    results = []
    for crop in forms:
        want = g(c.packed, size, crop=crop, channel_order=c.order24)
        assert torch.equal(bits(f(c.frames, size, crop=crop, channel_order=order)), bits(want))
        results.append(want)
    assert not torch.equal(results[0], results[1]) and torch.equal(results[3], results[4]) and torch.equal(results[3], results[5])
    clamped = torch.cat([f(c.frames[n:n + 1], size, crop=(*o, h, w), channel_order=order) for n, o in enumerate([(0, Ww - w), (Hh - h, 0), (0, 0)])])
    assert torch.equal(bits(results[6]), bits(clamped)) and c.untouched()


def test_frames_from_rgb32_second_grid_stride_trip(pkg, dev):
    """3 frames of 150 strips x 1200 columns are 540000 work items against 2048 x 256 threads: the end of the last frame runs in the
    second trip"""
    N, S, size = 3, 32, 1200
    assert N * ((size + 7) // 8) * size > GRID_THREADS
    c = Frames(dev, 13, "bgra", N, S, S)
    got = pkg.ops.frames_from_rgb32(c.frames, size, channel_order="bgra")
    want = pkg.ops.frames_from_u8(c.packed, size, channel_order="bgr")
    assert torch.equal(bits(got), bits(want)) and float(got[-1, :, -8:].abs().max()) > 0


# ---- out --------------------------------------------------------------------------------------------------------------------------
def check_out(pkg, x, c, rng=(-1, 1)):
    """``x`` [N,3,h,w] on the device into the frames of ``c``, with ``alpha=200`` and with keep: the colour bytes of ``frames_to_u8``,
    the fourth bytes 200 or as they were, every byte that is no pixel's of the frames intact.  -> the colour bytes"""
    want = pkg.ops.frames_to_u8(x, value_range=rng, channel_order=c.order24)
    for alpha in (200, None):
        out = c.fresh().frames
        assert pkg.ops.frames_to_rgb32(x, value_range=rng, channel_order=c.order, alpha=alpha, out=out) is out
        assert torch.equal(RC.packed(out, c.order), want), (c.order, alpha)
        fourth = RC.fourth(out, c.order)
        assert torch.equal(fourth, c.alpha) if alpha is None else bool((fourth == 200).all()), (c.order, alpha)
        assert c.outside_intact()
    return want


@pytest.mark.parametrize("order", RC.ORDERS)
@pytest.mark.parametrize("rng", [(-1, 1), (0, 1)])
def test_frames_to_rgb32_every_branch(pkg, dev, order, rng):
    ops = pkg.ops
    # the vector form behind a 16-aligned destination: contiguous, and pitched at a pitch and a base that are multiples of 16
    x = source(21, 2, 16, rng).to(dev)
    got = ops.frames_to_rgb32(x, value_range=rng, channel_order=order, alpha=200)
    want = ops.frames_to_u8(x, value_range=rng, channel_order=RC.colour_of(order)[0])
    assert got.dtype == torch.uint8 and got.shape == (2, 16, 16, 4) and got.is_contiguous() and got.data_ptr() % 16 == 0
    assert torch.equal(RC.packed(got, order), want) and bool((RC.fourth(got, order) == 200).all())
    kept = got.clone()
    RC.fourth(kept, order).copy_(torch.randint(0, 255, (2, 16, 16), generator=torch.Generator().manual_seed(3), dtype=torch.uint8))
    was = RC.fourth(kept, order).clone()
    x2 = source(22, 2, 16, rng).to(dev)
    assert ops.frames_to_rgb32(x2, value_range=rng, channel_order=order, alpha=None, out=kept) is kept           # keep, contiguous
    assert torch.equal(RC.packed(kept, order), ops.frames_to_u8(x2, value_range=rng, channel_order=RC.colour_of(order)[0]))
    assert torch.equal(RC.fourth(kept, order), was)
    assert torch.equal(ops.frames_to_rgb32(x, value_range=rng, channel_order=order), ops.frames_to_rgb32(x, value_range=rng, channel_order=order, alpha=255))
    c = Frames(dev, 31, order, 2, 16, 16)
    assert c.frames.data_ptr() % 16 == 0 and c.frames.stride(1) % 16 == 0 and c.frames.stride(0) % 16 == 0 and not c.frames.is_contiguous()
    assert torch.equal(check_out(pkg, x, c, rng), want)
    # the vector form behind a first pixel that is 4-aligned and not 16-aligned (W % 4 == 0)
    check_out(pkg, source(23, 1, 44, rng)[:, :, :32].contiguous().to(dev), roi(dev, 32, order, 32, 44), rng)
    # the tail form: W % 4 != 0 -- the 33 x 47 view, 5 x 7 and 2 x 2
    check_out(pkg, source(24, 1, 47, rng)[:, :, :33].contiguous().to(dev), roi(dev, 33, order), rng)
    check_out(pkg, source(25, 1, 7, rng)[:, :, :5].contiguous().to(dev), Frames(dev, 34, order, 1, 5, 7), rng)
    check_out(pkg, source(26, 1, 2, rng).to(dev), Frames(dev, 35, order, 1, 2, 2), rng)
    # an unaligned source: a view one float into a larger buffer (dword loads without a tail)
    buf = torch.zeros(2 * 3 * 16 * 16 + 1, device=dev)
    xu = buf[1:].view(2, 3, 16, 16)
    xu.copy_(x)
    assert xu.data_ptr() % 16 == 4 and torch.equal(check_out(pkg, xu, Frames(dev, 36, order, 2, 16, 16), rng), want)


@pytest.mark.parametrize("order", ["rgba", "abgr"])
def test_frames_to_rgb32_rounding_ties(pkg, dev, order):
    """The rounding-tie vector of tests/test_i420_axis_gpu.py: ties to even, the range ends, infinities, -0 and NaN -> 0; the anchor of
    the way out: the torch expression of tests/test_frame_io_gpu.py"""
    x = tie_vector(dev)                                                      # [.,3,4,16]
    c = Frames(dev, 41, order, x.size(0), 4, 16)
    colour = check_out(pkg, x, c)
    finite = torch.nan_to_num(x.cpu(), nan=-1.0)                             # NaN -> 0 is the kernel's rule: the reference takes the value that gives 0
    assert torch.equal(colour.cpu(), quant_ref(finite, -1, 1, bgr=c.order24 == "bgr"))
    narrow = x[:, :, :3, :5].contiguous()                                    # the same values through the tail form
    assert torch.equal(check_out(pkg, narrow, Frames(dev, 42, order, x.size(0), 3, 5)), colour[:, :3, :5])


def test_frames_to_rgb32_second_grid_stride_trip(pkg, dev):
    """3 frames of 840 rows of 210 groups are 529200 work items against 2048 x 256 threads"""
    N, S = 3, 840
    assert N * S * ((S + 3) // 4) > GRID_THREADS
    x = source(51, N, S).to(dev)
    got = pkg.ops.frames_to_rgb32(x, channel_order="bgra", alpha=7)
    assert torch.equal(got[..., :3], pkg.ops.frames_to_u8(x, channel_order="bgr")) and bool((got[..., 3] == 7).all())
    assert int(got[-1, -8:, :, :3].max()) > 0


# ---- paste ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,h,w", [(16, 37, 53), (32, 9, 11), (32, 32, 32)])
@pytest.mark.parametrize("origin", ["0,0", "1,1", "2,5", "corner"])
def test_paste_rgb32_is_paste_u8(pkg, dev, S, h, w, origin):
    o = (H - h, W - w) if origin == "corner" else tuple(int(v) for v in origin.split(","))
    N = 2
    f, g = pkg.ops.frames_paste_rgb32, pkg.ops.frames_paste_u8
    x = source(S + h, N, S).to(dev)
    for order in RC.ORDERS:
        c = Frames(dev, h + w, order, N, H, W)
        for feather in (0, 3):
            c.fresh()
            want = g(x, c.packed, (*o, h, w), feather=feather, channel_order=c.order24)
            got = f(x, c.frames, (*o, h, w), feather=feather, channel_order=order)               # out=None: a contiguous clone
            assert got.dtype == torch.uint8 and got.shape == (N, H, W, 4) and got.is_contiguous()
            assert torch.equal(RC.packed(got, order), want) and torch.equal(RC.fourth(got, order), c.alpha) and c.untouched()
            assert int((RC.packed(got, order) != c.packed).sum()) > 0.5 * N * h * w * 3
            other_flat = torch.zeros_like(c.flat)                            # out= a second buffer: it first receives a copy of the frames
            other = c.s.view(other_flat)
            assert f(x, c.frames, (*o, h, w), feather=feather, channel_order=order, out=other) is other
            assert torch.equal(RC.packed(other, order), want) and torch.equal(RC.fourth(other, order), c.alpha) and c.untouched()
            assert c.s.outside_intact(other_flat, torch.zeros_like(c.before))
            assert f(x, c.frames, (*o, h, w), feather=feather, channel_order=order, out=c.frames) is c.frames     # in place through the pitch
            assert torch.equal(RC.packed(c.frames, order), want) and torch.equal(RC.fourth(c.frames, order), c.alpha) and c.outside_intact()
    if (S, h, w) == (16, 37, 53) and origin == "1,1":                        # the anchor: RGB32 (abgr, feather 3) against fp64
        val = paste_ref(x.cpu(), c.packed.cpu(), [o] * N, h, w, 3, (-1, 1), c.order24 == "bgr")
        over = float((RC.packed(c.frames, order).cpu().double() - val).abs().max()) - 0.5
        print(f"paste_rgb32 {order} {S}^2 -> {h}x{w} at {o}, feather 3: largest |got - val| - 0.5 = {over:+.3e}, eps {eps_bytes(pkg, S, h, w):.3e}")
        assert over <= eps_bytes(pkg, S, h, w)


def test_paste_rgb32_per_frame_origins(pkg, dev):
    N, S, h, w = 3, 16, 37, 53
    f, g = pkg.ops.frames_paste_rgb32, pkg.ops.frames_paste_u8
    x = source(41, N, S).to(dev)
    for order in ("bgra", "argb"):
        c = Frames(dev, 42, order, N, H, W)
        yx = torch.tensor(ORIGINS, dtype=torch.int32, device=dev)
        want = g(x, c.packed, (yx, h, w), feather=3, channel_order=c.order24)
        for box in ([(*o, h, w) for o in ORIGINS], torch.tensor([(*o, h, w) for o in ORIGINS]), (yx, h, w)):
            got = f(x, c.frames, box, feather=3, channel_order=order)
            assert torch.equal(RC.packed(got, order), want) and torch.equal(RC.fourth(got, order), c.alpha)
        assert not torch.equal(got[0], f(x, c.frames, (*ORIGINS[1], h, w), feather=3, channel_order=order)[0])
        assert f(x, c.frames, (yx, h, w), feather=3, channel_order=order, out=c.frames) is c.frames
        assert torch.equal(RC.packed(c.frames, order), want) and torch.equal(RC.fourth(c.frames, order), c.alpha) and c.outside_intact()


def test_paste_rgb32_skip_rule(pkg, dev):
    """The nine edge-crossing and outside boxes of ``test_paste_i420_skip_rule``: over each frame edge, over two at a corner, wholly
    outside.  The colour bytes of the packed paste; the wholly-outside frames stay untouched; no byte outside the frames changes"""
    S, h, w = 16, 37, 53
    boxes = [(-10, 7), (5, -13), (5, W - 30), (H - 20, 7), (-9, -11), (H - 5, W - 6), (-h, 3), (3, W), (H - 1, W - 1)]
    N = len(boxes)
    x = source(44, N, S).to(dev)
    for order in ("rgba", "abgr"):
        c = Frames(dev, 43, order, N, H, W)
        yx = torch.tensor(boxes, dtype=torch.int32, device=dev)
        want = pkg.ops.frames_paste_u8(x, c.packed, (yx, h, w), feather=3, channel_order=c.order24)
        assert pkg.ops.frames_paste_rgb32(x, c.frames, (yx, h, w), feather=3, channel_order=order, out=c.frames) is c.frames
        assert torch.equal(RC.packed(c.frames, order), want) and torch.equal(RC.fourth(c.frames, order), c.alpha) and c.outside_intact()
        was = c.s.view(c.before)
        for n in (6, 7):                                                     # wholly outside: untouched
            assert torch.equal(c.frames[n].cpu(), was[n])
        for n in range(6):
            assert not torch.equal(c.frames[n].cpu(), was[n])
        assert int((c.frames[8].cpu() != was[8]).any(-1).sum()) <= 1         # one pixel in the frame


def test_paste_rgb32_second_grid_stride_trip(pkg, dev):
    """3 boxes of 420 x 420 pixels are 529200 work items against 2048 x 256 threads: the end of the last frame's box runs in the second
    trip"""
    N, S, h, w, Hh = 3, 16, 420, 420, 424
    assert N * h * w > GRID_THREADS
    c = Frames(dev, 50, "argb", N, Hh, Hh)
    x = source(49, N, S).to(dev)
    want = pkg.ops.frames_paste_u8(x, c.packed, (2, 1, h, w), feather=3, channel_order="rgb")
    assert pkg.ops.frames_paste_rgb32(x, c.frames, (2, 1, h, w), feather=3, channel_order="argb", out=c.frames) is c.frames
    assert torch.equal(RC.packed(c.frames, "argb"), want) and torch.equal(RC.fourth(c.frames, "argb"), c.alpha) and c.outside_intact()
    assert int((want[-1, -32:-3] != c.packed[-1, -32:-3]).sum()) > 0.9 * 29 * w * 3 * 0.5


# ---- plans and the public interface ---------------------------------------------------------------------------------------------
def test_rgb32_decoder_plan_is_the_fp32_plan_plus_one_op(irfd, pkg, dev, monkeypatch):
    """(The plan cache of a module holds ``plan.MAX_PLANS`` entries, least recently used dropped: the test never counts on more.)"""
    from oracle.weights_recipe import recipe_noises
    L, ops, PL = pkg._lib, pkg.ops, pkg.plan
    Gd = irfd.Gd
    Gd.__dict__.pop("_plans", None)
    cached = lambda: list(Gd.__dict__["_plans"].values())
    kinds_of = lambda p: [k for k, _ in p.ops]
    assert PL.MAX_PLANS >= 4
    feats = torch.randn(2, 6144, generator=torch.Generator().manual_seed(3)).to(dev)
    noises = [n.to(dev) for n in recipe_noises("nv12.plan", 2, RES)]
    y32 = Gd.plan_forward(feats, noises)
    ys = Gd.plan_forward(feats, seed=5)
    yu8 = Gd.plan_forward(feats, noises, output="uint8")
    before = [kinds_of(p) for p in cached()]
    yr = Gd.plan_forward(feats, noises, output="rgb32")
    plans = cached()
    assert len(plans) == 4
    p32, ps, pu8, pr = plans
    assert [p.output for p in plans] == ["f32", "f32", "uint8", "rgb32"] and ps.seeded and not pr.seeded
    k32, ks, ku8, kr = (kinds_of(p) for p in plans)
    assert [k32, ks, ku8] == before                                          # the f32 / seeded / uint8 plans keep their op lists
    assert L.OP_FRAMES_TO_RGB32 == 16 and L.OP_FRAMES_TO_RGB32 not in k32 + ks + ku8 and kr == k32 + [L.OP_FRAMES_TO_RGB32]
    assert ku8 == k32 + [L.OP_FRAMES_TO_U8] and ks[1:] == k32 and ks[0] == L.OP_NOISE_FILL
    assert all(p.to_rgb32 is None for p in plans[:3]) and pr.to_u8 is None and pr.to_nv12 is None and pr.to_i420 is None
    assert yr.shape == (2, RES, RES, 4) and yr.dtype == torch.uint8 and yr.is_contiguous() and torch.equal(yr, ops.frames_to_rgb32(y32))
    assert torch.equal(yr[..., :3], yu8) and bool((yr[..., 3] == 255).all())
    lib = L.lib()
    names = ("spk_launch_list", "spk_frames_f32_to_rgb32", "spk_frames_f32_to_u8", "spk_conv2d_fwd")
    real = {n: getattr(lib, n) for n in names}
    calls = dict.fromkeys(names, 0)

    def counting(name):
        def f(*a):
            calls[name] += 1
            return real[name](*a)
        return f

    for n in names:
        monkeypatch.setattr(lib, n, counting(n))
    again = Gd.plan_forward(feats, noises, output="rgb32")
    monkeypatch.undo()
    assert calls == {"spk_launch_list": 1, "spk_frames_f32_to_rgb32": 0, "spk_frames_f32_to_u8": 0, "spk_conv2d_fwd": 0}, calls
    assert torch.equal(again, yr) and cached()[-1] is pr and len(cached()) == 4
    assert torch.equal(Gd.plan_forward(feats, noises), y32) and torch.equal(Gd.plan_forward(feats, seed=5), ys)      # their bits too
    assert torch.equal(Gd.plan_forward(feats, noises, output="uint8"), yu8) and torch.equal(yu8, ops.frames_to_u8(y32))
    assert {id(p) for p in cached()} == {id(p) for p in plans}               # no plan was rebuilt
    # the NV12 and I420 plans: the op lists and the bits they always had
    ynv = Gd.plan_forward(feats, noises, output="nv12")
    assert kinds_of(cached()[-1]) == k32 + [L.OP_FRAMES_TO_NV12] and cached()[-1].to_rgb32 is None and torch.equal(ynv, ops.frames_to_nv12(y32))
    y420 = Gd.plan_forward(feats, noises, output="i420")
    assert kinds_of(cached()[-1]) == k32 + [L.OP_FRAMES_TO_I420] and cached()[-1].to_rgb32 is None and torch.equal(y420, ops.frames_to_i420(y32))
    # order, alpha and range are part of the key: a plan of its own each
    seen = [pr]
    for kw in (dict(channel_order="abgr"), dict(channel_order="bgra"), dict(alpha=0), dict(channel_order="argb", alpha=17), dict(value_range=(0, 1))):
        y = Gd.plan_forward(feats, noises, output="rgb32", **kw)
        p = cached()[-1]
        assert all(p is not q for q in seen) and p.output == "rgb32" and kinds_of(p) == kr and torch.equal(y, ops.frames_to_rgb32(y32, **kw)), kw
        seen.append(p)
    assert torch.equal(Gd.plan_forward(feats, seed=5, output="rgb32", channel_order="bgra"), ops.frames_to_rgb32(ys, channel_order="bgra"))
    assert kinds_of(cached()[-1]) == ks + [L.OP_FRAMES_TO_RGB32]
    seeds, frames = torch.tensor([5, 9], device=dev), torch.tensor([0, 4], device=dev)
    rows32 = Gd.plan_forward(feats, seed_rows=seeds, frame_rows=frames)
    assert torch.equal(Gd.plan_forward(feats, seed_rows=seeds, frame_rows=frames, output="rgb32", alpha=3), ops.frames_to_rgb32(rows32, alpha=3))


@pytest.fixture(scope="module")
def clip(dev):
    """Identity photo (packed), T = 3 RGB32 frames of 48 x 64 in ``bgra`` at pitch 272 between guards (pose and emotion), a fixed box at
    an odd origin, tracked boxes, transforms for ``align=``"""
    T = 3
    pose, emo = Frames(dev, 32, "bgra", T, 48, 64), Frames(dev, 34, "bgra", T, 48, 64)
    boxes = [(3, 5, 40, 44), (0, 20, 40, 44), (8, 1, 40, 44)]
    return dict(T=T, ident_u8=rand_u8(31, 56, 72, 3).to(dev), pose=pose, emo=emo, crop=boxes[0], tracked=boxes,
                rows=[(0.30, 0.02, 12.0, 4.0), (0.28, -0.03, 20.0, 6.0), (0.32, 0.0, 9.0, 3.0)])


def test_reenact_rgb32_is_reenact_uint8_with_alpha_255(irfd, pkg, clip, dev):
    c = clip
    ident = pkg.ops.frames_from_u8(c["ident_u8"], SIZE, channel_order="bgr")
    pose = pkg.ops.frames_from_rgb32(c["pose"].frames, SIZE, crop=c["crop"], channel_order="bgra")
    f32 = irfd.reenact(ident, pose, seed=7, chunk=2)                         # T = 3: one ragged chunk
    want = irfd.reenact(ident, pose, seed=7, chunk=2, output="uint8", channel_order="bgr")
    got = irfd.reenact(ident, pose, seed=7, chunk=2, output="rgb32", channel_order="bgra")
    assert got.dtype == torch.uint8 and got.shape == (c["T"], RES, RES, 4) and torch.equal(got[..., :3], want) and bool((got[..., 3] == 255).all())
    assert torch.equal(got, pkg.ops.frames_to_rgb32(f32, channel_order="bgra"))
    argb = irfd.reenact(ident, pose, seed=7, chunk=3, output="rgb32", channel_order="argb")
    assert torch.equal(argb[..., 1:], want.flip(-1)) and bool((argb[..., 0] == 255).all())
    with pytest.raises(ValueError, match="channel_order must be one of"):
        irfd.reenact(ident, pose, seed=7, output="rgb32")


@pytest.mark.parametrize("which", ["crop", "tracked"])
def test_reenact_video_rgb32_is_the_rgb24_call_on_the_stripped_clip(irfd, pkg, clip, dev, which):
    c = clip
    pose, emo = c["pose"].fresh(), c["emo"].fresh()
    kw = dict(size=SIZE, crop=c[which], seed=7, chunk=2)
    want = irfd.reenact_video(c["ident_u8"], pose.packed, emo.packed, channel_order="bgr", **kw)
    got = irfd.reenact_video(c["ident_u8"], pose.frames, emo.frames, pixel_format="rgb32", channel_order="bgra", **kw)
    assert got.dtype == torch.uint8 and got.shape == (c["T"], RES, RES, 4) and torch.equal(got[..., :3], want) and bool((got[..., 3] == 255).all())
    none = irfd.reenact_video(c["ident_u8"], pose.frames, None, pixel_format="rgb32", channel_order="bgra", **kw)      # emotion_u8=None: the pose frames
    assert torch.equal(none[..., :3], irfd.reenact_video(c["ident_u8"], pose.packed, None, channel_order="bgr", **kw))
    assert pose.untouched() and emo.untouched()


@pytest.mark.parametrize("which", ["crop", "tracked"])
def test_reenact_video_rgb32_paste(irfd, pkg, clip, dev, which, monkeypatch):
    """``paste=True``: the colour bytes of the rgb24 result, the fourth bytes of the pose clip; chunk 3 against 8; one
    ``spk_frames_paste_rgb32`` call per chunk and none of the packed edge's for the clip; in place into the pitched clip"""
    c, L = clip, pkg._lib
    pose, emo = c["pose"].fresh(), c["emo"].fresh()
    kw = dict(size=SIZE, crop=c[which], seed=7, paste=True, feather=4)
    want = irfd.reenact_video(c["ident_u8"], pose.packed, emo.packed, channel_order="bgr", chunk=3, **kw)
    rgb32 = dict(pixel_format="rgb32", channel_order="bgra")
    got = irfd.reenact_video(c["ident_u8"], pose.frames, emo.frames, chunk=3, **kw, **rgb32)
    assert got.dtype == torch.uint8 and got.shape == (c["T"], 48, 64, 4) and got.is_contiguous()
    assert torch.equal(got[..., :3], want) and torch.equal(got[..., 3], pose.alpha) and not torch.equal(got[..., :3], pose.packed)
    assert pose.untouched()
    assert torch.equal(irfd.reenact_video(c["ident_u8"], pose.frames, emo.frames, chunk=8, **kw, **rgb32), got)       # whatever the chunk
    lib = L.lib()
    names = [n for n in L.exported_symbols() if "frames_" in n]              # every launch of the video edge
    assert "spk_frames_paste_rgb32" in names and "spk_frames_paste_u8" in names and "spk_frames_rgb32_to_f32_boxes" in names
    real = {n: getattr(lib, n) for n in names}
    calls = dict.fromkeys(names, 0)

    def counting(name):
        def f(*args):
            calls[name] += 1
            return real[name](*args)
        return f

    for n in names:
        monkeypatch.setattr(lib, n, counting(n))
    again = irfd.reenact_video(c["ident_u8"], pose.frames, emo.frames, chunk=2, **kw, **rgb32)
    monkeypatch.undo()
    used = {n: k for n, k in calls.items() if k}
    way_in = "spk_frames_rgb32_to_f32" + ("_boxes" if which == "tracked" else "")      # one host box is a slice read in place
    assert used == {"spk_frames_u8_to_f32": 1, way_in: 2, "spk_frames_paste_rgb32": 2}, used         # the photo; pose and emotion; one paste per chunk
    assert torch.equal(again, got)
    # in place: the pitched clip itself becomes the result; a clip whose pixels are not aligned words is refused
    back = irfd.reenact_video(c["ident_u8"], pose.frames, emo.frames, chunk=2, inplace=True, **kw, **rgb32)
    assert back is pose.frames and torch.equal(pose.frames, got) and pose.outside_intact()
    raw = torch.zeros(c["T"] * 48 * 64 * 4 + 1, dtype=torch.uint8, device=dev)
    off = raw[1:].view(c["T"], 48, 64, 4)
    assert off.data_ptr() % 4 == 1
    with pytest.raises(L.SpkError, match="aligned 32-bit words"):
        irfd.reenact_video(c["ident_u8"], off, None, chunk=2, inplace=True, **kw, **rgb32)
    pose.fresh()


def test_reenact_video_rgb32_align_matte_and_colour_match(irfd, pkg, clip, dev):
    """``align=`` rows with a matte, a colour match and a colour window: the colour bytes of the rgb24 call, the fourth bytes intact"""
    c = clip
    pose, emo = c["pose"].fresh(), c["emo"].fresh()
    kw = dict(size=SIZE, align=c["rows"], seed=7, chunk=2, paste=True, feather=2, matte=pkg.ops.ellipse_matte((RES, RES), device=dev),
              colour_match=True, colour_smooth=2)
    want = irfd.reenact_video(c["ident_u8"], pose.packed, emo.packed, channel_order="bgr", **kw)
    got = irfd.reenact_video(c["ident_u8"], pose.frames, emo.frames, pixel_format="rgb32", channel_order="bgra", **kw)
    assert got.shape == (c["T"], 48, 64, 4) and torch.equal(got[..., :3], want) and torch.equal(got[..., 3], pose.alpha)
    assert not torch.equal(got[..., :3], pose.packed) and pose.untouched()
    plain = dict(kw, matte=None, colour_match=False, colour_smooth=0)        # the aligned crop and paste alone, in place, with an aligned photo
    ident_row = [(0.4, 0.0, 8.0, 2.0)]
    want = irfd.reenact_video(c["ident_u8"], pose.packed, None, channel_order="bgr", identity_align=ident_row, **plain)
    back = irfd.reenact_video(c["ident_u8"], pose.frames, None, pixel_format="rgb32", channel_order="bgra", identity_align=ident_row, inplace=True, **plain)
    assert back is pose.frames and torch.equal(RC.packed(back, "bgra"), want) and torch.equal(RC.fourth(back, "bgra"), pose.alpha) and pose.outside_intact()
    pose.fresh()
