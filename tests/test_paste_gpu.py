"""GPU checks of the full-frame way out of the video edge (csrc/frame_io.hip): ``ops.frames_paste_u8`` against an fp64 CPU
composition of torch's ``interpolate(antialias=True)``, the quantiser and the feather blend; bit for bit against
``ops.frames_to_u8`` where the paste is one; per-frame origins from the host and from the device; the skip rule inside an owned
guard buffer; ``ops.frames_from_u8`` with tracked boxes; ``IRFD.reenact_video(paste=True)`` against its hand composition.

Error bound of the paste, in byte units: ``0.5 + 255 * (taps_y + taps_x + 16) * 2^-23`` on every pixel -- half a step for the
final rounding, and for the value in front of it the dot-product bound of the input test (fp32-rounded weights, a separable sum)
plus the fp32 roundings of ``v``, of ``(v - lo) * k`` and of the two feather factors, in byte units (a value range maps to 255).
Measured (MI355X), largest ``|got - val| - 0.5`` over the ten cases: between -2.1e-3 and exactly 0 (a tie of the fp64 value,
rounded to even) against bounds of 5.5e-4 .. 9.1e-4; per case in DESIGN.md 4.2a."""
import importlib

import pytest
import torch
import torch.nn.functional as F

from oracle import irfd_ref as IR
from oracle.weights_recipe import fill_state_dict, recipe_noises

pytestmark = pytest.mark.gpu
H, W = 64, 80                       # the background frames


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


def frames(seed, *shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def source(seed, N, S, rng=(-1, 1)):
    """Generated frames: most values inside ``rng``, some beyond both ends."""
    x = torch.randn(N, 3, S, S, generator=torch.Generator().manual_seed(seed)) * 0.7
    return x if rng == (-1, 1) else x * 0.5 + 0.5


def feather_ref(n, feather):
    i = torch.arange(n, dtype=torch.float64)
    return torch.minimum(torch.ones(n, dtype=torch.float64), (torch.minimum(i, n - 1 - i) + 1) / (feather + 1.0))


def paste_ref(x, bg, boxes, h, w, feather=0, rng=(-1, 1), bgr=False):
    """fp64 on the CPU -> the unrounded value of every byte of the frames (the background outside the boxes).  ``boxes``: one
    ``(y0, x0)`` per frame; the part of a box outside the frame is clipped."""
    lo, hi = rng
    v = F.interpolate(x.double(), size=(h, w), mode="bilinear", align_corners=False, antialias=True)
    q = ((v - lo) * (255.0 / (hi - lo))).clamp(0, 255)
    if bgr:
        q = q.flip(1)
    q = q.permute(0, 2, 3, 1)
    m = (feather_ref(h, feather).view(h, 1) * feather_ref(w, feather).view(1, w)).view(h, w, 1)
    val = bg.double().clone()
    Hh, Ww = bg.shape[1:3]
    for n, (y0, x0) in enumerate(boxes):
        ya, yb, xa, xb = max(y0, 0), min(y0 + h, Hh), max(x0, 0), min(x0 + w, Ww)
        if ya >= yb or xa >= xb:
            continue
        b = val[n, ya:yb, xa:xb]
        val[n, ya:yb, xa:xb] = b + m[ya - y0:yb - y0, xa - x0:xb - x0] * (q[n, ya - y0:yb - y0, xa - x0:xb - x0] - b)
    return val


def eps_bytes(pkg, S, h, w):
    taps = pkg.ops.resize_tables(S, h)[2].shape[1] + pkg.ops.resize_tables(S, w)[2].shape[1]
    return 255.0 * (taps + 16) * 2.0 ** -23


def outside_mask(N, boxes, h, w, Hh=H, Ww=W):
    m = torch.ones(N, Hh, Ww, dtype=torch.bool)
    for n, (y0, x0) in enumerate(boxes):
        m[n, max(y0, 0):max(min(y0 + h, Hh), 0), max(x0, 0):max(min(x0 + w, Ww), 0)] = False
    return m


# S, h, w, N, origin, feather, bgr, value range
PASTE_CASES = [
    (16, 37, 53, 3, (5, 7), 0, False, (-1, 1)),          # enlarging, odd box, odd byte address
    (16, 37, 53, 3, (5, 7), 3, True, (-1, 1)),
    (16, 37, 53, 1, (0, 0), 40, False, (-1, 1)),         # a feather wider than half the box; the first pixel of the frame
    (16, 37, 53, 3, (H - 37, W - 53), 3, False, (0, 1)),  # the last pixel of the frame
    (32, 9, 11, 3, (20, 33), 0, False, (-1, 1)),         # shrinking
    (32, 9, 11, 1, (H - 9, W - 11), 3, True, (0, 1)),
    (32, 9, 11, 3, (0, 0), 40, False, (-1, 1)),
    (32, 32, 32, 3, (7, 9), 0, False, (-1, 1)),          # same size
    (32, 32, 32, 3, (7, 9), 3, True, (-1, 1)),
    (32, 32, 32, 1, (H - 32, W - 32), 40, False, (0, 1)),
]


@pytest.mark.parametrize("S,h,w,N,origin,feather,bgr,rng", PASTE_CASES)
def test_paste_vs_fp64_composition(pkg, dev, S, h, w, N, origin, feather, bgr, rng):
    x, bg = source(S * 100 + h + N, N, S, rng), frames(h * 10 + N, N, H, W, 3)
    got = pkg.ops.frames_paste_u8(x.to(dev), bg.to(dev), (*origin, h, w), feather=feather, value_range=rng,
                                  channel_order="bgr" if bgr else "rgb")
    assert got.dtype == torch.uint8 and got.shape == (N, H, W, 3)
    val = paste_ref(x, bg, [origin] * N, h, w, feather, rng, bgr)
    over = float((got.cpu().double() - val).abs().max()) - 0.5
    eps = eps_bytes(pkg, S, h, w)
    print(f"paste {N}x{S}^2 -> {h}x{w} at {origin}, feather {feather}, {'bgr' if bgr else 'rgb'}, range {rng}: "
          f"largest |got - val| - 0.5 = {over:+.3e}, eps {eps:.3e}")
    assert over <= eps
    outside = outside_mask(N, [origin] * N, h, w)
    assert torch.equal(got.cpu()[outside], bg[outside])               # every byte outside the box is the background
    if feather < 40:                                                     # and the box was written (feather 40: weights down to 6e-4)
        assert int((got.cpu() != bg).sum()) > 0.5 * N * h * w * 3


# ---- bit for bit: a paste over the whole frame at the same size without a feather is the quantiser -----------------------------
def tie_grid():
    """Every rounding tie of the (-1, 1) range -- the fp32 nearest (k + 0.5) / 127.5 - 1 and its two neighbours, k = 0..254 --
    and the range ends, values beyond them, infinities and -0."""
    k = torch.arange(255, dtype=torch.float64)
    mid = ((k + 0.5) / 127.5 - 1).float()
    vals = [mid, torch.nextafter(mid, torch.full_like(mid, 2.0)), torch.nextafter(mid, torch.full_like(mid, -2.0)),
            torch.tensor([1.0, -1.0, 1.0000001, -1.0000001, 3.0, -3.0, float("inf"), float("-inf"), -0.0])]
    return torch.cat(vals)


@pytest.mark.parametrize("shape", [(4, 16), (3, 5)])
def test_whole_frame_paste_is_frames_to_u8_bit_for_bit(pkg, dev, shape):
    v = tie_grid()
    n = 3 * shape[0] * shape[1]
    x = torch.cat([v, torch.zeros(-v.numel() % n)]).view(-1, 3, *shape).to(dev)
    x[-1, 0, 0, 0] = float("nan")                                        # NaN -> 0 in both
    N = x.size(0)
    want = pkg.ops.frames_to_u8(x)
    for seed in (1, 2):                                                  # whatever the background holds
        bg = frames(seed, N, *shape, 3).to(dev)
        assert torch.equal(pkg.ops.frames_paste_u8(x, bg, (0, 0, *shape)), want)
    assert torch.equal(pkg.ops.frames_paste_u8(x, bg, (0, 0, *shape), channel_order="bgr"), pkg.ops.frames_to_u8(x, channel_order="bgr"))
    x01 = x * 0.5 + 0.5
    assert torch.equal(pkg.ops.frames_paste_u8(x01, bg, (0, 0, *shape), value_range=(0, 1)), pkg.ops.frames_to_u8(x01, value_range=(0, 1)))


# ---- per-frame origins ----------------------------------------------------------------------------------------------------------
ORIGINS = [(5, 7), (0, 27), (H - 37, 0)]


def test_per_frame_origins_from_host_and_device(pkg, dev):
    N, S, h, w = 3, 16, 37, 53
    x, bg = source(41, N, S).to(dev), frames(42, N, H, W, 3).to(dev)
    singles = torch.cat([pkg.ops.frames_paste_u8(x[n:n + 1], bg[n:n + 1], (*ORIGINS[n], h, w), feather=3) for n in range(N)])
    assert not torch.equal(singles[0], singles[1])
    host = pkg.ops.frames_paste_u8(x, bg, [(*o, h, w) for o in ORIGINS], feather=3)
    assert torch.equal(host, singles)
    assert torch.equal(pkg.ops.frames_paste_u8(x, bg, torch.tensor([(*o, h, w) for o in ORIGINS]), feather=3), singles)
    yx = torch.tensor(ORIGINS, dtype=torch.int32, device=dev)
    assert torch.equal(pkg.ops.frames_paste_u8(x, bg, (yx, h, w), feather=3), singles)


def test_skip_rule_keeps_every_store_inside_the_frame(pkg, dev):
    """Device boxes partly (and wholly) outside the frame, the frames inside a larger buffer of sentinel bytes whose guards are
    larger than any overshoot: the visible part equals the clipped reference and no other byte of the buffer changes."""
    S, h, w = 16, 37, 53
    boxes = [(-10, 7), (5, -13), (5, W - 30), (-9, -11), (H - 5, W - 6), (-h, 3), (3, W), (5, 7), (H - 20, 7)]
    N = len(boxes)
    # a kernel without the rule would store up to h rows before the first frame (box 5) and after the last, and up to w pixels
    # past a row's end: the guards own more than that on both sides, so a wrong store lands in the buffer and shows below
    guard = ((h + 1) * 3 * W + 3 * w + 64) | 1
    raw = torch.full((guard + N * H * W * 3 + guard,), 0xA5, dtype=torch.uint8, device=dev)
    bg = frames(43, N, H, W, 3)
    view = raw[guard:guard + N * H * W * 3].view(N, H, W, 3)
    assert view.data_ptr() % 2 == 1
    view.copy_(bg.to(dev))
    x = source(44, N, S)
    yx = torch.tensor(boxes, dtype=torch.int32, device=dev)
    out = pkg.ops.frames_paste_u8(x.to(dev), view, (yx, h, w), feather=3, out=view)
    assert out.data_ptr() == view.data_ptr()
    got = view.cpu()
    val = paste_ref(x, bg, boxes, h, w, 3)
    assert float((got.double() - val).abs().max()) - 0.5 <= eps_bytes(pkg, S, h, w)
    outside = outside_mask(N, boxes, h, w)
    assert torch.equal(got[outside], bg[outside])
    assert torch.equal(got[5], bg[5]) and torch.equal(got[6], bg[6])                  # boxes wholly outside
    for n in (0, 1, 2, 3, 4, 7, 8):
        assert not torch.equal(got[n], bg[n])
    assert torch.all(raw[:guard] == 0xA5) and torch.all(raw[guard + N * H * W * 3:] == 0xA5)


def test_in_place_and_out(pkg, dev):
    N, S, h, w = 3, 16, 37, 53
    x, bg = source(45, N, S).to(dev), frames(46, N, H, W, 3).to(dev)
    keep = bg.clone()
    cloned = pkg.ops.frames_paste_u8(x, bg, (5, 7, h, w), feather=3)
    assert torch.equal(bg, keep) and cloned.data_ptr() != bg.data_ptr()              # without out the input is unchanged
    other = torch.empty_like(bg)
    assert pkg.ops.frames_paste_u8(x, bg, (5, 7, h, w), feather=3, out=other) is other and torch.equal(other, cloned)
    assert torch.equal(bg, keep)
    assert pkg.ops.frames_paste_u8(x, bg, (5, 7, h, w), feather=3, out=bg) is bg
    assert torch.equal(bg, cloned)


def test_strided_background_is_written_through_its_strides(pkg, dev):
    N, S, h, w = 3, 16, 20, 24
    big = frames(47, N, H + 9, W + 13, 3).to(dev)
    keep = big.clone()
    part = big[:, 4:4 + H, 5:5 + W]
    assert not part.is_contiguous() and part.data_ptr() % 2 == 1
    x = source(48, N, S).to(dev)
    want = pkg.ops.frames_paste_u8(x, part.contiguous(), (30, 40, h, w), feather=2)
    assert pkg.ops.frames_paste_u8(x, part, (30, 40, h, w), feather=2, out=part) is part
    assert torch.equal(part, want)
    rest = torch.ones(N, H + 9, W + 13, dtype=torch.bool)
    rest[:, 34:34 + h, 45:45 + w] = False
    assert torch.equal(big.cpu()[rest], keep.cpu()[rest])
    # a strided background without out: read in place, the result is a packed clone
    fresh = keep[:, 4:4 + H, 5:5 + W]
    got = pkg.ops.frames_paste_u8(x, fresh, (30, 40, h, w), feather=2)
    assert got.is_contiguous() and torch.equal(got, want)


def test_paste_second_grid_stride_trip(pkg, dev):
    """The launch is capped at 2048 workgroups of 256 threads, a thread per box pixel: 8 boxes of 264 x 256 are 540672 work
    items, so the last 16384 (the last 64 rows of the last frame's box) run in the second trip."""
    N, S, h, w = 8, 16, 264, 256
    assert N * h * w > 2048 * 256
    x, bg = source(49, N, S), frames(50, N, h + 3, w + 2, 3)
    got = pkg.ops.frames_paste_u8(x.to(dev), bg.to(dev), (3, 2, h, w), feather=3).cpu()
    val = paste_ref(x, bg, [(3, 2)] * N, h, w, 3)
    eps = eps_bytes(pkg, S, h, w)
    assert float((got.double() - val).abs().max()) - 0.5 <= eps
    assert float((got[-1, -64:].double() - val[-1, -64:]).abs().max()) - 0.5 <= eps
    assert int((got[-1, -64:] != bg[-1, -64:]).sum()) > 0.9 * 64 * w * 3
    assert torch.equal(got[:, :3], bg[:, :3]) and torch.equal(got[:, :, :2], bg[:, :, :2])


# ---- tracked boxes on the way in ------------------------------------------------------------------------------------------------
def test_frames_from_u8_with_tracked_boxes(pkg, dev):
    N, h, w = 3, 37, 53
    u = frames(51, N, H, W, 3).to(dev)
    f = pkg.ops.frames_from_u8
    singles = torch.cat([f(u[n:n + 1], 16, crop=(*ORIGINS[n], h, w), channel_order="bgr") for n in range(N)])
    assert not torch.equal(singles[0], singles[1])
    assert torch.equal(f(u, 16, crop=[(*o, h, w) for o in ORIGINS], channel_order="bgr"), singles)
    assert torch.equal(f(u, 16, crop=torch.tensor([(*o, h, w) for o in ORIGINS]), channel_order="bgr"), singles)
    yx = torch.tensor(ORIGINS, dtype=torch.int32, device=dev)
    assert torch.equal(f(u, 16, crop=(yx, h, w), channel_order="bgr"), singles)
    # a strided view of a larger frame, and a non-square target
    big = frames(52, N, H + 9, W + 13, 3).to(dev)
    part = big[:, 4:4 + H, 5:5 + W]
    assert torch.equal(f(part, (16, 24), crop=(yx, h, w)), torch.cat([f(part[n:n + 1], (16, 24), crop=(*ORIGINS[n], h, w)) for n in range(N)]))
    # device origins outside the frame give the result of the clamped origin
    wild = torch.tensor([(-4, W - w + 9), (H - h + 6, -7), (-3, -2)], dtype=torch.int32, device=dev)
    clamped = [(0, W - w), (H - h, 0), (0, 0)]
    assert torch.equal(f(u, 16, crop=(wild, h, w)), torch.cat([f(u[n:n + 1], 16, crop=(*clamped[n], h, w)) for n in range(N)]))


# ---- the public interface -------------------------------------------------------------------------------------------------------
SIZE = 128          # encoder input of the model-level cases, as tests/test_frame_io_gpu.py


@pytest.fixture(scope="module")
def irfd(dev):
    import model
    m = model.IRFD()
    sd = IR.irfd_recipe_state_dict()
    sd.update({"Gd." + k: v for k, v in fill_state_dict(m.Gd.state_dict(), prefix="Gd.").items()})
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("D.") for k in missing)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def clip(dev):
    """Identity photo, T = 3 BGR video frames of 48 x 64, a fixed box, tracked boxes of the same size, and explicit noise."""
    T = 3
    return dict(T=T, ident_u8=frames(31, 56, 72, 3).to(dev), pose_u8=frames(32, T, 48, 64, 3).to(dev), emo_u8=frames(33, T, 48, 64, 3).to(dev),
                crop=(3, 5, 40, 44), tracked=[(3, 5, 40, 44), (0, 20, 40, 44), (8, 0, 40, 44)],
                noises=[n.to(dev) for n in recipe_noises("frame_io", T, 256)])


@pytest.mark.parametrize("which", ["crop", "tracked"])
def test_reenact_video_paste_is_paste_of_reenact(irfd, pkg, clip, dev, which):
    c, f = clip, pkg.ops.frames_from_u8
    crop = c[which]
    keep = c["pose_u8"].clone()
    ident, pose, emo = f(c["ident_u8"], SIZE, channel_order="bgr"), f(c["pose_u8"], SIZE, crop=crop, channel_order="bgr"), \
        f(c["emo_u8"], SIZE, crop=crop, channel_order="bgr")
    f32 = irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2)
    want = pkg.ops.frames_paste_u8(f32, c["pose_u8"], crop, feather=4, channel_order="bgr")
    got = irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], size=SIZE, crop=crop, channel_order="bgr", noises=c["noises"],
                             chunk=2, paste=True, feather=4)
    assert got.dtype == torch.uint8 and got.shape == (c["T"], 48, 64, 3) and torch.equal(got, want)
    assert torch.equal(c["pose_u8"], keep) and got.data_ptr() != c["pose_u8"].data_ptr()
    assert not torch.equal(got, keep)
    if which == "tracked":                                                  # the same origins from the device
        yx = torch.tensor([b[:2] for b in crop], dtype=torch.int32, device=dev)
        assert torch.equal(irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], size=SIZE, crop=(yx, 40, 44), channel_order="bgr",
                                              noises=c["noises"], chunk=2, paste=True, feather=4), want)
    # in place: the pose frames become the result
    video = c["pose_u8"].clone()
    back = irfd.reenact_video(c["ident_u8"], video, c["emo_u8"], size=SIZE, crop=crop, channel_order="bgr", noises=c["noises"], chunk=2,
                              paste=True, feather=4, inplace=True)
    assert back is video and torch.equal(video, want)


def test_reenact_video_paste_whole_frame_and_chunk_invariance(irfd, pkg, clip, dev):
    c = clip
    kw = dict(size=SIZE, channel_order="bgr", paste=True, seed=7)
    a = irfd.reenact_video(c["ident_u8"], c["pose_u8"], chunk=2, crop=c["tracked"], feather=4, **kw)
    b = irfd.reenact_video(c["ident_u8"], c["pose_u8"], chunk=3, crop=c["tracked"], feather=4, **kw)
    assert torch.equal(a, b)
    # crop=None: the box is the whole frame, the result is the generated frame at the video's size
    whole = irfd.reenact_video(c["ident_u8"], c["pose_u8"], chunk=2, **kw)
    f32 = irfd.reenact(pkg.ops.frames_from_u8(c["ident_u8"], SIZE, channel_order="bgr"),
                       pkg.ops.frames_from_u8(c["pose_u8"], SIZE, channel_order="bgr"), chunk=3, seed=7)
    assert torch.equal(whole, pkg.ops.frames_paste_u8(f32, c["pose_u8"], (0, 0, 48, 64), channel_order="bgr"))


def test_reenact_video_paste_launches(irfd, pkg, clip, dev, monkeypatch):
    """One ``spk_launch_list`` per encoder / decoder plan as without the paste, plus exactly one ``spk_frames_paste_u8`` per chunk;
    the fp32 decoder plan keeps its ops and ``paste=False`` its result."""
    c, L = clip, pkg._lib
    args = (c["ident_u8"], c["pose_u8"], c["emo_u8"])
    kw = dict(size=SIZE, crop=c["tracked"], channel_order="bgr", noises=c["noises"], chunk=2)
    plain = irfd.reenact_video(*args, **kw)                                 # warm: every plan is built
    pasted = irfd.reenact_video(*args, paste=True, feather=4, **kw)
    lib = L.lib()
    names = ("spk_launch_list", "spk_frames_paste_u8", "spk_frames_f32_to_u8", "spk_frames_u8_to_f32_boxes", "spk_conv2d_fwd")
    real = {n: getattr(lib, n) for n in names}
    calls = dict.fromkeys(names, 0)

    def counting(name):
        def f(*a):
            calls[name] += 1
            return real[name](*a)
        return f

    for n in names:
        monkeypatch.setattr(lib, n, counting(n))
    again = irfd.reenact_video(*args, **kw)
    base = dict(calls)
    for n in names:
        calls[n] = 0
    again_pasted = irfd.reenact_video(*args, paste=True, feather=4, **kw)
    monkeypatch.undo()
    assert torch.equal(again, plain) and torch.equal(again_pasted, pasted)
    # Ei once, then Ee + Ep + Gd per chunk of T = 3 at chunk 2
    assert base == {"spk_launch_list": 1 + 2 * 3, "spk_frames_paste_u8": 0, "spk_frames_f32_to_u8": 0, "spk_frames_u8_to_f32_boxes": 2,
                    "spk_conv2d_fwd": 0}, base
    assert calls == {"spk_launch_list": 1 + 2 * 3, "spk_frames_paste_u8": 2, "spk_frames_f32_to_u8": 0, "spk_frames_u8_to_f32_boxes": 2,
                     "spk_conv2d_fwd": 0}, calls
    plans = [p for p in irfd.Gd.__dict__["_plans"].values() if p.output == "f32"]
    assert plans and all(L.OP_FRAMES_TO_U8 not in [k for k, _ in p.ops] and p.to_u8 is None for p in plans)
    assert plain.shape == (c["T"], 256, 256, 3)
