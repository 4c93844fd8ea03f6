"""GPU checks of the video-frame edge (csrc/frame_io.hip): ``ops.frames_from_u8`` against torch's fp64 CPU
``interpolate(antialias=True)``, ``ops.frames_to_u8`` bit for bit against the torch CPU expression it replaces, the uint8 decoder
plan and ``IRFD.reenact(output="uint8")`` / ``IRFD.reenact_video`` against their hand compositions.

Error bound of the input kernel: ``(taps_x + taps_y + 8) * 2^-23`` absolute on an output in [-1, 1] -- the dot-product bound for a
separable sum of values <= 255 scaled by 2/255 with fp32-rounded weights and the final roundings.  The kernel's sums run in fp64,
so its chain is no longer than the bound assumes; measured (MI355X): 0.67 - 1.57 x 2^-23 over the cases below (bounds 10 - 32), the
identity 1.12 ulp from 2u/255 - 1, an all-255 frame exactly 1 ulp above +1 (the fp32 scale's own rounding), an all-0 frame exactly -1.  "ulp" below is 2^-23,
the spacing of fp32 at the ends of the output range: the scale 2/255 is passed as an fp32 number whose own rounding already moves
``scale * u`` by up to |2u/255| * 2^-24, so an error measured in ulps of a result near 0 is not what the formula can meet."""
import importlib

import pytest
import torch
import torch.nn.functional as F

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


def frames(seed, *shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def resize_ref(u8, Hout, Wout, bgr=False, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
    """fp64 on the CPU: ToTensor + antialiased bilinear Resize + Normalize."""
    x = u8.double().permute(0, 3, 1, 2)
    if bgr:
        x = x.flip(1)
    y = F.interpolate(x, size=(Hout, Wout), mode="bilinear", align_corners=False, antialias=True) / 255
    m, s = torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    return (y - m) / s


def taps(pkg, Hin, Win, Hout, Wout):
    return pkg.ops.resize_tables(Hin, Hout)[2].shape[1] + pkg.ops.resize_tables(Win, Wout)[2].shape[1]


# N, Hin, Win, Hout, Wout
RESIZE_CASES = [(3, 37, 53, 16, 16), (3, 135, 240, 32, 32), (3, 20, 28, 32, 32), (3, 32, 32, 32, 32), (3, 40, 40, 24, 40), (1, 37, 53, 16, 16)]


@pytest.mark.parametrize("N,Hin,Win,Hout,Wout", RESIZE_CASES)
def test_frames_from_u8_vs_fp64_interpolate(pkg, dev, N, Hin, Win, Hout, Wout):
    u = frames(Hin * 1000 + Wout + N, N, Hin, Win, 3)
    got = pkg.ops.frames_from_u8(u.to(dev), (Hout, Wout))
    assert got.shape == (N, 3, Hout, Wout) and got.dtype == torch.float32
    err = float((got.cpu().double() - resize_ref(u, Hout, Wout)).abs().max())
    t = taps(pkg, Hin, Win, Hout, Wout)
    print(f"frames_from_u8 {N}x{Hin}x{Win} -> {Hout}x{Wout}: max-abs error {err / ULP:.2f} x 2^-23, bound {t + 8} x 2^-23 ({t} taps)")
    assert err <= (t + 8) * ULP
    if (Hin, Win) == (Hout, Wout):
        # identity: one tap of weight 1 per axis, the result is scale * u + shift
        exact = float((got.cpu().double() - (2 * u.double().permute(0, 3, 1, 2) / 255 - 1)).abs().max())
        print(f"  identity: {exact / ULP:.2f} ulp from 2u/255 - 1")
        assert exact <= 2 * ULP
    # a square size given as one number is the same call
    if Hout == Wout:
        assert torch.equal(pkg.ops.frames_from_u8(u.to(dev), Hout), got)


@pytest.mark.parametrize("N,Hin,Win,Hout,Wout", RESIZE_CASES)
def test_constant_frames_stay_constant(pkg, dev, N, Hin, Win, Hout, Wout):
    """The rows of the tables sum to exactly 1: an all-255 / all-0 frame is +1 / -1 within one ulp at every size."""
    for value, want in ((255, 1.0), (0, -1.0)):
        u = torch.full((N, Hin, Win, 3), value, dtype=torch.uint8)
        got = pkg.ops.frames_from_u8(u.to(dev), (Hout, Wout)).cpu().double()
        off = float((got - want).abs().max())
        print(f"constant {value} {Hin}x{Win} -> {Hout}x{Wout}: {off / ULP:.2f} ulp from {want:+.0f}")
        assert off <= ULP


def test_frames_from_u8_bgr_and_normalisation(pkg, dev):
    N, Hin, Win, Hout, Wout = 3, 37, 53, 16, 16
    u = frames(11, N, Hin, Win, 3)
    rgb = pkg.ops.frames_from_u8(u.to(dev), 16)
    bgr = pkg.ops.frames_from_u8(u.to(dev), 16, channel_order="bgr")
    assert torch.equal(bgr, rgb.flip(1))
    bound = (taps(pkg, Hin, Win, Hout, Wout) + 8) * ULP
    assert float((bgr.cpu().double() - resize_ref(u, 16, 16, bgr=True)).abs().max()) <= bound
    # a non-default mean / std triple (ImageNet's): |scale| grows to 1 / (255 * 0.224), the bound with it
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    got = pkg.ops.frames_from_u8(u.to(dev), 16, mean=mean, std=std)
    err = float((got.cpu().double() - resize_ref(u, 16, 16, mean=mean, std=std)).abs().max())
    # values reach (1 - 0.406) / 0.225 = 2.64: the final rounding is up to 2^-23 (half an ulp in [2, 4)), the sum's share scales by
    # 0.5 / 0.224
    print(f"mean/std triple: max-abs error {err / ULP:.2f} x 2^-23, bound {bound * 0.5 / 0.224 / ULP:.1f} x 2^-23")
    assert err <= bound * 0.5 / 0.224
    one = pkg.ops.frames_from_u8(u.to(dev), 16, mean=0.25, std=0.5)
    assert torch.equal(one, pkg.ops.frames_from_u8(u.to(dev), 16, mean=(0.25, 0.25, 0.25), std=(0.5, 0.5, 0.5)))


def test_frames_from_u8_crop_reads_odd_addresses_in_place(pkg, dev):
    u = frames(12, 3, 64, 80, 3).to(dev)
    y0, x0, h, w = 5, 7, 37, 53
    box = u[:, y0:y0 + h, x0:x0 + w]
    assert box.data_ptr() % 2 == 1 and box.stride(1) > 3 * w and not box.is_contiguous()
    got = pkg.ops.frames_from_u8(u, 16, crop=(y0, x0, h, w))
    assert torch.equal(got, pkg.ops.frames_from_u8(box.contiguous(), 16))
    assert torch.equal(got, pkg.ops.frames_from_u8(box, 16))                  # a strided view is read in place too
    assert float((got.cpu().double() - resize_ref(box.cpu(), 16, 16)).abs().max()) <= (taps(pkg, h, w, 16, 16) + 8) * ULP
    assert torch.equal(pkg.ops.frames_from_u8(u[1], 16, crop=(y0, x0, h, w)), got[1:2])      # one [H,W,3] frame


def test_frames_from_u8_second_grid_stride_trip(pkg, dev):
    """The launch is capped at 2048 workgroups of 256 threads, a thread per (frame, 8-row strip, column): N = 8 frames of
    96 strips x 720 columns are 552960 work items, so the last 28672 (the end of the last frame) run in the second trip."""
    N, Hin, Win, Hout, Wout = 8, 24, 20, 768, 720
    assert N * ((Hout + 7) // 8) * Wout > 2048 * 256
    u = frames(13, N, Hin, Win, 3)
    got = pkg.ops.frames_from_u8(u.to(dev), (Hout, Wout)).cpu()
    ref = resize_ref(u, Hout, Wout)
    err = float((got.double() - ref).abs().max())
    print(f"grid-stride case: max-abs error {err / ULP:.2f} x 2^-23")
    assert err <= (taps(pkg, Hin, Win, Hout, Wout) + 8) * ULP
    assert float((got[-1, :, -8:].double() - ref[-1, :, -8:]).abs().max()) <= (taps(pkg, Hin, Win, Hout, Wout) + 8) * ULP


# ---- output kernel -----------------------------------------------------------------------------------------------------
def quant_ref(x, lo, hi, bgr=False):
    """The torch expression the kernel replaces, on the CPU in fp32."""
    k = 255.0 / (hi - lo)
    q = ((x - lo) * k).clamp(0, 255).round().to(torch.uint8)
    if bgr:
        q = q.flip(1)
    return q.permute(0, 2, 3, 1).contiguous()


def tie_grid():
    """Every rounding tie of the (-1, 1) range -- the fp32 nearest (k + 0.5) / 127.5 - 1 and its two neighbours, k = 0..254 --
    and the range ends, values beyond them, infinities and -0."""
    k = torch.arange(255, dtype=torch.float64)
    mid = ((k + 0.5) / 127.5 - 1).float()
    vals = [mid, torch.nextafter(mid, torch.full_like(mid, 2.0)), torch.nextafter(mid, torch.full_like(mid, -2.0)),
            torch.tensor([1.0, -1.0, 1.0000001, -1.0000001, 3.0, -3.0, float("inf"), float("-inf"), -0.0])]
    return torch.cat(vals)


@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (1, 3, 5, 6)])
@pytest.mark.parametrize("bgr,rng", [(False, (-1, 1)), (True, (-1, 1)), (False, (0, 1))])
def test_frames_to_u8_is_the_torch_expression_bit_for_bit(pkg, dev, shape, bgr, rng):
    g = torch.Generator().manual_seed(shape[2] * 10 + shape[3])
    x = torch.randn(shape, generator=g) * 0.7
    if rng == (0, 1):
        x = x * 0.5 + 0.5
    got = pkg.ops.frames_to_u8(x.to(dev), value_range=rng, channel_order="bgr" if bgr else "rgb")
    assert got.dtype == torch.uint8 and got.shape == (shape[0], shape[2], shape[3], 3)
    assert torch.equal(got.cpu(), quant_ref(x, *rng, bgr=bgr))


@pytest.mark.parametrize("W", [16, 6])
def test_frames_to_u8_rounding_ties_and_range_ends(pkg, dev, W):
    v = tie_grid()
    n = 3 * 4 * W
    v = torch.cat([v, torch.zeros(-v.numel() % n)])
    x = v.view(-1, 3, 4, W)                      # W = 16: the float4 / dword form; W = 6: H*W = 24, float4 too; see below for the tail
    got = pkg.ops.frames_to_u8(x.to(dev))
    assert torch.equal(got.cpu(), quant_ref(x, -1, 1))
    x2 = v[: (v.numel() // 45) * 45].view(-1, 3, 3, 5)         # H*W = 15: the dword-load / byte-store form with its tail
    assert torch.equal(pkg.ops.frames_to_u8(x2.to(dev)).cpu(), quant_ref(x2, -1, 1))
    x01 = (x * 0.5 + 0.5)
    assert torch.equal(pkg.ops.frames_to_u8(x01.to(dev), value_range=(0, 1)).cpu(), quant_ref(x01, 0, 1))


def test_frames_to_u8_into_a_buffer_one_byte_off_alignment(pkg, dev):
    x = torch.randn(3, 3, 4, 8, generator=torch.Generator().manual_seed(5)) * 0.7
    raw = torch.full((3 * 4 * 8 * 3 + 8,), 77, device=dev, dtype=torch.uint8)
    out = raw[1:1 + 3 * 4 * 8 * 3].view(3, 4, 8, 3)
    assert out.data_ptr() % 4 == 1
    pkg.ops.frames_to_u8(x.to(dev), channel_order="bgr", out=out)
    assert torch.equal(out.cpu(), quant_ref(x, -1, 1, bgr=True))
    assert int(raw[0]) == 77 and torch.all(raw[1 + 3 * 4 * 8 * 3:] == 77)      # nothing written around it


def test_round_trip_is_exact(pkg, dev):
    u = frames(21, 1, 32, 32, 3).to(dev)
    assert torch.equal(pkg.ops.frames_to_u8(pkg.ops.frames_from_u8(u, 32)), u)
    bgr = pkg.ops.frames_to_u8(pkg.ops.frames_from_u8(u, 32, channel_order="bgr"), channel_order="bgr")
    assert torch.equal(bgr, u)


# ---- plans and the public interface ---------------------------------------------------------------------------------------
SIZE = 128          # encoder input of the model-level cases (a frame size of test_reenact_gpu.py); the decoder always makes 256^2


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
def clip(pkg, dev):
    """Identity photo, T = 3 BGR video frames of 48 x 64 with a crop box, and explicit noise."""
    T = 3
    ident_u8, pose_u8, emo_u8 = frames(31, 56, 72, 3).to(dev), frames(32, T, 48, 64, 3).to(dev), frames(33, T, 48, 64, 3).to(dev)
    crop = (3, 5, 40, 44)
    noises = [n.to(dev) for n in recipe_noises("frame_io", T, 256)]
    f = pkg.ops.frames_from_u8
    ident, pose, emo = f(ident_u8, SIZE, channel_order="bgr"), f(pose_u8, SIZE, crop=crop, channel_order="bgr"), \
        f(emo_u8, SIZE, crop=crop, channel_order="bgr")
    return dict(T=T, ident_u8=ident_u8, pose_u8=pose_u8, emo_u8=emo_u8, crop=crop, noises=noises, ident=ident, pose=pose, emo=emo)


def test_reenact_uint8_is_frames_to_u8_of_reenact(irfd, pkg, clip, dev):
    c = clip
    f32 = irfd.reenact(c["ident"], c["pose"], c["emo"], noises=c["noises"], chunk=2)         # T = 3: one ragged chunk
    again = irfd.reenact(c["ident"], c["pose"], c["emo"], noises=c["noises"], chunk=2, output="f32")
    assert f32.dtype == torch.float32 and torch.equal(f32, again)                        # the default path, twice in one process
    u8 = irfd.reenact(c["ident"], c["pose"], c["emo"], noises=c["noises"], chunk=2, output="uint8")
    assert u8.dtype == torch.uint8 and u8.shape == (c["T"], 256, 256, 3)
    assert torch.equal(u8, pkg.ops.frames_to_u8(f32))
    print(f"uint8 frames: mean {float(u8.float().mean()):.1f}, std {float(u8.float().std()):.1f}, {u8.unique().numel()} distinct values")
    bgr = irfd.reenact(c["ident"], c["pose"], c["emo"], noises=c["noises"], chunk=2, output="uint8", channel_order="bgr")
    assert torch.equal(bgr, pkg.ops.frames_to_u8(f32, channel_order="bgr")) and torch.equal(bgr, u8.flip(3))
    assert torch.equal(irfd.reenact(c["ident"], c["pose"], c["emo"], noises=c["noises"], chunk=2), f32)     # and the fp32 plans are as they were


def test_uint8_decoder_plan_is_the_fp32_plan_plus_one_op(irfd, pkg, dev, monkeypatch):
    L, PL = pkg._lib, importlib.import_module("speak-hack_amd.plan")
    Gd = irfd.Gd
    Gd.__dict__.pop("_plans", None)
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(2, 6144, generator=g).to(dev)
    noises = [n.to(dev) for n in recipe_noises("frame_io.plan", 2, 256)]
    y32 = Gd.plan_forward(feats, noises)
    y8 = Gd.plan_forward(feats, noises, output="uint8")
    plans = list(Gd.__dict__["_plans"].values())
    assert len(plans) == 2                                                  # side by side
    p32, p8 = plans
    assert p32.output == "f32" and p8.output == "uint8" and p32.to_u8 is None
    k32, k8 = [k for k, _ in p32.ops], [k for k, _ in p8.ops]
    assert L.OP_FRAMES_TO_U8 not in k32 and k8 == k32 + [L.OP_FRAMES_TO_U8]
    for (ka, da), (kb, db) in zip(p32.ops, p8.ops):                         # the same launches: kinds, and for the convs flags and shapes
        if ka == L.OP_CONV2D:
            assert (da.flags, da.B, da.Cin, da.Cout, da.H, da.W, da.config, da.ksplit) == (db.flags, db.B, db.Cin, db.Cout, db.H, db.W, db.config, db.ksplit)
    assert torch.equal(y8, pkg.ops.frames_to_u8(y32))
    lib = L.lib()
    calls = {"list": 0, "quant": 0, "conv": 0}
    real = {n: getattr(lib, n) for n in ("spk_launch_list", "spk_frames_f32_to_u8", "spk_conv2d_fwd")}

    def counting(name, slot):
        def f(*a):
            calls[slot] += 1
            return real[name](*a)
        return f

    monkeypatch.setattr(lib, "spk_launch_list", counting("spk_launch_list", "list"))
    monkeypatch.setattr(lib, "spk_frames_f32_to_u8", counting("spk_frames_f32_to_u8", "quant"))
    monkeypatch.setattr(lib, "spk_conv2d_fwd", counting("spk_conv2d_fwd", "conv"))
    again = Gd.plan_forward(feats, noises, output="uint8")
    monkeypatch.undo()
    assert calls == {"list": 1, "quant": 0, "conv": 0}, calls
    assert torch.equal(again, y8)
    assert torch.equal(Gd.plan_forward(feats, noises), y32)                 # the fp32 plan: unchanged, still cached
    assert len(Gd.__dict__["_plans"]) == 2 and p32 in Gd.__dict__["_plans"].values() and p8 in Gd.__dict__["_plans"].values()
    # range and channel order are part of the key
    y01 = Gd.plan_forward(feats, noises, output="uint8", value_range=(0, 1), swap_rb=True)
    assert len(Gd.__dict__["_plans"]) == 3 and torch.equal(y01, pkg.ops.frames_to_u8(y32, value_range=(0, 1), channel_order="bgr"))


def test_reenact_video_is_frames_from_u8_then_reenact(irfd, pkg, clip, dev):
    c = clip
    want = irfd.reenact(c["ident"], c["pose"], c["emo"], noises=c["noises"], chunk=2, output="uint8", channel_order="bgr")
    got = irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], size=SIZE, crop=c["crop"], channel_order="bgr",
                             noises=c["noises"], chunk=2)
    assert got.dtype == torch.uint8 and got.shape == (c["T"], 256, 256, 3) and torch.equal(got, want)
    a = irfd.reenact_video(c["ident_u8"], c["pose_u8"], None, size=SIZE, crop=c["crop"], channel_order="bgr", noises=c["noises"], chunk=2)
    b = irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["pose_u8"], size=SIZE, crop=c["crop"], channel_order="bgr", noises=c["noises"], chunk=2)
    assert torch.equal(a, b)
