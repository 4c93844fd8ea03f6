"""GPU checks of the aligned video edge (csrc/frame_sim.hip): ``ops.frames_from_u8_aligned`` and ``ops.frames_paste_u8_aligned``
against the numpy fp64 model tests/sim_ref.py (written from the definitions in include/spk.h, every frame pixel in every sum),
against the table-driven launchers where an axis-aligned crop makes the two forms one, and ``IRFD.reenact_video(align=...)``
against its hand composition.

Bounds.  Way in, on (-1, 1) outputs: 5e-7 absolute -- the fp64 sums contribute <= 1e-12, the one rounding to fp32 of a value
below 2 is <= 1.2e-7, a last-bit tie against the model's own rounding another 2.4e-7.  Way out: ``|dst - z| <= 0.5 + 1e-4`` on
every byte against the model's value ``z`` in front of the final rounding (the fp32 quantise chain contributes <= ~5e-5 byte
units), and every byte outside the model's region is the background, bit for bit.  No pixel is left out: each case asserts, on
the CPU, that every pixel centre lies >= 1e-6 from the edges of its region in (u, v), so no rounding can move one across."""
import importlib

import numpy as np
import pytest
import torch

import sim_ref as R
from oracle import irfd_ref as IR
from oracle.weights_recipe import fill_state_dict, recipe_noises

pytestmark = pytest.mark.gpu
H, W = 40, 56                                   # the frames
NETS = [(16, 16), (12, 20)]                     # the network image, and the generated one
ANGLE_SCALE = [(0.3, 1.3), (-1.1, 0.6), (0.77, 2.3), (0.0, 1.0)]
CENTRES = [(20.3, 27.6), (18.9, 30.2), (21.4, 25.1), (19.7, 28.4)]
TOL_IN, TOL_OUT, MARGIN = 5e-7, 0.5 + 1e-4, 1e-6


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


def source(seed, N, Hs, Ws):
    """Generated frames: most values inside (-1, 1), some beyond both ends."""
    return torch.randn(N, 3, Hs, Ws, generator=torch.Generator().manual_seed(seed)) * 0.7


def rows_for(which, net):
    """fp32 rows for the (angle, scale) cases ``which``: the ``net`` image onto a rectangle ``scale * net width`` wide."""
    return torch.tensor([R.rows(CENTRES[i], ANGLE_SCALE[i][1] * net[1], ANGLE_SCALE[i][0], net) for i in which], dtype=torch.float64).float()


def affine(mean, std):
    """(scale, shift) as the launcher passes them: fp64 on the host, rounded to fp32 at the C boundary"""
    mean, std = ([v] * 3 if isinstance(v, float) else list(v) for v in (mean, std))
    return [float(np.float32(1.0 / (255.0 * s))) for s in std], [float(np.float32(-m / s)) for m, s in zip(mean, std)]


def check_in(got, u8, rows, net, mean=0.5, std=0.5, bgr=False, what=""):
    """got against the model; outputs the model holds at V = 0 by rule must be shift_c exactly.  -> the model's hit mask"""
    scale, shift = affine(mean, std)
    want, hit = R.warp_in(u8.numpy(), rows.numpy(), *net, scale=scale, shift=shift, swap_rb=bgr)
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"way in {what}: largest |got - model| = {err:.3e} (bound {TOL_IN:.1e}); outputs at shift by rule: {int((~hit).sum())}")
    assert err <= TOL_IN
    for c in range(3):
        assert (got[:, c][~hit] == np.float32(shift[c])).all()
    return hit


# ---- the way in -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("which", [(0, 1, 2), (3, 2, 0)])
def test_way_in_a_different_row_per_frame(pkg, dev, net, which):
    """Scale and angle change from frame to frame inside one call: the case the table-driven launcher refuses."""
    u8 = frames(sum(which) + net[0], 3, H, W, 3)
    rows = rows_for(which, net)
    got = pkg.ops.frames_from_u8_aligned(u8.to(dev), net, rows)
    hit = check_in(got, u8, rows, net, what=f"{net}, rows {which}")
    assert hit.mean() > 0.5
    # host rows and device rows of the same values: the same bits
    assert torch.equal(pkg.ops.frames_from_u8_aligned(u8.to(dev), net, rows.to(dev)), got)
    assert torch.equal(pkg.ops.frames_from_u8_aligned(u8.to(dev), net, rows.tolist()), got)
    with pytest.raises(ValueError, match="one filter table"):               # what the table form says to boxes of these sizes
        pkg.ops.frames_from_u8(u8.to(dev), net, crop=[(0, 0, 20, 20), (0, 0, 10, 10), (0, 0, 36, 36)])


@pytest.mark.parametrize("net", NETS)
def test_way_in_footprints_that_leave_the_frame(pkg, dev, net):
    """angle 2.0, scale 1.0, centred at (35.1, 50.3): some footprints are cut by the frame's edge, some miss the frame."""
    u8 = frames(7, 2, H, W, 3)
    rows = torch.tensor([R.rows((35.1, 50.3), 1.0 * net[1], 2.0, net), R.rows((3.2, 4.9), 1.0 * net[1], 2.0, net)], dtype=torch.float64).float()
    mean, std = (0.4, 0.5, 0.6), (0.2, 0.25, 0.5)
    got = pkg.ops.frames_from_u8_aligned(u8.to(dev), net, rows, mean=mean, std=std)
    hit = check_in(got, u8, rows, net, mean, std, what=f"{net}, leaving the frame")
    assert hit.any() and not hit.all()


def test_way_in_invalid_device_rows_give_shift(pkg, dev):
    net = (16, 16)
    u8 = frames(8, 3, H, W, 3)
    rows = rows_for((0, 1, 2), net)
    rows[1, 2] = float("nan")
    rows[2, :2] = torch.tensor([100.0, 0.0])                                # s = 100
    mean, std = (0.4, 0.5, 0.6), (0.2, 0.25, 0.5)
    got = pkg.ops.frames_from_u8_aligned(u8.to(dev), net, rows.to(dev), mean=mean, std=std)
    hit = check_in(got, u8, rows, net, mean, std, what="a NaN row and a row with s = 100")
    assert hit[0].any() and not hit[1:].any()
    shift = torch.tensor(affine(mean, std)[1], dtype=torch.float32).view(1, 3, 1, 1)
    assert torch.equal(got[1:].cpu(), shift.expand(2, 3, *net))
    for bad in (rows, rows.tolist()):                                       # the same rows from the host are refused
        with pytest.raises(ValueError, match="sim"):
            pkg.ops.frames_from_u8_aligned(u8.to(dev), net, bad)
    wild = rows_for((0, 1, 2), net)
    wild[0, 2], wild[1, 3], wild[2, 2] = 3.0e38, -3.0e38, 1.0e12             # finite, far beyond any index
    assert torch.equal(pkg.ops.frames_from_u8_aligned(u8.to(dev), net, wild.to(dev)).cpu(), torch.full((3, 3, *net), -1.0))


def test_way_in_bgr_and_a_strided_slice_at_an_odd_address(pkg, dev):
    net = (12, 20)
    rows = rows_for((2, 0, 1), net)
    big = frames(9, 3, H + 9, W + 13, 3)
    part = big.to(dev)[:, 4:4 + H, 5:5 + W]
    assert not part.is_contiguous() and part.data_ptr() % 2 == 1
    got = pkg.ops.frames_from_u8_aligned(part, net, rows, channel_order="bgr")
    check_in(got, big[:, 4:4 + H, 5:5 + W], rows, net, bgr=True, what="bgr, strided, odd address")
    assert torch.equal(got, pkg.ops.frames_from_u8_aligned(part.contiguous(), net, rows, channel_order="bgr"))
    assert torch.equal(got.flip(1), pkg.ops.frames_from_u8_aligned(part, net, rows))
    one = pkg.ops.frames_from_u8_aligned(part[1], net, rows[1:2])          # [H,W,3]: one frame
    assert torch.equal(one, pkg.ops.frames_from_u8_aligned(part, net, rows)[1:2])


def test_way_in_whole_frame_is_the_table_form(pkg, dev):
    """c = 0, s = 2, the whole frame: ``ops.frames_from_u8``.  <= 2e-6: the table's fp32 weights carry 2^-24 relative error each,
    over two axes, on bytes <= 255, scaled by 2 / 255."""
    u8 = frames(10, 2, H, W, 3).to(dev)
    got = pkg.ops.frames_from_u8_aligned(u8, (H // 2, W // 2), [[2, 0, 0, 0]] * 2)
    want = pkg.ops.frames_from_u8(u8, (H // 2, W // 2))
    err = float((got.double() - want.double()).abs().max())
    print(f"way in, whole frame at s = 2 against frames_from_u8: {err:.3e}")
    assert err <= 2e-6


# ---- the way out ------------------------------------------------------------------------------------------------------------------
def check_out(got, x, bg, rows, feather=0.0, bgr=False, what=""):
    """got against the model on EVERY byte; -> (z, region)"""
    z, region, margin = R.paste_out(x.numpy(), bg.numpy(), rows.numpy(), feather=feather, swap_rb=bgr)
    assert margin >= MARGIN, f"{what}: a pixel centre lies {margin:.2e} from a region edge"
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == z.shape
    over = float(np.abs(got.astype(np.float64) - z).max())
    print(f"way out {what}: largest |got - z| = {over:.6f} (bound {TOL_OUT}); region pixels {int(region.sum())}, margin {margin:.2e}")
    assert over <= TOL_OUT
    assert np.array_equal(got[~region], bg.numpy()[~region])                # every byte outside the region is the background
    return z, region


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("feather", [0, 2.5])
@pytest.mark.parametrize("which", [(0, 1, 2), (3, 2, 0)])
def test_way_out_a_different_row_per_frame(pkg, dev, net, feather, which):
    x, bg = source(sum(which) + net[1], 3, *net), frames(11 + net[0], 3, H, W, 3)
    rows = rows_for(which, net)
    got = pkg.ops.frames_paste_u8_aligned(x.to(dev), bg.to(dev), rows, feather=feather)
    z, region = check_out(got, x, bg, rows, feather, what=f"{net}, rows {which}, feather {feather}")
    assert all(region[n].sum() > 50 for n in range(3))
    assert int((got.cpu().numpy() != bg.numpy()).sum()) > 0.5 * 3 * int(region.sum())   # and the region was written
    # host rows and device rows of the same values: identical bytes
    assert torch.equal(pkg.ops.frames_paste_u8_aligned(x.to(dev), bg.to(dev), rows.to(dev), feather=feather), got)
    assert torch.equal(pkg.ops.frames_paste_u8_aligned(x.to(dev), bg.to(dev), rows.tolist(), feather=feather), got)


def test_way_out_regions_that_leave_the_frame_bgr_and_invalid_rows(pkg, dev):
    """Regions cut by two edges of the frame and one wholly outside it, inside a larger buffer of sentinel bytes; a NaN row from
    the device leaves its frame unchanged."""
    net = (16, 16)
    rows = torch.tensor([R.rows((35.1, 50.3), 1.3 * 16, 2.0, net), R.rows((2.2, 3.9), 2.3 * 16, -0.4, net), R.rows((20.2, 90.4), 16.0, 0.3, net),
                         R.rows((20.3, 27.6), 20.0, 0.3, net), R.rows((20.3, 27.6), 20.0, 0.3, net)], dtype=torch.float64).float()
    rows[3, 0] = float("nan")
    rows[4, :2] = torch.tensor([0.0, 100.0])
    N = 5
    guard = 4 * 3 * W + 1
    raw = torch.full((guard + N * H * W * 3 + guard,), 0xA5, dtype=torch.uint8, device=dev)
    view = raw[guard:guard + N * H * W * 3].view(N, H, W, 3)
    assert view.data_ptr() % 2 == 1
    x, bg = source(13, N, *net), frames(14, N, H, W, 3)
    view.copy_(bg.to(dev))
    out = pkg.ops.frames_paste_u8_aligned(x.to(dev), view, rows.to(dev), feather=2.5, channel_order="bgr", out=view)
    assert out is view
    z, region = check_out(view, x, bg, rows, 2.5, bgr=True, what="leaving the frame, bgr")
    assert 0 < region[0].sum() < 16 * 16 * 1.69 * 0.9 and 0 < region[1].sum() and not region[2:].any()
    got = view.cpu()
    assert torch.equal(got[2:], bg[2:]) and not torch.equal(got[0], bg[0]) and not torch.equal(got[1], bg[1])
    assert torch.all(raw[:guard] == 0xA5) and torch.all(raw[guard + N * H * W * 3:] == 0xA5)
    for bad in (rows, rows.tolist()):
        with pytest.raises(ValueError, match="sim"):
            pkg.ops.frames_paste_u8_aligned(x.to(dev), bg.to(dev), bad)


def test_way_out_in_place_out_and_a_strided_background(pkg, dev):
    net = (12, 20)
    rows = rows_for((0, 1, 3), net)
    x, bg = source(15, 3, *net).to(dev), frames(16, 3, H, W, 3).to(dev)
    keep = bg.clone()
    f = pkg.ops.frames_paste_u8_aligned
    cloned = f(x, bg, rows, feather=2.5)
    assert torch.equal(bg, keep) and cloned.data_ptr() != bg.data_ptr()              # without out the input is unchanged
    other = torch.empty_like(bg)
    assert f(x, bg, rows, feather=2.5, out=other) is other and torch.equal(other, cloned) and torch.equal(bg, keep)
    assert f(x, bg, rows, feather=2.5, out=bg) is bg and torch.equal(bg, cloned)
    # a strided background at an odd byte address, written through its strides; the rest of the buffer stays
    big = frames(17, 3, H + 9, W + 13, 3).to(dev)
    big[:, 4:4 + H, 5:5 + W] = keep
    before = big.clone()
    part = big[:, 4:4 + H, 5:5 + W]
    assert not part.is_contiguous() and part.data_ptr() % 2 == 1
    assert f(x, part, rows, feather=2.5, out=part) is part and torch.equal(part, cloned)
    rest = torch.ones(3, H + 9, W + 13, dtype=torch.bool)
    rest[:, 4:4 + H, 5:5 + W] = False
    assert torch.equal(big.cpu()[rest], before.cpu()[rest])
    got = f(x, before[:, 4:4 + H, 5:5 + W], rows, feather=2.5)                        # strided in, no out: a packed clone
    assert got.is_contiguous() and torch.equal(got, cloned)


@pytest.mark.parametrize("feather", [0, 2.5])
def test_way_out_integer_box_is_the_table_form(pkg, dev, feather):
    """c = 0, s = 1.5, an integer origin: ``ops.frames_paste_u8``.  Bytes differ by <= 1, and only where the model's value is
    within 1e-4 of a rounding tie (the table form sums with fp32 weights)."""
    S, h, origin = 16, 24, (5, 7)
    x, bg = source(18, 3, S, S), frames(19, 3, H, W, 3)
    rows = torch.tensor([[h / S, 0, origin[1], origin[0]]] * 3)
    got = pkg.ops.frames_paste_u8_aligned(x.to(dev), bg.to(dev), rows, feather=feather)
    z, region = check_out(got, x, bg, rows, feather, what=f"integer box, feather {feather}")
    box = np.zeros((3, H, W), dtype=bool)
    box[:, origin[0]:origin[0] + h, origin[1]:origin[1] + h] = True
    assert np.array_equal(region, box)
    want = pkg.ops.frames_paste_u8(x.to(dev), bg.to(dev), (*origin, h, h), feather=feather)
    diff = (got.int() - want.int()).abs().cpu().numpy()
    near_tie = np.abs(z - np.floor(z) - 0.5) <= 1e-4
    print(f"integer box, feather {feather}: {int((diff > 0).sum())} of {diff.size} bytes differ from frames_paste_u8")
    assert diff.max() <= 1 and not (diff > 0)[~near_tie].any()


# ---- the public interface ---------------------------------------------------------------------------------------------------------
SIZE = 128          # encoder input of the model-level cases, as tests/test_paste_gpu.py


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
    """Identity photo, T = 3 BGR video frames of 64 x 80, a transform per frame (scale and angle change), explicit noise."""
    T = 3
    rows = pkg.ops.similarity_rows([(30.3, 41.6), (33.9, 38.2), (28.4, 44.1)], [44.0, 52.0, 36.0], [0.2, -0.3, 0.1], SIZE)
    return dict(T=T, ident_u8=frames(31, 56, 72, 3).to(dev), pose_u8=frames(32, T, 64, 80, 3).to(dev), emo_u8=frames(33, T, 64, 80, 3).to(dev),
                rows=rows, noises=[n.to(dev) for n in recipe_noises("frame_io", T, 256)])


def test_reenact_video_align_is_its_hand_composition(irfd, pkg, clip, dev):
    c, ops = clip, pkg.ops
    keep = c["pose_u8"].clone()
    ident = ops.frames_from_u8(c["ident_u8"], SIZE, channel_order="bgr")
    pose, emo = (ops.frames_from_u8_aligned(c[k], SIZE, c["rows"], channel_order="bgr") for k in ("pose_u8", "emo_u8"))
    kw = dict(size=SIZE, align=c["rows"], channel_order="bgr", noises=c["noises"], chunk=2)
    # paste=False: the generated frames
    want = irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2, output="uint8", channel_order="bgr")
    got = irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], **kw)
    assert got.dtype == torch.uint8 and got.shape == (c["T"], 256, 256, 3) and torch.equal(got, want)
    # paste=True: the full frames; the generated image has 256 pixels where the network image has 128
    f32 = irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2)
    half = c["rows"] * torch.tensor([0.5, 0.5, 1.0, 1.0])
    want = ops.frames_paste_u8_aligned(f32, c["pose_u8"], half, feather=4, channel_order="bgr")
    got = irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], paste=True, feather=4, **kw)
    assert got.dtype == torch.uint8 and got.shape == (c["T"], 64, 80, 3) and torch.equal(got, want)
    assert torch.equal(c["pose_u8"], keep) and got.data_ptr() != c["pose_u8"].data_ptr() and not torch.equal(got, keep)
    # the same rows from the device; in place
    kw["align"] = c["rows"].to(dev)
    assert torch.equal(irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], paste=True, feather=4, **kw), want)
    video = c["pose_u8"].clone()
    assert irfd.reenact_video(c["ident_u8"], video, c["emo_u8"], paste=True, feather=4, inplace=True, **kw) is video and torch.equal(video, want)


def test_reenact_video_align_chunks_and_launches(irfd, pkg, clip, dev, monkeypatch):
    """``chunk=1`` and ``chunk=2`` give identical bytes; exactly one ``spk_frames_paste_u8_sim`` launch per chunk and one
    ``spk_frames_u8_to_f32_sim`` per clip of pose frames, none of the table-driven paste."""
    c = clip
    kw = dict(size=SIZE, align=c["rows"], channel_order="bgr", paste=True, feather=4, seed=7)
    a = irfd.reenact_video(c["ident_u8"], c["pose_u8"], chunk=1, **kw)
    lib = pkg._lib.lib()
    names = ("spk_frames_paste_u8_sim", "spk_frames_u8_to_f32_sim", "spk_frames_paste_u8", "spk_frames_u8_to_f32_boxes")
    real = {n: getattr(lib, n) for n in names}
    calls = dict.fromkeys(names, 0)

    def counting(name):
        def f(*args):
            calls[name] += 1
            return real[name](*args)
        return f

    for n in names:
        monkeypatch.setattr(lib, n, counting(n))
    b = irfd.reenact_video(c["ident_u8"], c["pose_u8"], chunk=2, **kw)
    monkeypatch.undo()
    assert torch.equal(a, b) and not torch.equal(a, c["pose_u8"])
    assert calls == {"spk_frames_paste_u8_sim": 2, "spk_frames_u8_to_f32_sim": 1, "spk_frames_paste_u8": 0, "spk_frames_u8_to_f32_boxes": 0}, calls
