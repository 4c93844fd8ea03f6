"""GPU checks of the seamless paste-back (csrc/frame_blend.hip): ``ops.frames_paste_u8_aligned(matte=, colour=)`` and
``ops.paste_colour_match`` against the numpy fp64 model tests/blend_ref.py (written from the definitions in include/spk.h),
against the plain aligned paste where the two must be one, and ``IRFD.reenact_video(matte=, colour_match=True)`` against its hand
composition.  The cases are those of tests/blend_cases.py; tests/test_blend_cpu.py asserts their margins and variances.

Bounds.  Paste with a matte: ``|dst - z| <= 0.5 + 1e-4`` on every byte, the bound of tests/test_align_gpu.py (the fp32 quantise
chain contributes <= ~5e-5 byte units; the matte adds only fp64 work).  Colour rows: ``|g - g_ref| <= 2^-22 g_ref`` and
``|o - o_ref| <= 2^-15``: with at most 40 * 56 non-negative terms the fp64 sums agree with the model's to about 1e-12 relative, the
cancellation in a variance of at least 100 levels^2 amplifies that by at most 255^2 / 100, so only the one rounding to fp32 can
differ, by one ulp; the bounds are two ulps of g, and two ulps of a value below 256 for o.  Paste with colour rows, the model fed
the rows the device produced: ``0.5 + 2e-4`` for gains <= 2 -- the quantise chain's 5e-5 times the gain, plus one ``fmaf`` rounding
of a value of at most 255 (1.5e-5)."""
import importlib

import numpy as np
import pytest
import torch

import blend_cases as BC
import blend_ref as B
from oracle import irfd_ref as IR
from oracle.weights_recipe import fill_state_dict, recipe_noises

pytestmark = pytest.mark.gpu
H, W = BC.H, BC.W
TOL_MATTE, TOL_COLOUR, TOL_G, TOL_O = 0.5 + 1e-4, 0.5 + 2e-4, 2.0 ** -22, 2.0 ** -15


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


def on(c, dev):
    """A case's tensors where the kernels want them: -> (x, bg, rows, matte, keywords of both launchers)"""
    kw = dict(feather=c["feather"], channel_order="bgr" if c["bgr"] else "rgb")
    return c["x"].to(dev), c["bg"].to(dev), c["rows"].to(dev), None if c["matte"] is None else c["matte"].to(dev), kw


# ---- 1. no matte, no colour: the plain aligned paste, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("feather", [0, 2.5])
def test_blend_entry_without_matte_and_colour_is_the_plain_paste(pkg, dev, feather):
    """The new entry point called directly (the launcher would route this call to the old one): rotation, s < 1, s > 2, a region
    leaving the frame, an invalid row; rgb and bgr."""
    import sim_ref as R
    lib, L = pkg._lib.lib(), pkg._lib
    for net in BC.NETS:
        rows = torch.cat([BC.rows_for((0, 1, 2), net), torch.tensor([R.rows((35.1, 50.3), 1.3 * net[1], 2.0, net), [float("nan"), 0, 0, 0]],
                                                                    dtype=torch.float64).float()]).to(dev)
        N = rows.size(0)
        x, bg = BC.source(40 + net[0], N, *net).to(dev), BC.frames(41 + net[0], N, H, W, 3).to(dev)
        for order in ("rgb", "bgr"):
            want = pkg.ops.frames_paste_u8_aligned(x, bg, rows, feather=feather, channel_order=order)
            got = bg.clone()
            L.check(lib.spk_frames_paste_u8_sim_blend(x.data_ptr(), N, *net, got.data_ptr(), got.stride(0), got.stride(1), H, W, rows.data_ptr(),
                                                      int(order == "bgr"), float(feather), -1.0, 127.5, None, 0, None, L.stream_ptr()), "blend")
            assert torch.equal(got, want) and not torch.equal(got[:4], bg[:4]) and torch.equal(got[4], bg[4])
            # identity rows through the launcher take the new kernel's colour step and change nothing either
            ident = torch.tensor([1.0, 0.0], device=dev).repeat(N, 3, 1)
            assert torch.equal(pkg.ops.frames_paste_u8_aligned(x, bg, rows, feather=feather, channel_order=order, colour=ident), want)


# ---- 2. matte, shared and per frame ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.MATTE_CASES)
def test_paste_with_a_matte_against_the_model(pkg, dev, name):
    c, ref = BC.case(name), BC.reference(name)
    x, bg, rows, matte, kw = on(c, dev)
    got_dev = pkg.ops.frames_paste_u8_aligned(x, bg, rows, matte=matte, **kw)
    got = got_dev.cpu().numpy()
    z, region, bg_np = ref["z"], ref["region"], c["bg"].numpy()
    over = float(np.abs(got.astype(np.float64) - z).max())
    zero = (ref["Mt"] == 0) & region
    print(f"matte, {name}: largest |got - z| = {over:.6f} (bound {TOL_MATTE}); region pixels {int(region.sum())}, of them Mt = 0: {int(zero.sum())}")
    assert ref["margin"] >= BC.MARGIN and over <= TOL_MATTE
    assert np.array_equal(got[~region], bg_np[~region])                     # every byte outside the region is the background
    assert zero.any() and np.array_equal(got[zero], bg_np[zero])            # and so is every byte where the matte is exactly 0
    assert int((got != bg_np).sum()) > 0.2 * 3 * int(region.sum())          # the region was written
    # host rows and device rows of the same values: identical bytes; a shared matte is that matte for every frame
    assert torch.equal(pkg.ops.frames_paste_u8_aligned(x, bg, c["rows"], matte=matte, **kw), got_dev)
    if matte.dim() == 2:
        assert torch.equal(pkg.ops.frames_paste_u8_aligned(x, bg, rows, matte=matte.expand(x.size(0), -1, -1).contiguous(), **kw), got_dev)
    # in place through out=
    video = bg.clone()
    assert pkg.ops.frames_paste_u8_aligned(x, video, rows, matte=matte, out=video, **kw) is video and torch.equal(video, got_dev)


# ---- 3. colour rows against the model -------------------------------------------------------------------------------------------------
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
    if c["kind"] == "tenth":                                                # the gain meets max_gain exactly
        assert (got[:, :, 0] == BC.MAX_GAIN).all()
    if c["kind"] == "constant":                                             # var_q = 0: g == 1 exactly, o = mu_b - mu_q
        assert (got[:, :, 0] == 1.0).all()


@pytest.mark.parametrize("name", BC.COLOUR_CASES)
def test_colour_rows_against_the_model(pkg, dev, name):
    c, ref = BC.case(name), BC.reference(name)
    x, bg, rows, matte, kw = on(c, dev)
    if name == "strided":                                                   # a strided background at an odd address, read in place
        big = BC.frames(77, x.size(0), H + 9, W + 13, 3).to(dev)
        big[:, 4:4 + H, 5:5 + W] = bg
        bg = big[:, 4:4 + H, 5:5 + W]
        assert not bg.is_contiguous() and bg.data_ptr() % 2 == 1
    keep = bg.clone()
    got = pkg.ops.paste_colour_match(x, bg, rows, matte=matte, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (x.size(0), 3, 2) and got.is_cuda
    check_rows(got, ref, c, name)
    assert torch.equal(bg, keep)                                            # it reads the background and writes no frame
    # two calls on the same inputs: the same bits; out= is written and returned
    out = torch.full_like(got, 7.0)
    assert pkg.ops.paste_colour_match(x, bg, rows, matte=matte, out=out, **kw) is out and torch.equal(out, got)
    if not c["by_rule"]:                                                    # host rows (all valid) and device rows: the same bits
        assert torch.equal(pkg.ops.paste_colour_match(x, bg, c["rows"], matte=matte, **kw), got)
    # a frame's row depends on that frame alone
    assert torch.equal(pkg.ops.paste_colour_match(x[1:2], bg[1:2], rows[1:2], matte=matte if matte is None or matte.dim() == 2 else matte[1:2], **kw),
                       got[1:2])


def test_colour_rows_follow_their_parameters(pkg, dev):
    """max_gain, min_sigma and min_weight as the definition uses them, on the generic case."""
    c, ref = BC.case("generic"), BC.reference("generic")
    x, bg, rows, matte, kw = on(c, dev)
    for params in (dict(max_gain=1.0), dict(max_gain=1.05, min_sigma=0.0), dict(min_sigma=200.0), dict(min_weight=1e6), dict(min_weight=0.0)):
        p = dict(max_gain=BC.MAX_GAIN, min_sigma=BC.MIN_SIGMA, min_weight=BC.MIN_WEIGHT)
        p.update(params)
        want, _, _ = B.colour_rows(ref["sums"], ref["valid"], **p)
        got = pkg.ops.paste_colour_match(x, bg, rows, **kw, **params).cpu().numpy().astype(np.float64)
        assert (np.abs(got[:, :, 0] - want[:, :, 0]) <= TOL_G * want[:, :, 0]).all() and (np.abs(got[:, :, 1] - want[:, :, 1]) <= TOL_O).all(), params
        if "max_gain" in params and params["max_gain"] == 1.0 or params.get("min_sigma") == 200.0:
            assert (got[:, :, 0] == 1.0).all()
        if params.get("min_weight") == 1e6:
            assert got.tolist() == [[[1.0, 0.0]] * 3] * x.size(0)


# ---- 4. paste with colour rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.PASTE_COLOUR_CASES)
def test_paste_with_colour_rows_against_the_model(pkg, dev, name):
    """The model is fed the rows the device produced, read back, so this test does not inherit the ulp of the rows."""
    c = BC.case(name)
    x, bg, rows, matte, kw = on(c, dev)
    colour = pkg.ops.paste_colour_match(x, bg, rows, matte=matte, **kw)
    assert float(colour[:, :, 0].max()) <= 2.0
    got = pkg.ops.frames_paste_u8_aligned(x, bg, rows, matte=matte, colour=colour, **kw).cpu().numpy()
    ref = B.blend(c["x"].numpy(), c["bg"].numpy(), c["rows"].numpy(), feather=c["feather"], swap_rb=c["bgr"],
                  matte=None if c["matte"] is None else c["matte"].numpy(), colour=colour.cpu().numpy())
    over = float(np.abs(got.astype(np.float64) - ref["z"]).max())
    plain = BC.reference(name)["z"]
    print(f"paste with colour, {name}: largest |got - z| = {over:.6f} (bound {TOL_COLOUR}); the rows move z by up to {np.abs(ref['z'] - plain).max():.1f}")
    assert ref["margin"] >= BC.MARGIN and over <= TOL_COLOUR
    assert np.array_equal(got[~ref["region"]], c["bg"].numpy()[~ref["region"]])
    assert np.abs(ref["z"] - plain).max() > 2.0                             # the rows did something


def test_a_nan_gain_is_the_identity_for_that_channel_only(pkg, dev):
    c = BC.case("bgr")
    x, bg, rows, matte, kw = on(c, dev)
    colour = pkg.ops.paste_colour_match(x, bg, rows, **kw)
    holed = colour.clone()
    holed[1, 2, 0] = float("nan")                                           # frame 1, network channel 2: its gain
    holed[2, 0, 1] = float("inf")                                           # frame 2, network channel 0: its offset
    fixed = holed.clone()
    fixed[1, 2], fixed[2, 0] = torch.tensor([1.0, 0.0], device=dev), torch.tensor([1.0, 0.0], device=dev)
    got = pkg.ops.frames_paste_u8_aligned(x, bg, rows, colour=holed, **kw)
    assert torch.equal(got, pkg.ops.frames_paste_u8_aligned(x, bg, rows, colour=fixed, **kw))
    full = pkg.ops.frames_paste_u8_aligned(x, bg, rows, colour=colour, **kw)
    plain = pkg.ops.frames_paste_u8_aligned(x, bg, rows, **kw)
    # bgr frames: network channel 2 is byte 0, network channel 0 is byte 2
    assert torch.equal(got[1, :, :, 0], plain[1, :, :, 0]) and torch.equal(got[1, :, :, 1:], full[1, :, :, 1:]) and not torch.equal(got[1], plain[1])
    assert torch.equal(got[2, :, :, 2], plain[2, :, :, 2]) and torch.equal(got[2, :, :, :2], full[2, :, :, :2]) and torch.equal(got[0], full[0])


# ---- 5. guards ------------------------------------------------------------------------------------------------------------------------
def guarded(dev, nbytes, guard, dtype=torch.uint8):
    """``nbytes`` bytes between two runs of ``guard`` 0xA5 bytes: -> (the whole buffer, the view of the middle as ``dtype``)"""
    raw = torch.full((guard + nbytes + guard,), 0xA5, dtype=torch.uint8, device=dev)
    return raw, raw[guard:guard + nbytes].view(dtype)


def intact(raw, nbytes, guard):
    return bool(torch.all(raw[:guard] == 0xA5)) and bool(torch.all(raw[guard + nbytes:] == 0xA5))


def test_guard_bytes_around_frames_rows_and_workspace(pkg, dev):
    """Regions cut by two edges of the frame and one wholly outside it, an invalid row, bgr, matte and feather: the bytes around
    the frames (at an odd address), around ``colour_out`` and around the workspace are intact after every launcher."""
    import sim_ref as R
    lib, L = pkg._lib.lib(), pkg._lib
    net, N = (16, 16), 5
    rows = torch.tensor([R.rows((35.1, 50.3), 1.3 * 16, 2.0, net), R.rows((2.2, 3.9), 2.3 * 16, -0.4, net), R.rows((20.2, 90.4), 16.0, 0.3, net),
                         R.rows((20.3, 27.6), 20.0, 0.3, net), R.rows((20.3, 27.6), 20.0, 0.3, net)], dtype=torch.float64).float()
    rows[3, 0] = float("nan")
    rows[4, :2] = torch.tensor([0.0, 100.0])
    x, bg, matte = BC.source(13, N, *net), BC.frames(14, N, H, W, 3), BC.matte_for(15, N, *net)
    fguard, nframes = 4 * 3 * W + 1, N * H * W * 3
    raw_f, view = guarded(dev, nframes, fguard)
    view = view.view(N, H, W, 3)
    assert view.data_ptr() % 2 == 1
    view.copy_(bg.to(dev))
    raw_c, colour = guarded(dev, N * 6 * 4, 256, torch.float32)
    colour = colour.view(N, 3, 2)
    need = lib.spk_paste_colour_match_workspace_bytes(N)
    raw_w, ws = guarded(dev, need, 256)
    assert ws.data_ptr() % 8 == 0
    xd, rd, md = x.to(dev), rows.to(dev), matte.to(dev)
    kw = dict(feather=2.5, channel_order="bgr")
    # the statistics through the C entry point, with a workspace of exactly the size it asks for
    L.check(lib.spk_paste_colour_match_sim(xd.data_ptr(), N, *net, view.data_ptr(), view.stride(0), view.stride(1), H, W, rd.data_ptr(), 1, 2.5,
                                           -1.0, 127.5, md.data_ptr(), N, 2.0, 1.0, 16.0, colour.data_ptr(), ws.data_ptr(), need, L.stream_ptr()),
            "spk_paste_colour_match_sim")
    torch.cuda.synchronize()
    assert intact(raw_f, nframes, fguard) and intact(raw_c, N * 24, 256) and intact(raw_w, need, 256)
    assert torch.equal(view.cpu(), bg)                                      # no frame byte written
    assert torch.equal(ws.view(torch.float64).view(N, -1, 13)[2:].cpu(), torch.zeros(3, need // (N * 104), 13, dtype=torch.float64))
    assert colour[2:].cpu().tolist() == [[[1.0, 0.0]] * 3] * 3              # outside the frame, a NaN row, s = 100: by rule
    # the launcher writes the same rows into out=
    again, out = guarded(dev, N * 24, 256, torch.float32)
    assert torch.equal(pkg.ops.paste_colour_match(xd, view, rd, matte=md, out=out.view(N, 3, 2), **kw), colour) and intact(again, N * 24, 256)
    ref = B.blend(x.numpy(), bg.numpy(), rows.numpy(), feather=2.5, swap_rb=True, matte=matte.numpy(), colour=colour.cpu().numpy())
    assert ref["margin"] >= BC.MARGIN
    # the paste, in place
    assert pkg.ops.frames_paste_u8_aligned(xd, view, rd, matte=md, colour=colour, out=view, **kw) is view
    torch.cuda.synchronize()
    assert intact(raw_f, nframes, fguard) and intact(raw_c, N * 24, 256)
    got = view.cpu()
    over = float(np.abs(got.numpy().astype(np.float64) - ref["z"]).max())
    print(f"guards: largest |got - z| = {over:.6f} (bound {TOL_COLOUR}); region pixels per frame {ref['region'].sum((1, 2)).tolist()}")
    assert over <= TOL_COLOUR and np.array_equal(got.numpy()[~ref["region"]], bg.numpy()[~ref["region"]])
    assert 0 < ref["region"][0].sum() and 0 < ref["region"][1].sum() and not ref["region"][2:].any()
    assert torch.equal(got[2:], bg[2:]) and not torch.equal(got[0], bg[0]) and not torch.equal(got[1], bg[1])


# ---- 6. the public interface ----------------------------------------------------------------------------------------------------------
SIZE = 128          # encoder input of the model-level cases, as tests/test_align_gpu.py


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
    """Identity photo, T = 3 BGR video frames of 64 x 80, a transform per frame, explicit noise, a matte in the generated size."""
    T = 3
    rows = pkg.ops.similarity_rows([(30.3, 41.6), (33.9, 38.2), (28.4, 44.1)], [44.0, 52.0, 36.0], [0.2, -0.3, 0.1], SIZE)
    return dict(T=T, ident_u8=BC.frames(31, 56, 72, 3).to(dev), pose_u8=BC.frames(32, T, 64, 80, 3).to(dev), emo_u8=BC.frames(33, T, 64, 80, 3).to(dev),
                rows=rows, noises=[n.to(dev) for n in recipe_noises("frame_io", T, 256)], matte=pkg.ops.ellipse_matte((256, 256), device=dev))


def count_calls(pkg, monkeypatch, names):
    lib = pkg._lib.lib()
    real = {n: getattr(lib, n) for n in names}
    calls = dict.fromkeys(names, 0)

    def counting(name):
        def f(*args):
            calls[name] += 1
            return real[name](*args)
        return f

    for n in names:
        monkeypatch.setattr(lib, n, counting(n))
    return calls


def test_reenact_video_blend_is_its_hand_composition(irfd, pkg, clip, dev, monkeypatch):
    c, ops = clip, pkg.ops
    keep = c["pose_u8"].clone()
    ident = ops.frames_from_u8(c["ident_u8"], SIZE, channel_order="bgr")
    pose, emo = (ops.frames_from_u8_aligned(c[k], SIZE, c["rows"], channel_order="bgr") for k in ("pose_u8", "emo_u8"))
    f32 = irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2)
    half = (c["rows"] * torch.tensor([0.5, 0.5, 1.0, 1.0])).to(dev)        # the generated image has 256 pixels where the network's has 128
    mattes = {"shared": c["matte"], "frames": torch.stack([c["matte"], c["matte"].flip(0) * 0.8, c["matte"].flip(1)]).contiguous()}
    kw = dict(size=SIZE, align=c["rows"], channel_order="bgr", noises=c["noises"], paste=True, feather=4)
    for how, matte in mattes.items():
        colour = ops.paste_colour_match(f32, c["pose_u8"], half, matte=matte, feather=4, channel_order="bgr")
        want = ops.frames_paste_u8_aligned(f32, c["pose_u8"], half, matte=matte, colour=colour, feather=4, channel_order="bgr")
        names = ("spk_paste_colour_match_sim", "spk_frames_paste_u8_sim_blend", "spk_frames_paste_u8_sim")
        calls = count_calls(pkg, monkeypatch, names)
        got = irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], matte=matte, colour_match=True, chunk=2, **kw)
        monkeypatch.undo()
        assert calls == {"spk_paste_colour_match_sim": 2, "spk_frames_paste_u8_sim_blend": 2, "spk_frames_paste_u8_sim": 0}, (how, calls)
        assert got.dtype == torch.uint8 and got.shape == (c["T"], 64, 80, 3) and torch.equal(got, want), how
        assert torch.equal(c["pose_u8"], keep) and got.data_ptr() != c["pose_u8"].data_ptr() and not torch.equal(got, keep)
        # neither chunk nor inplace changes a byte
        assert torch.equal(irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], matte=matte, colour_match=True, chunk=8, **kw), want)
        video = c["pose_u8"].clone()
        assert irfd.reenact_video(c["ident_u8"], video, c["emo_u8"], matte=matte, colour_match=True, chunk=2, inplace=True, **kw) is video
        assert torch.equal(video, want)
    # each of the two alone
    want = ops.frames_paste_u8_aligned(f32, c["pose_u8"], half, matte=c["matte"], feather=4, channel_order="bgr")
    calls = count_calls(pkg, monkeypatch, names)
    got = irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], matte=c["matte"], chunk=2, **kw)
    monkeypatch.undo()
    assert torch.equal(got, want) and calls == {"spk_paste_colour_match_sim": 0, "spk_frames_paste_u8_sim_blend": 2, "spk_frames_paste_u8_sim": 0}
    colour = ops.paste_colour_match(f32, c["pose_u8"], half, feather=4, channel_order="bgr")
    want = ops.frames_paste_u8_aligned(f32, c["pose_u8"], half, colour=colour, feather=4, channel_order="bgr")
    assert torch.equal(irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], colour_match=True, chunk=2, **kw), want)
    plain = ops.frames_paste_u8_aligned(f32, c["pose_u8"], half, feather=4, channel_order="bgr")
    assert not torch.equal(want, plain)


def test_reenact_video_without_the_new_arguments_launches_what_it_did(irfd, pkg, clip, dev, monkeypatch):
    """The counts of tests/test_align_gpu.py's launch test, with the two new entry points counted beside them: zero."""
    c = clip
    kw = dict(size=SIZE, align=c["rows"], channel_order="bgr", paste=True, feather=4, seed=7)
    a = irfd.reenact_video(c["ident_u8"], c["pose_u8"], chunk=1, **kw)
    names = ("spk_frames_paste_u8_sim", "spk_frames_u8_to_f32_sim", "spk_frames_paste_u8", "spk_frames_u8_to_f32_boxes",
             "spk_frames_paste_u8_sim_blend", "spk_paste_colour_match_sim")
    calls = count_calls(pkg, monkeypatch, names)
    b = irfd.reenact_video(c["ident_u8"], c["pose_u8"], chunk=2, **kw)
    monkeypatch.undo()
    assert torch.equal(a, b) and not torch.equal(a, c["pose_u8"])
    assert calls == {"spk_frames_paste_u8_sim": 2, "spk_frames_u8_to_f32_sim": 1, "spk_frames_paste_u8": 0, "spk_frames_u8_to_f32_boxes": 0,
                     "spk_frames_paste_u8_sim_blend": 0, "spk_paste_colour_match_sim": 0}, calls
