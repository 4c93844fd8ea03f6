"""CPU-side checks of the axis-aligned RGB32 edge (csrc/frame_rgb32.hip): the argument refusals of the four entry points through
ctypes (they return before a launch, so no GPU is needed), ``SPK_OP_FRAMES_TO_RGB32`` and its descriptor against include/spk.h,
every host refusal of ``ops.frames_from_rgb32`` / ``ops.frames_to_rgb32`` / ``ops.frames_paste_rgb32``, of
``DecoderPlan(output="rgb32")``, of ``IRFD.reenact(output="rgb32")`` and of ``IRFD.reenact_video(pixel_format="rgb32", ...)`` -- each
raised before a device is used: the stream, the device tables and the plan's buffers are replaced by functions that fail the test --
and the error texts the older tests pin, for the inputs they use."""
import ctypes
import importlib
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")


@pytest.fixture
def no_device(pkg, monkeypatch):
    """Whatever a launcher does once its host checks are through fails the test"""
    def touched(*a, **k):
        raise AssertionError("a device was used before the host refusal")
    monkeypatch.setattr(pkg._lib, "stream_ptr", touched)
    monkeypatch.setattr(pkg.frames, "_device_tables", touched)
    monkeypatch.setattr(pkg.frames, "_paste_tables", touched)
    monkeypatch.setattr(pkg.plan.LaunchPlan, "buf", touched)


# ---- the C interface ------------------------------------------------------------------------------------------------------------------
def test_the_op_kind_and_its_descriptor_mirror_the_header(pkg):
    L = pkg._lib
    text = open(os.path.join(ROOT, "include", "spk.h")).read()
    assert "SPK_OP_FRAMES_TO_RGB32 = SPK_OP_FRAMES_TO_I420 + 1" in text and L.OP_FRAMES_TO_RGB32 == L.OP_FRAMES_TO_I420 + 1 == 16
    body = re.search(r"typedef struct spk_frames_to_rgb32_args \{(.*?)\} spk_frames_to_rgb32_args;", text, re.S).group(1)
    names = re.findall(r"\w+(?=\s*[,;])", body)                              # the identifier in front of every , and ;
    assert names == [n for n, _ in L.FramesToRgb32Args._fields_], names
    assert names[:12] == ["x", "y", "image_stride", "row_stride", "N", "H", "W", "swap_rb", "alpha_first", "alpha", "lo", "k"]
    assert ctypes.sizeof(L.FramesToRgb32Args) == 4 * 8 + 6 * 4 + 2 * 4 == 64 and ctypes.sizeof(L.FramesToRgb32Args) % 8 == 0
    for name in ("spk_frames_rgb32_to_f32", "spk_frames_rgb32_to_f32_boxes", "spk_frames_paste_rgb32", "spk_frames_f32_to_rgb32"):
        assert name in L.exported_symbols() and re.search(rf"\bint {name}\(", text)
    assert "alpha = -1 means KEEP" in text                                   # the header says what alpha means on the way out


def test_the_entry_points_refuse_bad_arguments(pkg):
    """Every refusal comes before a launch and before anything is dereferenced: the pointers are numbers"""
    lib = pkg._lib.lib()
    P, T, F = 0x7000_0000_0000, 0x7100_0000_0000, 0x7200_0000_0000
    S = dict(px=P + 64, img=384, row=48, N=1, H=8, W=8, swap=1, af=0)         # 8 x 8 frames at pitch 48: 4 W = 32

    def to_f32(dst=F, tab=T, w=T, taps=2, Hout=2, Wout=2, **kw):
        a = dict(S, **kw)
        return lib.spk_frames_rgb32_to_f32(a["px"], a["img"], a["row"], a["N"], a["H"], a["W"], a["swap"], a["af"], tab, tab, w, taps, tab, tab, w, taps,
                                           dst, Hout, Wout, 1, 1, 1, 0, 0, 0, None)

    def boxes(dst=F, tab=T, w=T, yx=T, Hin=4, Win=4, taps=2, Hout=2, Wout=2, **kw):
        a = dict(S, **kw)
        return lib.spk_frames_rgb32_to_f32_boxes(a["px"], a["img"], a["row"], a["N"], a["H"], a["W"], yx, Hin, Win, a["swap"], a["af"], tab, tab, w,
                                                 taps, tab, tab, w, taps, dst, Hout, Wout, 1, 1, 1, 0, 0, 0, None)

    def paste(src=F, tab=T, w=T, ay=None, ax=None, Hs=4, Ws=4, h=4, w_=4, taps=2, lo=-1.0, k=127.5, **kw):
        a = dict(S, **kw)
        return lib.spk_frames_paste_rgb32(src, a["N"], Hs, Ws, a["px"], a["img"], a["row"], a["H"], a["W"], h, w_, 1, 1, None, a["swap"], a["af"], tab,
                                          tab, w, taps, tab, tab, w, taps, ay, ax, lo, k, None)

    def to_rgb32(src=F, alpha=255, lo=-1.0, k=127.5, **kw):
        a = dict(S, **kw)
        return lib.spk_frames_f32_to_rgb32(src, a["px"], a["img"], a["row"], a["N"], a["H"], a["W"], a["swap"], a["af"], alpha, lo, k, None)

    frames = [(dict(px=None), "null frame pointer"), (dict(N=0), "N / H / W"), (dict(N=-2), "N / H / W"), (dict(row=31), "smaller than 4 * W"),
              (dict(row=24), "smaller than 4 * W"), (dict(row=-48), "smaller than 4 * W"), (dict(W=2 ** 31 - 1), "smaller than 4 * W"),
              (dict(row=49), "not a multiple of 4"), (dict(row=50), "not a multiple of 4"), (dict(row=51), "not a multiple of 4"),
              (dict(N=2, img=386), "image stride 386 is not a multiple of 4"), (dict(px=P + 65), "aligned to 4 bytes"),
              (dict(px=P + 66), "aligned to 4 bytes"), (dict(px=P + 67), "aligned to 4 bytes"), (dict(af=2), "alpha_first"), (dict(af=-1), "alpha_first")]
    calls = [(lambda f=f, bad=bad: f(**bad), words) for f in (to_f32, boxes, paste, to_rgb32) for bad, words in frames]
    calls += [(lambda f=f, bad=bad: f(**bad), words) for f in (to_f32, paste, to_rgb32) for bad, words in
              [(dict(H=0), "N / H / W"), (dict(W=-8), "N / H / W")]]
    calls += [(lambda f=f, bad=bad: f(**bad), words) for f in (to_f32, boxes) for bad, words in
              [(dict(dst=None), "null frame pointer"), (dict(tab=None), "null table"), (dict(w=None), "null table"), (dict(taps=0), "tap count"),
               (dict(Hout=0), "N / H / W"), (dict(Wout=-1), "N / H / W"), (dict(N=2, img=-384), "negative image stride"),
               (dict(N=2, img=-4), "negative image stride")]]
    calls += [(lambda bad=bad: boxes(**bad), words) for bad, words in
              [(dict(yx=None), "null box origin"), (dict(Hin=0), "N / H / W"), (dict(Win=-1), "N / H / W"), (dict(Hin=9), "does not fit"),
               (dict(Win=9), "does not fit"), (dict(H=0), "does not fit")]]
    written = [(dict(src=None), "null frame pointer"), (dict(lo=math.nan), "value range"), (dict(k=0.0), "value range"), (dict(k=math.inf), "value range"),
               (dict(N=2, img=364), "overlap"), (dict(N=2, img=0), "overlap"), (dict(N=2, img=-384), "overlap"),
               (dict(N=2, H=2 ** 31 - 2, img=384), "overlap"),              # (H - 1) * row stride: 64-bit, no wrap
               (dict(N=2, row=2 ** 32 + 48, img=368), "overlap")]           # the pitch 48 if it wrapped, whose extent 368 would pass
    calls += [(lambda f=f, bad=bad: f(**bad), words) for f in (paste, to_rgb32) for bad, words in written]
    calls += [(lambda bad=bad: paste(**bad), words) for bad, words in
              [(dict(tab=None), "null table"), (dict(w=None), "null table"), (dict(ay=T), "feather"), (dict(ax=T), "feather"), (dict(Hs=0), "N / H / W"),
               (dict(Ws=-1), "N / H / W"), (dict(h=0), "N / H / W"), (dict(w_=0), "N / H / W"), (dict(taps=0), "tap count")]]
    calls += [(lambda bad=bad: to_rgb32(**bad), words) for bad, words in
              [(dict(alpha=256), "alpha must be"), (dict(alpha=-2), "alpha must be"), (dict(alpha=2 ** 31 - 1), "alpha must be")]]
    for n, (call, words) in enumerate(calls):
        assert call() == -1 and words in lib.spk_last_error().decode(), (n, words, lib.spk_last_error().decode())
    # frames that pass are refused for what FOLLOWS the frames check: a view that is 4-aligned and not 16-aligned, frames that touch,
    # the smallest frame, argb, keep
    for ok in (dict(), dict(px=P + 64 + 48 * 3 + 20), dict(N=2, img=368), dict(H=1, W=1, row=4), dict(af=1, swap=0), dict(img=3)):
        assert paste(k=0.0, **ok) == -1 and "value range" in lib.spk_last_error().decode(), ok
        assert to_rgb32(k=0.0, **ok) == -1 and "value range" in lib.spk_last_error().decode(), ok
        assert to_rgb32(k=0.0, alpha=-1, **ok) == -1 and "value range" in lib.spk_last_error().decode(), ok
        assert to_rgb32(alpha=300, **ok) == -1 and "alpha must be" in lib.spk_last_error().decode(), ok


# ---- the launchers --------------------------------------------------------------------------------------------------------------------
def test_launchers_refuse_cpu_tensors_and_bad_arguments(pkg, no_device):
    ops, SpkError = pkg.ops, pkg._lib.SpkError
    frames = u8(2, 8, 8, 4)
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_from_rgb32(frames, 4)
    for bad in (dict(channel_order="rgb"), dict(channel_order="bgr"), dict(channel_order="rgbx"), dict(channel_order=None), dict(crop=(4, 4, 8, 2)),
                dict(crop=[(0, 0, 4, 4)]), dict(std=(0.5, 0.0, 0.5)), dict(mean=(0.5, 0.5))):
        with pytest.raises(ValueError):
            ops.frames_from_rgb32(frames, 4, **bad)
    with pytest.raises(ValueError, match="channel_order must be one of 'rgba', 'bgra', 'argb', 'abgr'"):
        ops.frames_from_rgb32(frames, 4, channel_order="rgb")
    with pytest.raises(ValueError):
        ops.frames_from_rgb32(frames, 0)
    for bad in (u8(2, 8, 8, 3), u8(2, 8, 8), u8(0, 8, 8, 4), u8(2, 2, 8, 8, 4), "bgra"):
        with pytest.raises(ValueError, match=r"\[N,H,W,4\]"):                # packed RGB, a surface, no frame, a batch of clips, no tensor
            ops.frames_from_rgb32(bad, 4)

    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_to_rgb32(x)
    for bad in (dict(value_range=(1, 1)), dict(channel_order="rgb"), dict(channel_order="RGBA"), dict(alpha=256), dict(alpha=-1), dict(alpha=1.5),
                dict(alpha=True), dict(alpha="opaque")):
        with pytest.raises(ValueError):
            ops.frames_to_rgb32(x, **bad)
    with pytest.raises(ValueError, match="alpha=None"):
        ops.frames_to_rgb32(x, alpha=None)                                   # keep, and nothing to keep
    for bad in (torch.zeros(2, 4, 8, 8), torch.zeros(2, 8, 8, 3), torch.zeros(3, 8, 8)):
        with pytest.raises(ValueError):
            ops.frames_to_rgb32(bad)

    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_paste_rgb32(x, frames, (0, 0, 4, 4))
    for bad in (dict(feather=-1), dict(feather=float("nan")), dict(value_range=(1, 0)), dict(channel_order="bgr"), dict(channel_order="gbra")):
        with pytest.raises(ValueError):
            ops.frames_paste_rgb32(x, frames, (0, 0, 4, 4), **bad)
    with pytest.raises(ValueError):
        ops.frames_paste_rgb32(x, frames, (0, 0, 0, 4))
    with pytest.raises(ValueError, match=r"\[2,H,W,4\]"):
        ops.frames_paste_rgb32(x, frames[:1], (0, 0, 4, 4))                  # one frame for two generated ones
    with pytest.raises(ValueError):
        ops.frames_paste_rgb32(x, u8(2, 8, 8, 3), (0, 0, 4, 4))
    with pytest.raises(ValueError):
        ops.frames_paste_rgb32(torch.zeros(2, 8, 8, 3), frames, (0, 0, 4, 4))


def test_written_frames_that_do_not_fit_are_refused(pkg, monkeypatch):
    """``out=`` of the way out and of the paste: the checks of ``rgb32_pixels`` come before a launch.  The tensors are CPU tensors made
    to look like device tensors to the two checks in front (``is_cuda``, ``L.dptr``): nothing here reaches the library"""
    ops, SpkError, FR = pkg.ops, pkg._lib.SpkError, pkg.frames
    raw = torch.zeros(4096, dtype=torch.uint8)
    base = (-raw.data_ptr()) % 16
    good = raw[base:base + 2 * 8 * 8 * 4].view(2, 8, 8, 4)
    assert FR.rgb32_pixels(good) and FR.rgb32_pixels(raw[base + 4:base + 4 + 512].view(2, 8, 8, 4)) and FR.rgb32_pixels(good[:, 1:6, 2:7])
    misaligned = raw[base + 1:base + 1 + 512].view(2, 8, 8, 4)
    overlapping = raw.as_strided((2, 8, 8, 4), (128, 32, 4, 1), base)        # the second frame begins inside the first
    rows_overlap = raw.as_strided((2, 8, 8, 4), (512, 16, 4, 1), base)
    odd_pitch = raw.as_strided((2, 8, 8, 4), (512, 34, 4, 1), base)
    odd_frames = raw.as_strided((2, 8, 8, 4), (514, 32, 4, 1), base)
    pixel_stride = raw.as_strided((2, 8, 8, 4), (1024, 64, 8, 1), base)
    bad = dict(misaligned=misaligned, overlapping=overlapping, rows_overlap=rows_overlap, odd_pitch=odd_pitch, odd_frames=odd_frames,
               pixel_stride=pixel_stride)
    assert not any(FR.rgb32_pixels(t) for t in bad.values())

    def reached(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(pkg._lib, "dptr", lambda t, name="tensor": 0x7000_0000_0000)
    monkeypatch.setattr(pkg._lib, "lib", reached)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    x = torch.zeros(2, 3, 8, 8)
    for name, out in bad.items():
        with pytest.raises(SpkError, match="aligned 32-bit words"):
            ops.frames_to_rgb32(x, out=out)
        with pytest.raises(SpkError, match="aligned 32-bit words"):
            ops.frames_to_rgb32(x, out=out, alpha=None)
        with pytest.raises(SpkError, match="aligned 32-bit words"):
            ops.frames_paste_rgb32(x, good, (0, 0, 4, 4), out=out)
        with pytest.raises(SpkError, match="aligned 32-bit words"):
            ops.frames_paste_rgb32(x, out, (0, 0, 4, 4), out=out)            # in place
    for out in (torch.zeros(2, 8, 8, 4), u8(2, 8, 8, 3), u8(1, 8, 8, 4), u8(2, 8, 4, 4)):
        with pytest.raises(SpkError, match="out: expected a uint8 HIP tensor"):
            ops.frames_to_rgb32(x, out=out)
        with pytest.raises(SpkError, match="out: expected a uint8 HIP tensor"):
            ops.frames_paste_rgb32(x, good, (0, 0, 4, 4), out=out)


# ---- plans and the model --------------------------------------------------------------------------------------------------------------
def test_plan_and_reenact_output_refusals(pkg, no_device):
    import model
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="output must be 'f32', 'uint8', 'nv12' or 'i420', got 'nv21'"):
        pkg.plan.DecoderPlan(None, 2, cpu, output="nv21")
    with pytest.raises(ValueError, match="rgb32"):
        pkg.plan.DecoderPlan(None, 2, cpu, output="rgba")                    # the message names the new output
    for alpha in (256, -1, 1.0, None, "255"):
        with pytest.raises(ValueError, match="alpha"):
            pkg.plan.DecoderPlan(None, 2, cpu, output="rgb32", alpha=alpha)
    for output in ("f32", "uint8", "nv12", "i420"):
        with pytest.raises(ValueError, match="alpha_first / alpha apply to rgb32 output only"):
            pkg.plan.DecoderPlan(None, 2, cpu, output=output, alpha=0)
        with pytest.raises(ValueError, match="alpha_first / alpha apply to rgb32 output only"):
            pkg.plan.DecoderPlan(None, 2, cpu, output=output, alpha_first=True)
    with pytest.raises(Exception) as e:                                      # past the argument checks: the plan is built next (no synthesis: fails)
        pkg.plan.DecoderPlan(None, 2, cpu, output="rgb32", swap_rb=True, alpha_first=True, alpha=0)
    assert not isinstance(e.value, ValueError), e.value
    m = model.IRFD()
    feats = torch.zeros(2, 6144)
    for bad in (dict(channel_order="rgb"), dict(channel_order="bgr"), dict(swap_rb=True)):
        with pytest.raises(ValueError):
            m.Gd.plan_forward(feats, output="rgb32", **bad)
    for output in ("f32", "uint8", "nv12", "i420"):
        with pytest.raises(ValueError, match="channel_order / alpha apply to rgb32 output only"):
            m.Gd.plan_forward(feats, output=output, channel_order="bgra")
        with pytest.raises(ValueError, match="channel_order / alpha apply to rgb32 output only"):
            m.Gd.plan_forward(feats, output=output, alpha=0)
    img, frames = torch.zeros(1, 3, 64, 64), torch.zeros(3, 3, 64, 64)
    with pytest.raises(ValueError, match="output must be 'f32', 'uint8', 'nv12' or 'i420', got 'nv21'"):
        m.reenact(img, frames, output="nv21")
    with pytest.raises(ValueError, match="output must be"):
        m.reenact(img, frames, output="RGB32")
    with pytest.raises(ValueError, match="channel_order must be one of 'rgba', 'bgra', 'argb', 'abgr', got 'rgb'"):
        m.reenact(img, frames, output="rgb32")                               # the default order is none of the four
    with pytest.raises(ValueError, match="channel_order must be one of"):
        m.reenact(img, frames, output="rgb32", channel_order="bgr")
    for output in ("f32", "uint8", "rgb32"):
        with pytest.raises(ValueError, match="standard / full_range apply to nv12 output only, and to i420"):
            m.reenact(img, frames, output=output, standard="bt709", channel_order="bgra" if output == "rgb32" else "rgb")
    with pytest.raises(ValueError, match="standard / full_range apply to nv12 output only, and to i420"):
        m.reenact(img, frames, output="rgb32", channel_order="bgra", full_range=True)
    # for every other output the channel_order checks and their messages are what they were
    with pytest.raises(ValueError, match="reenact: channel_order must be 'rgb' or 'bgr', got 'bgra'"):
        m.reenact(img, frames, output="uint8", channel_order="bgra")
    with pytest.raises(ValueError, match="reenact: channel_order applies to uint8 output only"):
        m.reenact(img, frames, output="f32", channel_order="bgr")
    with pytest.raises(ValueError, match="reenact: channel_order applies to uint8 output only"):
        m.reenact(img, frames, output="i420", channel_order="bgr")
    with pytest.raises(ValueError, match="frame0"):
        m.reenact(img, frames, output="rgb32", channel_order="argb", frame0=3)
    with pytest.raises(ValueError, match="emotion_frames"):
        m.reenact(img, frames, frames[:2], output="rgb32", channel_order="argb")
    with pytest.raises(ValueError, match="seed"):
        m.reenact(img, frames, output="rgb32", channel_order="argb", noise="fixed")
    for order in ("rgba", "bgra", "argb", "abgr"):
        with pytest.raises(Exception) as e:                                  # past every host check: the encoder is next, which has no CPU path
            m.reenact(img, frames, output="rgb32", channel_order=order)
        assert not isinstance(e.value, (ValueError, AssertionError)), e.value


def test_reenact_video_rgb32_argument_errors(pkg, no_device):
    """What ``test_reenact_video_i420_argument_errors`` checks, where it applies to RGB32, and what is RGB32's own"""
    import model
    m = model.IRFD()
    ident, clip, rgb = u8(16, 16, 3), u8(3, 16, 16, 4), u8(3, 16, 16, 3)
    rows = [(1.0, 0.0, 8.0, 8.0)] * 3
    for name in ("yuv420p", "I420", "yv12", "nv21", "rgba", "RGB32", "bgra", "rgb48"):
        with pytest.raises(ValueError, match="pixel_format must be 'rgb24' or 'nv12' or 'i420'"):
            m.reenact_video(ident, clip, pixel_format=name)
    with pytest.raises(ValueError, match="pixel_format must be 'rgb24' or 'nv12' or 'i420' or 'rgb32', got 'rgba'"):
        m.reenact_video(ident, clip, pixel_format="rgba")
    for colour in (dict(standard="bt709"), dict(full_range=True)):
        with pytest.raises(ValueError, match="standard / full_range apply to pixel_format='nv12' only, and to 'i420'"):
            m.reenact_video(ident, rgb, **colour)                            # rgb24, as ever
        with pytest.raises(ValueError, match="standard / full_range apply to pixel_format='nv12' only, and to 'i420'"):
            m.reenact_video(ident, clip, pixel_format="rgb32", channel_order="bgra", **colour)
    with pytest.raises(ValueError, match="channel_order must be one of 'rgba', 'bgra', 'argb', 'abgr', got 'rgb'"):
        m.reenact_video(ident, clip, pixel_format="rgb32")                   # the default order is none of the four
    with pytest.raises(ValueError, match="channel_order must be one of"):
        m.reenact_video(ident, clip, pixel_format="rgb32", channel_order="bgr")
    for name in ("nv12", "i420"):                                            # that refusal stays
        surf = u8(3, 24, 16)
        with pytest.raises(ValueError, match="align applies to pixel_format='rgb24' only"):
            m.reenact_video(ident, surf, pixel_format=name, align=rows)
    rgb32 = lambda **kw: m.reenact_video(ident, clip, pixel_format="rgb32", channel_order="bgra", **kw)
    with pytest.raises(ValueError, match="standard / full_range apply"):
        rgb32(standard="bt2020")
    with pytest.raises(ValueError, match="crop"):
        rgb32(crop=(0, 0, 17, 4))                                            # the box leaves the 16 x 16 frame
    with pytest.raises(ValueError, match="crop"):
        rgb32(crop=[(0, 0, 8, 8)] * 2)                                       # two boxes for three frames
    with pytest.raises(ValueError, match="inplace"):
        rgb32(inplace=True)                                                  # inplace applies to paste=True only
    with pytest.raises(ValueError, match="feather"):
        rgb32(feather=2)
    with pytest.raises(ValueError, match="feather"):
        rgb32(paste=True, feather=-1)
    with pytest.raises(ValueError, match="seed"):
        rgb32(noise="fixed")
    with pytest.raises(ValueError, match="crop and align"):
        rgb32(align=rows, crop=(0, 0, 8, 8))
    with pytest.raises(ValueError, match="align"):
        rgb32(paste=True, matte=torch.zeros(4, 4))                           # a matte needs align=
    with pytest.raises(ValueError, match="align"):
        rgb32(paste=True, colour_match=True)
    with pytest.raises(ValueError, match="paste=True"):
        rgb32(align=rows, colour_match=True)                                 # and paste=True
    with pytest.raises(ValueError, match="colour_match"):
        rgb32(paste=True, colour_smooth=2)
    with pytest.raises(ValueError, match="matte must be"):
        rgb32(align=rows, paste=True, matte=torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="per-frame matte"):
        rgb32(align=rows, paste=True, matte=torch.zeros(2, 4, 4))            # two matte frames for three frames
    with pytest.raises(ValueError, match="align"):
        rgb32(align=rows[:2])                                                # two rows for three frames
    with pytest.raises(ValueError, match="identity_align"):
        rgb32(identity_align=[(1.0, 0.0, 8.0, 8.0)] * 2)                     # one photo, two rows
    for bad in (rgb, u8(3, 24, 16), u8(16, 16, 4), u8(0, 16, 16, 4), (clip, clip)):
        with pytest.raises(ValueError, match=r"\[T,H,W,4\]"):                # packed RGB, a surface, one frame, no frame, a pair
            m.reenact_video(ident, bad, pixel_format="rgb32", channel_order="bgra", paste=True)
    with pytest.raises(pkg._lib.SpkError, match="inplace needs pixels that are aligned 32-bit words"):      # a byte stride of 2 inside a pixel
        m.reenact_video(ident, u8(3, 16, 16, 8)[..., ::2], pixel_format="rgb32", channel_order="bgra", paste=True, inplace=True)
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):           # every host check passed: the photo is next, and has no CPU path
        rgb32(paste=True, inplace=True, align=rows, matte=torch.zeros(4, 4), colour_match=True, colour_smooth=2)
