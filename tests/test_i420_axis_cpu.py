"""CPU-side checks of the axis-aligned I420 edge (csrc/frame_i420.hip): the argument refusals of the three entry points through
ctypes (they return before a launch, so no GPU is needed), ``SPK_OP_FRAMES_TO_I420`` and its descriptor against include/spk.h, every
host refusal of ``ops.frames_from_i420`` / ``ops.frames_to_i420`` / ``ops.frames_paste_i420``, of ``DecoderPlan(output=)``, of
``IRFD.reenact(output=)`` and of ``IRFD.reenact_video(pixel_format="i420", ...)`` -- each raised before a device is used: the
stream, the device tables and the plan's buffers are replaced by functions that fail the test -- and the packed layout that
``frames_to_i420`` documents, through ``i420_planes``."""
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
    assert "SPK_OP_FRAMES_TO_I420 = SPK_OP_NOISE_FILL_ROWS + 1" in text and L.OP_FRAMES_TO_I420 == L.OP_NOISE_FILL_ROWS + 1 == 15
    body = re.search(r"typedef struct spk_frames_to_i420_args \{(.*?)\} spk_frames_to_i420_args;", text, re.S).group(1)
    names = re.findall(r"\w+(?=\s*[,;])", body)                              # the identifier in front of every , and ;
    assert names == [n for n, _ in L.FramesToI420Args._fields_], names
    assert ctypes.sizeof(L.FramesToI420Args) == 4 * 8 + 6 * 8 + 5 * 4 + 2 * 4 + 4 == 112
    for name in ("spk_frames_i420_to_f32", "spk_frames_f32_to_i420", "spk_frames_paste_i420"):
        assert name in L.exported_symbols() and re.search(rf"\bint {name}\(", text)


def test_the_entry_points_refuse_bad_arguments(pkg):
    """Every refusal comes before a launch and before anything is dereferenced: the pointers are numbers"""
    lib = pkg._lib.lib()
    P, T, F = 0x7000_0000_0000, 0x7100_0000_0000, 0x7200_0000_0000
    S = dict(y=P, yi=96, yr=8, u=P + 65, ui=21, ur=5, v=P + 1024, vi=16, vr=4, N=1, H=8, W=8, std=601, full=0)      # odd U base, pitch, image stride

    def surf(a):
        return (a["y"], a["yi"], a["yr"], a["u"], a["ui"], a["ur"], a["v"], a["vi"], a["vr"])

    def to_f32(dst=F, tab=T, w=T, Hin=4, Win=4, taps=2, Hout=2, Wout=2, **kw):
        a = dict(S, **kw)
        return lib.spk_frames_i420_to_f32(*surf(a), a["N"], a["H"], a["W"], None, 1, 1, Hin, Win, 0, a["std"], a["full"], tab, tab, w, taps, tab, tab, w,
                                          taps, dst, Hout, Wout, 1, 1, 1, 0, 0, 0, None)

    def paste(src=F, tab=T, w=T, ay=None, ax=None, Hs=4, Ws=4, h=4, w_=4, taps=2, lo=-1.0, k=127.5, **kw):
        a = dict(S, **kw)
        return lib.spk_frames_paste_i420(src, a["N"], Hs, Ws, *surf(a), a["H"], a["W"], h, w_, 1, 1, None, a["std"], a["full"], tab, tab, w, taps, tab, tab,
                                         w, taps, ay, ax, lo, k, None)

    def to_i420(src=F, lo=-1.0, k=127.5, **kw):
        a = dict(S, **kw)
        return lib.spk_frames_f32_to_i420(src, a["N"], a["H"], a["W"], *surf(a), a["std"], a["full"], lo, k, None)

    surface = [(dict(y=None), "null plane"), (dict(u=None), "null plane"), (dict(v=None), "null plane"), (dict(N=0), "N must"), (dict(N=-2), "N must"),
               (dict(H=0), "H, W >= 2"), (dict(W=-8), "H, W >= 2"), (dict(H=7), "even height and width"), (dict(W=9), "even height and width"),
               (dict(yr=7), "Y row stride 7"), (dict(ur=3), "U row stride 3"), (dict(vr=3), "V row stride 3"), (dict(vr=-4), "V row stride"),
               (dict(W=2 ** 31 - 2), "Y row stride"), (dict(std=2020), "standard"), (dict(std=0), "standard"), (dict(full=2), "full_range"),
               (dict(full=-1), "full_range")]
    calls = [(lambda f=f, bad=bad: f(**bad), words) for f in (to_f32, paste, to_i420) for bad, words in surface]
    calls += [(lambda bad=bad: to_f32(**bad), words) for bad, words in
              [(dict(dst=None), "null frame pointer"), (dict(tab=None), "null table"), (dict(w=None), "null table"), (dict(Hin=0), "sizes must be"),
               (dict(Win=-1), "sizes must be"), (dict(Hin=10), "does not fit"), (dict(Win=10), "does not fit"), (dict(taps=0), "tap count"),
               (dict(Hout=0), "sizes must be"), (dict(Wout=-1), "sizes must be"), (dict(N=2, yi=-1), "negative image stride"),
               (dict(N=2, ui=-21), "negative image stride"), (dict(N=2, vi=-1), "negative image stride")]]
    written = [(dict(src=None), "null frame pointer"), (dict(lo=math.nan), "value range"), (dict(k=0.0), "value range"), (dict(k=math.inf), "value range"),
               (dict(N=2, yi=63), "overlap"), (dict(N=2, ui=17), "overlap"), (dict(N=2, vi=15), "overlap"), (dict(N=2, yi=0), "overlap"),
               (dict(N=2, ui=-21), "overlap"), (dict(N=2, H=2 ** 31 - 2, yi=64), "overlap"),           # (H - 1) * row stride: 64-bit, no wrap
               (dict(N=2, H=2 ** 31 - 2, yi=2 ** 34 - 9, ui=2 ** 32), "overlap")]      # Y clears its extent 2^34 - 16; U's, 5 * 2^30, is past 32 bits
    calls += [(lambda f=f, bad=bad: f(**bad), words) for f in (paste, to_i420) for bad, words in written]
    calls += [(lambda bad=bad: paste(**bad), words) for bad, words in
              [(dict(tab=None), "null table"), (dict(w=None), "null table"), (dict(ay=T), "feather"), (dict(ax=T), "feather"), (dict(Hs=0), "sizes must be"),
               (dict(Ws=-1), "sizes must be"), (dict(h=0), "sizes must be"), (dict(w_=0), "sizes must be"), (dict(taps=0), "tap count")]]
    for n, (call, words) in enumerate(calls):
        assert call() == -1 and words in lib.spk_last_error().decode(), (n, words, lib.spk_last_error().decode())
    # a surface that passes is refused for what FOLLOWS the surface check: odd chroma base and pitch, V before U, planes far apart
    for bad in (dict(), dict(u=P + 2048, v=P + 1025, vr=7), dict(u=2 ** 40 + 1, v=2 ** 41), dict(N=2, yi=64, ui=17 - 1 + 4, vi=16)):
        assert to_f32(dst=None, **bad) == -1 and "null frame pointer" in lib.spk_last_error().decode(), bad
        assert paste(k=0.0, **bad) == -1 and "value range" in lib.spk_last_error().decode(), bad
        assert to_i420(k=0.0, **bad) == -1 and "value range" in lib.spk_last_error().decode(), bad


# ---- the launchers --------------------------------------------------------------------------------------------------------------------
def test_launchers_refuse_cpu_tensors_and_bad_arguments(pkg, no_device):
    ops, SpkError = pkg.ops, pkg._lib.SpkError
    surf = u8(2, 12, 8)
    triple = (u8(2, 8, 8), u8(2, 4, 4), u8(2, 4, 4))
    for frames in (surf, triple):
        with pytest.raises(SpkError, match="HIP|device|CPU"):
            ops.frames_from_i420(frames, 4)
        for bad in (dict(channel_order="gbr"), dict(crop=(4, 4, 8, 2)), dict(std=(0.5, 0.0, 0.5)), dict(standard="bt2020"), dict(full_range=3)):
            with pytest.raises(ValueError):
                ops.frames_from_i420(frames, 4, **bad)
        with pytest.raises(ValueError):
            ops.frames_from_i420(frames, 0)
    for bad in (u8(2, 8, 8, 3), surf[:, :, ::2], u8(2, 12, 7), (u8(2, 8, 8), u8(2, 4, 4)), (u8(2, 8, 8), u8(2, 4, 4), u8(2, 4, 3)),
                (u8(2, 8, 8), u8(2, 4, 4), torch.zeros(2, 4, 4)), torch.zeros(2, 12, 8), u8(2, 12, 16)[:, :, :8], "yuv"):
        with pytest.raises(ValueError, match="i420"):                        # packed RGB, a pixel stride, odd sizes, pairs, a pitched packed tensor
            ops.frames_from_i420(bad, 4)
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_to_i420(x)
    for bad in (dict(value_range=(1, 1)), dict(standard="rec709"), dict(full_range="yes")):
        with pytest.raises(ValueError):
            ops.frames_to_i420(x, **bad)
    for bad in (torch.zeros(2, 3, 7, 8), torch.zeros(2, 3, 8, 6 + 1), torch.zeros(2, 8, 8, 3)):
        with pytest.raises(ValueError):
            ops.frames_to_i420(bad)
    with pytest.raises(ValueError, match="I420 frames have an even height and width"):
        ops.frames_to_i420(torch.zeros(2, 3, 7, 8))
    for frames in (surf, triple):
        with pytest.raises(SpkError, match="HIP|device|CPU"):
            ops.frames_paste_i420(x, frames, (0, 0, 4, 4))
        for bad in (dict(feather=-1), dict(feather=float("nan")), dict(value_range=(1, 0)), dict(standard="bt2020"), dict(full_range=2)):
            with pytest.raises(ValueError):
                ops.frames_paste_i420(x, frames, (0, 0, 4, 4), **bad)
        with pytest.raises(ValueError):
            ops.frames_paste_i420(x, frames, (0, 0, 0, 4))
    with pytest.raises(ValueError, match="2 generated frames, 1 I420 frames"):
        ops.frames_paste_i420(x, surf[:1], (0, 0, 4, 4))                     # one surface for two frames
    with pytest.raises(ValueError):
        ops.frames_paste_i420(x, u8(2, 8, 8, 3), (0, 0, 4, 4))
    with pytest.raises(ValueError):
        ops.frames_paste_i420(torch.zeros(2, 8, 8, 3), surf, (0, 0, 4, 4))


def test_plan_and_reenact_output_refusals(pkg, no_device):
    import model
    with pytest.raises(ValueError, match="output must be 'f32', 'uint8', 'nv12' or 'i420', got 'nv21'"):
        pkg.plan.DecoderPlan(None, 2, torch.device("cpu"), output="nv21")
    with pytest.raises(ValueError, match="output must be"):
        pkg.plan.DecoderPlan(None, 2, torch.device("cpu"), output="yuv420p")
    m = model.IRFD()
    img, frames = torch.zeros(1, 3, 64, 64), torch.zeros(3, 3, 64, 64)
    with pytest.raises(ValueError, match="output must be 'f32', 'uint8', 'nv12' or 'i420', got 'nv21'"):
        m.reenact(img, frames, output="nv21")
    with pytest.raises(ValueError, match="output must be"):
        m.reenact(img, frames, output="I420")
    with pytest.raises(ValueError, match="channel_order"):
        m.reenact(img, frames, output="i420", channel_order="bgr")
    with pytest.raises(ValueError, match="standard must be"):
        m.reenact(img, frames, output="i420", standard="bt2020")
    with pytest.raises(ValueError, match="full_range must be"):
        m.reenact(img, frames, output="i420", full_range=2)
    for output in ("f32", "uint8"):
        with pytest.raises(ValueError, match="standard / full_range apply to nv12 output only, and to i420"):
            m.reenact(img, frames, output=output, standard="bt709")
    with pytest.raises(ValueError, match="frame0"):
        m.reenact(img, frames, output="i420", frame0=3)
    with pytest.raises(ValueError, match="emotion_frames"):
        m.reenact(img, frames, frames[:2], output="i420")
    with pytest.raises(Exception) as e:                                      # past every host check: the encoder is next, which has no CPU path
        m.reenact(img, frames, output="i420", standard="bt709", full_range=True)
    assert not isinstance(e.value, (ValueError, AssertionError)), e.value


def test_reenact_video_i420_argument_errors(pkg, no_device):
    import model
    m = model.IRFD()
    ident, surf, rgb = u8(16, 16, 3), u8(3, 24, 16), u8(3, 16, 16, 3)
    triple = (u8(3, 16, 16), u8(3, 8, 8), u8(3, 8, 8))
    rows = [(1.0, 0.0, 8.0, 8.0)] * 3
    for name in ("yuv420p", "I420", "yv12", "nv21"):
        with pytest.raises(ValueError, match="pixel_format must be 'rgb24' or 'nv12' or 'i420'"):
            m.reenact_video(ident, surf, pixel_format=name)
    for colour in (dict(standard="bt709"), dict(full_range=True)):
        with pytest.raises(ValueError, match="standard / full_range apply to pixel_format='nv12' only, and to 'i420'"):
            m.reenact_video(ident, rgb, **colour)
    for frames in (surf, triple):
        i420 = lambda **kw: m.reenact_video(ident, frames, pixel_format="i420", **kw)
        with pytest.raises(ValueError, match="standard must be"):
            i420(standard="bt2020")
        with pytest.raises(ValueError, match="full_range must be"):
            i420(full_range=2)
        with pytest.raises(ValueError, match="crop"):
            i420(crop=(0, 0, 17, 4))                                         # the box leaves the 16 x 16 frame
        with pytest.raises(ValueError, match="crop"):
            i420(crop=[(0, 0, 8, 8)] * 2)                                    # two boxes for three frames
        with pytest.raises(ValueError, match="inplace"):
            i420(inplace=True)                                               # inplace applies to paste=True only
        with pytest.raises(ValueError, match="feather"):
            i420(feather=2)
        with pytest.raises(ValueError, match="feather"):
            i420(paste=True, feather=-1)
        with pytest.raises(ValueError, match="seed"):
            i420(noise="fixed")
        with pytest.raises(ValueError, match="align applies to pixel_format='rgb24' only"):
            i420(align=rows)
        with pytest.raises(ValueError, match="align"):
            i420(align=rows, paste=True, matte=torch.zeros(4, 4))
        with pytest.raises(ValueError, match="align"):
            i420(paste=True, matte=torch.zeros(4, 4))
        with pytest.raises(ValueError, match="align"):
            i420(paste=True, colour_match=True)
        with pytest.raises(ValueError, match="align"):
            i420(align=rows, paste=True, colour_match=True)
        with pytest.raises(ValueError, match="colour_match"):
            i420(paste=True, colour_smooth=2)
        with pytest.raises(ValueError, match="identity_align"):
            i420(identity_align=[(1.0, 0.0, 8.0, 8.0)] * 2)                  # one photo, two rows
    for bad in (rgb, u8(3, 24, 32)[:, :, :16], u8(3, 24, 15), (u8(3, 16, 16), u8(3, 8, 8)), (u8(3, 16, 16), u8(3, 8, 8, 2)),
                (u8(3, 16, 16), u8(3, 8, 8), u8(3, 8, 4))):
        with pytest.raises(ValueError, match="i420"):                        # packed RGB, a pitched packed tensor, an odd width, NV12 pairs
            m.reenact_video(ident, bad, pixel_format="i420")
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):           # every host check passed: the photo is next, and has no CPU path
        m.reenact_video(ident, surf, pixel_format="i420", paste=True, inplace=True, standard="bt709", full_range=True)


# ---- the packed layout ----------------------------------------------------------------------------------------------------------------
def test_i420_planes_round_trips_the_packed_layout(pkg):
    """``frames_to_i420`` documents a packed ``[N, 3H/2, W]`` result: the ``H`` rows of Y, then the ``HW/4`` bytes of U, then those of
    V.  ``i420_planes`` gives exactly those bytes back as views, for a width whose half is odd too."""
    for N, H, W in ((2, 4, 6), (1, 2, 2), (3, 6, 8)):
        g = torch.Generator().manual_seed(H * W)
        y, u, v = (torch.randint(0, 256, s, generator=g, dtype=torch.uint8) for s in ((N, H, W), (N, H // 2, W // 2), (N, H // 2, W // 2)))
        packed = torch.cat([y.flatten(1), u.flatten(1), v.flatten(1)], 1).view(N, 3 * H // 2, W)
        py, pu, pv = pkg.ops.i420_planes(packed)
        assert torch.equal(py, y) and torch.equal(pu, u) and torch.equal(pv, v)
        assert py.data_ptr() == packed.data_ptr() and pu.data_ptr() == packed.data_ptr() + H * W and pv.data_ptr() == pu.data_ptr() + H * W // 4
        if N > 1:                                                            # (the strides of a dimension of one entry say nothing)
            assert (pu.stride(1), pv.stride(1)) == (W // 2, W // 2) and pu.stride(0) == pv.stride(0) == 3 * H * W // 2      # W = 6: the odd pitch 3
        pu.fill_(7), pv.fill_(9)                                             # views: a launcher that writes the planes writes the tensor
        assert torch.equal(packed.view(N, -1)[:, H * W:], torch.cat([torch.full((N, H * W // 4), 7), torch.full((N, H * W // 4), 9)], 1).to(torch.uint8))
        ty, tu, tv = pkg.ops.i420_planes((py, pu, pv))                       # a triple passes through as it is
        assert ty is py and tu is pu and tv is pv
