"""CPU checks of the colour rows pooled over a frame window: the numpy model tests/colour_window_ref.py against
``blend_ref.colour_rows`` and against what the feature is for (less flicker, a bridged drop-out); the header against the ctypes
prototypes; the refusals of the three new entry points, which need no device; and every argument check of the new launchers and of
``IRFD.reenact_video(colour_smooth=, colour_sigma=)``, which raise on CPU tensors before anything is launched."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import blend_cases as BC
import blend_ref as B
import colour_window_ref as CW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = dict(max_gain=BC.MAX_GAIN, min_sigma=BC.MIN_SIGMA, min_weight=BC.MIN_WEIGHT)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "holes", "gap"])
def test_model_at_radius_0_is_the_per_frame_model_exactly(name):
    clip = CW.window_clip(name)
    got = CW.window_rows(clip, 0, **PARAMS)
    with np.errstate(invalid="ignore", divide="ignore"):
        want, var_q, var_b = B.colour_rows(clip, ~np.isnan(clip[:, 0]), **PARAMS)    # ``S0 <= min_weight`` lets a NaN S0 through; the kernels' ``>`` does not
    assert np.array_equal(got["rows"], want, equal_nan=True) and np.array_equal(got["var_q"], var_q, equal_nan=True)
    assert np.array_equal(got["P"][got["any"]], clip[got["any"]], equal_nan=True)    # k_0 = 1: the sums themselves
    assert got["terms"].max() == 1
    # the sums of a blend case, as the device hands them over (zeros for an invalid row)
    ref = BC.reference("invalid and zero")
    sums = np.where(ref["valid"][:, None], ref["sums"], 0.0)
    assert np.array_equal(CW.window_rows(sums, 0, **PARAMS)["rows"], ref["rows"])


@pytest.mark.parametrize("radius,sigma", [(1, None), (3, None), (3, 0.8), (64, None)])
def test_model_a_clip_of_equal_frames_gives_the_per_frame_rows(radius, sigma):
    frame = CW.window_clip("plain")[3]
    clip = np.tile(frame, (7, 1))
    got = CW.window_rows(clip, radius, sigma, **PARAMS)
    want, _, _ = B.colour_rows(clip, np.ones(7, dtype=bool), **PARAMS)
    # P = K S with K = sum k_d: K cancels in every quotient up to the roundings of the pooling, 13 per sum at most
    g, o = got["rows"][:, :, 0], got["rows"][:, :, 1]
    assert np.abs(g - want[:, :, 0]).max() <= 64 * np.finfo(float).eps * want[:, :, 0].max()
    amp = (frame[2::4] / frame[0] / np.nanmin(got["var_q"], 0)).max() + (frame[4::4] / frame[0] / np.nanmin(got["var_b"], 0)).max()
    assert np.abs(o - want[:, :, 1]).max() <= 64 * np.finfo(float).eps * 255.0 * amp
    assert got["terms"].tolist() == [min(t, radius) + min(6 - t, radius) + 1 for t in range(7)]


def test_model_flicker_fixture_is_steadier_and_bridges_the_drop_out():
    clip = CW.flicker_clip()
    T, drop = clip.shape[0], 1
    r0, r2 = CW.window_rows(clip, 0, **PARAMS), CW.window_rows(clip, 2, **PARAMS)
    assert r0["rows"][drop].tolist() == [[1.0, 0.0]] * 3 and not r0["any"][drop] and r2["any"].all()
    keep = [t for t in range(T) if t != drop]
    for c in range(3):
        o0, o2 = r0["rows"][keep, c, 1], r2["rows"][:, c, 1]
        step0, step2 = np.abs(np.diff(o0)).max(), np.abs(np.diff(o2)).max()
        assert step2 < step0 and np.ptp(o2) < np.ptp(o0), (c, step0, step2)  # frame to frame, and over the clip
        assert np.ptp(o0) > 20.0                                             # +-12 levels of background: the per-frame rows follow it
        for k in (0, 1):                                                    # the drop-out's row lies between its neighbours'
            lo, hi = sorted((r2["rows"][drop - 1, c, k], r2["rows"][drop + 1, c, k]))
            assert lo <= r2["rows"][drop, c, k] <= hi, (c, k)


def test_model_participation_rules():
    holes, gap = CW.window_clip("holes"), CW.window_clip("gap")
    r = CW.window_rows(holes, 1, **PARAMS)
    assert r["terms"].tolist() == [2, 2, 1, 1, 1, 3, 1]                     # 5 is served (itself, 4 and 6); 4 and 6 do not see 5
    assert np.isnan(r["P"][5, 1]) and np.isfinite(r["P"][[4, 6]]).all()     # the NaN of frame 5 stays in frame 5
    assert r["any"].all()
    r = CW.window_rows(gap, 2, **PARAMS)
    assert r["any"].tolist() == [True, True, True, False, True, True, True]
    assert r["rows"][3].tolist() == [[1.0, 0.0]] * 3
    assert CW.window_rows(gap, 1, **PARAMS)["any"].tolist() == [True, True, False, False, False, True, True]
    assert CW.takes_part(holes, 5, 0, 16.0) and not CW.takes_part(holes, 5, 1, 16.0) and not CW.takes_part(holes, 5, -1, 16.0)
    # a sub-range is the slice of the whole
    whole, part = CW.window_rows(holes, 3, 1.1, **PARAMS), CW.window_rows(holes, 3, 1.1, start=2, stop=6, **PARAMS)
    assert np.array_equal(part["rows"], whole["rows"][2:6], equal_nan=True)


# ---- the C interface ------------------------------------------------------------------------------------------------------------------
NEW = ("spk_paste_colour_sums_sim", "spk_paste_colour_sums_nv12_sim", "spk_colour_rows_window")


def test_header_and_ctypes_agree_on_the_new_entries(pkg):
    L = pkg._lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spk.h")).read(), flags=re.S)
    lib = L.lib()
    ctype = {"int": "c_int", "int64_t": "c_long", "float": "c_float", "double": "c_double", "size_t": "c_ulong"}
    for name in NEW:
        decl = re.search(name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert decl, f"{name} is not declared in include/spk.h"
        params = [p.strip() for p in decl.group(1).split(",")]
        assert name in L.exported_symbols() and len(getattr(lib, name).argtypes) == len(params), name
        for p, t in zip(params, getattr(lib, name).argtypes):
            assert t.__name__ == ("c_void_p" if "*" in p else ctype[p.split()[0]]), (name, p, t)
    # the sums take the match's arguments up to matte_frames, then the output, the workspace and the stream
    for match, sums in (("spk_paste_colour_match_sim", NEW[0]), ("spk_paste_colour_match_nv12_sim", NEW[1])):
        old, new = getattr(lib, match).argtypes, getattr(lib, sums).argtypes
        assert list(new) == list(old[:-7]) + list(old[-4:]) and len(new) == len(old) - 3


def test_entry_refusals_need_no_device(pkg):
    """Every refusal of the three entry points happens before a launch: -1 and a message, on a machine without a GPU."""
    lib = pkg._lib.lib()
    p = 4096
    nan, inf = float("nan"), float("inf")
    per = lib.spk_paste_colour_match_workspace_bytes(1)

    def rgb(src=p, dst=p, sim=p, N=1, Hs=4, Ws=4, H=8, W=8, row=24, img=192, feather=0.0, lo=-1.0, k=127.5, matte=None, mf=0, out=p, ws=p, wsb=None):
        wsb = lib.spk_paste_colour_match_workspace_bytes(max(N, 1)) if wsb is None else wsb
        return lib.spk_paste_colour_sums_sim(src, N, Hs, Ws, dst, img, row, H, W, sim, 0, feather, lo, k, matte, mf, out, ws, wsb, None)

    def nv12(src=p, y=p, uv=p, sim=p, N=1, Hs=4, Ws=4, H=8, W=8, y_row=8, y_img=64, uv_row=8, uv_img=32, std=601, full=0, feather=0.0, lo=-1.0,
             k=127.5, matte=None, mf=0, out=p, ws=p, wsb=None):
        wsb = lib.spk_paste_colour_match_workspace_bytes(max(N, 1)) if wsb is None else wsb
        return lib.spk_paste_colour_sums_nv12_sim(src, N, Hs, Ws, y, y_img, y_row, uv, uv_img, uv_row, H, W, sim, std, full, feather, lo, k, matte,
                                                  mf, out, ws, wsb, None)

    shared = (dict(src=None), dict(sim=None), dict(N=0), dict(Hs=0), dict(Ws=0), dict(H=0), dict(W=0), dict(feather=-0.5), dict(feather=nan),
              dict(k=0.0), dict(lo=nan), dict(matte=p, mf=0), dict(matte=p, mf=2), dict(mf=1),
              dict(out=None), dict(out=p + 4), dict(ws=None), dict(ws=p + 4), dict(wsb=per - 1), dict(wsb=0), dict(N=2, wsb=per))
    for f in (rgb, nv12):
        for bad in shared:
            assert f(**bad) == -1, (f.__name__, bad)
            assert lib.spk_last_error(), bad
        assert f(out=None) == -1 and b"sums" in lib.spk_last_error()
        assert f(wsb=8) == -1 and b"workspace" in lib.spk_last_error()
    for bad in (dict(dst=None), dict(row=23), dict(N=2, img=0), dict(N=2, img=7 * 24 + 23)):
        assert rgb(**bad) == -1, bad
    for bad in (dict(y=None), dict(uv=None), dict(H=7), dict(W=6, y_row=5), dict(uv_row=7), dict(std=2020), dict(full=2), dict(uv=p + 1)):
        assert nv12(**bad) == -1, bad

    def window(sums=p, T=7, n0=0, n=7, radius=2, sigma=1.0, gain=2.0, min_sigma=1.0, weight=16.0, out=p):
        return lib.spk_colour_rows_window(sums, T, n0, n, radius, sigma, gain, min_sigma, weight, out, None)

    for bad in (dict(sums=None), dict(out=None), dict(sums=p + 4), dict(T=0), dict(T=-1), dict(n=0), dict(n0=-1), dict(n0=1), dict(n=8),
                dict(n0=0x7fffffff, n=1), dict(n0=1, n=0x7fffffff), dict(T=0x7fffffff, n0=0x7fffffff), dict(radius=-1), dict(radius=65),
                dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf), dict(gain=0.99), dict(gain=nan), dict(gain=inf),
                dict(min_sigma=-1.0), dict(min_sigma=nan), dict(min_sigma=inf), dict(weight=-1.0), dict(weight=nan), dict(weight=inf)):
        assert window(**bad) == -1, bad
        assert lib.spk_last_error(), bad
    assert window(radius=65) == -1 and b"radius" in lib.spk_last_error()
    assert window(n0=3, n=5) == -1 and b"range" in lib.spk_last_error()
    assert window(gain=0.5) == -1 and b"max_gain" in lib.spk_last_error()


# ---- the launchers and reenact_video: what is refused before a device is touched, without the library ----------------------------------
@pytest.fixture(scope="module")
def bare():
    """The package as imported, and a guard: no entry point may be reached by a call that is refused"""
    return importlib.import_module("speak-hack_amd")


@pytest.fixture
def no_library(bare, monkeypatch):
    def lib():
        raise AssertionError("a refused call reached the library")
    monkeypatch.setattr(bare._lib, "lib", lib)
    return bare


def test_sums_launchers_refuse_what_the_match_launchers_refuse(no_library):
    ops, SpkError = no_library.ops, no_library._lib.SpkError
    x, u8 = torch.zeros(2, 3, 4, 6), torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    surf = torch.zeros(2, 12, 8, dtype=torch.uint8)
    good = [[1, 0, 0, 0], [0.5, 0.5, 1, 2]]
    for f, frames in ((ops.paste_colour_sums, u8), (ops.paste_colour_sums_nv12, surf)):
        for bad in (torch.zeros(4), torch.zeros(6, 4), torch.zeros(3, 4, 6), torch.zeros(4, 6, dtype=torch.float64), [[0.0] * 6] * 4):
            with pytest.raises(ValueError, match="matte"):
                f(x, frames, good, matte=bad)
        with pytest.raises(ValueError, match="feather"):
            f(x, frames, good, feather=-1)
        with pytest.raises(ValueError):
            f(x, frames, good, value_range=(1, 1))
        with pytest.raises(ValueError, match="sim"):
            f(x, frames, [[1, 0, 0, 0], [float("nan"), 0, 0, 0]])
        with pytest.raises(ValueError):
            f(x, frames[:1], good)
        with pytest.raises(TypeError):                                      # the row formula's parameters are not theirs
            f(x, frames, good, max_gain=2.0)
        with pytest.raises(SpkError, match="HIP|device|CPU"):               # well-formed: there is no CPU path
            f(x, frames, good, matte=torch.zeros(2, 4, 6), out=torch.zeros(2, 13, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.paste_colour_sums(x, u8, good, channel_order="gbr")
    with pytest.raises(ValueError):
        ops.paste_colour_sums_nv12(x, surf, good, standard="bt2020")


def test_colour_rows_from_sums_refuses_before_any_device_use(no_library):
    ops, SpkError = no_library.ops, no_library._lib.SpkError
    sums = torch.zeros(7, 13, dtype=torch.float64)
    for bad in (-1, 65, 1.0, True, None, "2"):
        with pytest.raises(ValueError, match="radius"):
            ops.colour_rows_from_sums(sums, bad)
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            ops.colour_rows_from_sums(sums, 2, bad)
    for kw in (dict(max_gain=0.5), dict(max_gain=float("nan")), dict(max_gain=float("inf")), dict(min_sigma=-1), dict(min_sigma=float("nan")),
               dict(min_weight=-0.5), dict(min_weight=float("inf"))):
        with pytest.raises(ValueError, match="max_gain|min_sigma"):
            ops.colour_rows_from_sums(sums, 2, **kw)
    for bad in (torch.zeros(7, 13), torch.zeros(7, 12, dtype=torch.float64), torch.zeros(13, dtype=torch.float64),
                torch.zeros(0, 13, dtype=torch.float64), torch.zeros(1, 7, 13, dtype=torch.float64), [[0.0] * 13] * 7):
        with pytest.raises(ValueError, match="sums"):
            ops.colour_rows_from_sums(bad, 2)
    for kw in (dict(start=-1), dict(start=7), dict(stop=8), dict(stop=0), dict(start=3, stop=3), dict(start=4, stop=2), dict(start=1.0),
               dict(stop=True)):
        with pytest.raises(ValueError, match="start"):
            ops.colour_rows_from_sums(sums, 2, **kw)
    with pytest.raises(SpkError, match="HIP|device|CPU"):                   # well-formed: there is no CPU path
        ops.colour_rows_from_sums(sums, 2, 1.5, start=1, stop=5)


def test_reenact_video_colour_smooth_argument_errors(no_library):
    import model
    m = model.IRFD()
    ident, video = torch.zeros(48, 64, 3, dtype=torch.uint8), torch.zeros(3, 48, 64, 3, dtype=torch.uint8)
    good = [[0.25, 0, 3, 4]] * 3
    kw = dict(align=good, paste=True)
    for smooth in (dict(colour_smooth=2), dict(colour_sigma=1.0), dict(colour_smooth=2, colour_sigma=1.0), dict(colour_smooth=-1)):
        with pytest.raises(ValueError, match="colour_match"):               # without colour_match
            m.reenact_video(ident, video, **kw, **smooth)
        with pytest.raises(ValueError, match="colour_match"):
            m.reenact_video(ident, video, matte=torch.ones(256, 256), **kw, **smooth)
    for bad in (-1, 65, 2.0, True, "2", None):
        with pytest.raises(ValueError, match="colour_smooth"):
            m.reenact_video(ident, video, colour_match=True, colour_smooth=bad, **kw)
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            m.reenact_video(ident, video, colour_match=True, colour_smooth=2, colour_sigma=bad, **kw)
    with pytest.raises(ValueError, match="align"):                          # what colour_match itself needs still comes first or next
        m.reenact_video(ident, video, paste=True, colour_match=True, colour_smooth=2)
    with pytest.raises(ValueError, match="paste"):
        m.reenact_video(ident, video, align=good, colour_match=True, colour_smooth=2)
    with pytest.raises(ValueError, match="align|nv12"):                     # NV12 stays refused with align=
        m.reenact_video(ident, torch.zeros(3, 72, 64, dtype=torch.uint8), pixel_format="nv12", colour_match=True, colour_smooth=2, **kw)
