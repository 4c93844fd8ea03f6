"""CPU-side checks of the seamless paste-back (csrc/frame_blend.hip): ``ops.ellipse_matte`` against its closed form, the fp64
model tests/blend_ref.py against what it must reduce to, the three entry points on both sides of the C boundary with their
refusals (all before a launch, so without a device), every ``ValueError`` of the launchers and of ``IRFD.reenact_video(matte=,
colour_match=)`` that is raised before a device is touched, and -- for every case tests/test_blend_gpu.py runs -- what that test
relies on: no pixel centre within 1e-6 of a region's edge, and weighted channel variances of at least 100 levels^2, so that no
case needs a pixel or a channel left out."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import blend_cases as BC
import blend_ref as B
import sim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")


# ---- ellipse_matte -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,centre,radii,softness", [((16, 16), (0.5, 0.5), (0.36, 0.46), 0.1), ((12, 20), (0.45, 0.55), (0.3, 0.4), 0.25),
                                                        ((33, 17), (0.5, 0.5), (0.36, 0.46), 1.0)])
def test_ellipse_matte_against_its_closed_form(pkg, size, centre, radii, softness):
    m = pkg.ops.ellipse_matte(size, centre, radii, softness)
    Hs, Ws = size
    assert m.dtype == torch.float32 and tuple(m.shape) == size and not m.is_cuda
    for j in range(Hs):
        for i in range(Ws):
            rho = math.sqrt(((i + 0.5) / Ws - centre[0]) ** 2 / radii[0] ** 2 + ((j + 0.5) / Hs - centre[1]) ** 2 / radii[1] ** 2)
            want = min(max((1.0 - rho) / softness, 0.0), 1.0)
            assert abs(float(m[j, i]) - want) <= 1e-7, (j, i)             # fp64 on the host, one rounding to fp32
    assert all(float(m[j, i]) == 0.0 for j in (0, Hs - 1) for i in (0, Ws - 1))          # exact 0 at the corners


def test_ellipse_matte_defaults_and_refusals(pkg):
    ops = pkg.ops
    m = ops.ellipse_matte((17, 17))
    assert float(m[8, 8]) == 1.0 and float(m[0, 0]) == 0.0 and float(m[16, 16]) == 0.0      # exact 1 at the centre
    assert torch.equal(ops.ellipse_matte(17), m) and 0.0 < float(m[8, 13]) <= 1.0 and float(m.min()) == 0.0
    for softness in (0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="softness"):
            ops.ellipse_matte((16, 16), softness=softness)
    with pytest.raises(ValueError):
        ops.ellipse_matte((16, 0))
    with pytest.raises(ValueError, match="radii"):
        ops.ellipse_matte((16, 16), radii=(0.0, 0.4))


# ---- the model against what it reduces to ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feather,bgr", [(0.0, False), (2.5, True)])
def test_model_without_matte_and_colour_is_sim_ref(feather, bgr):
    x, bg = BC.source(1, 4, 16, 16).numpy(), BC.frames(2, 4, BC.H, BC.W, 3).numpy()
    rows = BC.rows_for((0, 1, 2, 3), (16, 16)).numpy()
    rows[3, 1] = np.nan
    z, region, margin = R.paste_out(x, bg, rows, feather=feather, swap_rb=bgr)
    got = B.blend(x, bg, rows, feather=feather, swap_rb=bgr)
    assert np.array_equal(got["z"], z) and np.array_equal(got["region"], region) and got["margin"] == margin
    assert got["valid"].tolist() == [True, True, True, False] and (got["sums"][3] == 0).all()
    assert np.array_equal(got["Mt"], region.astype(np.float64))
    # the identity rows change nothing
    same = B.blend(x, bg, rows, feather=feather, swap_rb=bgr, colour=np.tile([1.0, 0.0], (4, 3, 1)))
    assert np.array_equal(same["z"], z)


def test_model_a_zero_matte_leaves_the_background():
    x, bg = BC.source(3, 3, 12, 20).numpy(), BC.frames(4, 3, BC.H, BC.W, 3).numpy()
    rows = BC.rows_for((0, 1, 2), (12, 20)).numpy()
    matte = BC.matte_for(5, 3, 12, 20).numpy()
    matte[1] = 0.0
    got = B.blend(x, bg, rows, feather=2.5, matte=matte)
    assert got["region"][1].any() and np.array_equal(got["z"][1], bg[1].astype(np.float64)) and got["sums"][1, 0] == 0.0
    assert not np.array_equal(got["z"][0], bg[0]) and (got["Mt"] >= 0).all() and (got["Mt"] <= 1).all()
    assert ((got["Mt"][0] == 0) & got["region"][0]).any()                 # the patch of exact zeros is seen as exact zeros
    rows_, _, _ = B.colour_rows(got["sums"], got["valid"])
    assert rows_[1].tolist() == [[1.0, 0.0]] * 3


def test_model_rows_by_hand_on_a_constant_image():
    """A constant generated image and the whole region weighted 1: q is one level, so the pasted value is g q + o by hand; and
    rows computed from sums written by hand reproduce the definition."""
    N, net = 1, (16, 16)
    x = np.broadcast_to(np.array([0.2, -0.3, 0.5], dtype=np.float32).reshape(1, 3, 1, 1), (N, 3, *net)).copy()
    bg = BC.frames(6, N, BC.H, BC.W, 3).numpy()
    rows = np.array([[1.0, 0.0, 7.0, 5.0]])                               # a box at an integer origin: every weight is exactly 1
    colour = np.array([[[1.5, -20.0], [0.75, 30.0], [float("nan"), 5.0]]])
    got = B.blend(x, bg, rows, colour=colour)
    q = (x[0, :, 0, 0].astype(np.float64) + 1.0) * 127.5
    want = [1.5 * q[0] - 20.0, 0.75 * q[1] + 30.0, q[2]]                  # a NaN gain: (1, 0) for that channel only
    inside = got["region"][0]
    for c in range(3):
        assert np.abs(got["z"][0][inside][:, c] - want[c]).max() <= 1e-10
    # S0 = 10, q of mean 100 and variance 25, b of mean 50 and variance 100: g = 2, o = 50 - 2 * 100
    sums = np.zeros((1, 13))
    sums[0, 0] = 10.0
    for c in range(3):
        sums[0, 1 + 4 * c:5 + 4 * c] = [1000.0, 10.0 * (25.0 + 100.0 ** 2), 500.0, 10.0 * (100.0 + 50.0 ** 2)]
    r, vq, vb = B.colour_rows(sums, np.array([True]), max_gain=4.0, min_sigma=1.0, min_weight=5.0)
    assert np.allclose(r[0], [[2.0, -150.0]] * 3, rtol=0, atol=1e-9) and np.allclose(vq, 25.0) and np.allclose(vb, 100.0)
    assert B.colour_rows(sums, np.array([True]), 1.5, 1.0, 5.0)[0][0, 0].tolist() == [1.5, 50.0 - 1.5 * 100.0]       # the gain is capped
    assert B.colour_rows(sums, np.array([True]), 4.0, 5.0, 5.0)[0][0, 0].tolist() == [1.0, -50.0]                    # var_q <= min_sigma^2
    assert B.colour_rows(sums, np.array([True]), 4.0, 1.0, 10.0)[0][0].tolist() == [[1.0, 0.0]] * 3                  # S0 <= min_weight
    assert B.colour_rows(sums, np.array([False]), 4.0, 1.0, 5.0)[0][0].tolist() == [[1.0, 0.0]] * 3                  # an invalid row


# ---- what the GPU cases rely on ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BC.SPECS))
def test_gpu_cases_keep_their_margins_and_variances(name):
    c, ref = BC.case(name), BC.reference(name)
    assert ref["margin"] >= BC.MARGIN, f"{name}: a pixel centre lies {ref['margin']:.2e} from a region edge"
    N = c["x"].size(0)
    assert 3 <= N <= 4 and tuple(c["bg"].shape) == (N, BC.H, BC.W, 3)
    for n in range(N if name in BC.COLOUR_CASES else 0):                  # the cases whose rows are compared
        S0 = ref["sums"][n, 0]
        if n in c["by_rule"]:
            assert ref["rows"][n].tolist() == [[1.0, 0.0]] * 3 and (S0 == 0.0 or not ref["valid"][n])
            continue
        assert ref["valid"][n] and S0 >= 2 * BC.MIN_WEIGHT, f"{name}: frame {n} has S0 = {S0:.2f}"       # far from the threshold
        assert (ref["var_b"][n] >= 100.0).all(), (name, n, ref["var_b"][n])
        if c["kind"] == "constant":                                       # the rule var_q <= min_sigma^2 decides: g = 1 exactly
            assert (ref["var_q"][n] <= 1e-6).all() and (ref["rows"][n, :, 0] == 1.0).all()
            continue
        assert (ref["var_q"][n] >= 100.0).all(), (name, n, ref["var_q"][n])
        ratio = np.sqrt(ref["var_b"][n] / ref["var_q"][n])
        if c["kind"] == "tenth":                                          # the cap decides, and from far away
            assert (ratio >= 1.5 * BC.MAX_GAIN).all() and (ref["rows"][n, :, 0] == BC.MAX_GAIN).all()
        # a ratio within rounding of an end of [1 / max_gain, max_gain] could be capped by one side and not by the other
        assert (np.abs(ratio / BC.MAX_GAIN - 1.0) > 0.01).all() and (np.abs(ratio * BC.MAX_GAIN - 1.0) > 0.01).all(), (name, n, ratio)
        assert (np.abs(ref["rows"][n, :, 1]) < 256.0).all()
    if c["matte"] is not None and name in BC.MATTE_CASES:
        zero = (ref["Mt"] == 0) & ref["region"]
        assert zero.any() and ((ref["Mt"] > 0) & (ref["Mt"] < 1)).any()


# ---- the C boundary ----------------------------------------------------------------------------------------------------------------
NEW = ("spk_frames_paste_u8_sim_blend", "spk_paste_colour_match_workspace_bytes", "spk_paste_colour_match_sim")


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
        for p, t in zip(params, getattr(lib, name).argtypes):         # pointers travel as void*, scalars by their C type
            assert t.__name__ == ("c_void_p" if "*" in p else ctype[p.split()[0]]), (name, p, t)
    # the blend takes the paste's arguments, then three more and the stream
    old, new = lib.spk_frames_paste_u8_sim.argtypes, lib.spk_frames_paste_u8_sim_blend.argtypes
    assert list(new[:len(old) - 1]) == list(old[:-1]) and len(new) == len(old) + 3


def test_entry_refusals_need_no_device(pkg):
    """Every refusal of the three entry points happens before a launch: -1 and a message, on a machine without a GPU."""
    lib = pkg._lib.lib()
    p = 4096                     # any non-null, aligned address: the arguments are refused before anything is read or launched
    nan, inf = float("nan"), float("inf")
    assert lib.spk_paste_colour_match_workspace_bytes(0) == -1 and lib.spk_paste_colour_match_workspace_bytes(-3) == -1
    per = lib.spk_paste_colour_match_workspace_bytes(1)
    assert per > 0 and per % (13 * 8) == 0 and lib.spk_paste_colour_match_workspace_bytes(5) == 5 * per

    def blend(src=p, dst=p, sim=p, N=1, Hs=4, Ws=4, H=8, W=8, row=24, img=192, feather=0.0, lo=-1.0, k=127.5, matte=None, mf=0, colour=None):
        return lib.spk_frames_paste_u8_sim_blend(src, N, Hs, Ws, dst, img, row, H, W, sim, 0, feather, lo, k, matte, mf, colour, None)

    def match(src=p, dst=p, sim=p, N=1, Hs=4, Ws=4, H=8, W=8, row=24, img=192, feather=0.0, lo=-1.0, k=127.5, matte=None, mf=0, gain=2.0,
              sigma=1.0, weight=16.0, out=p, ws=p, wsb=None):
        wsb = lib.spk_paste_colour_match_workspace_bytes(max(N, 1)) if wsb is None else wsb
        return lib.spk_paste_colour_match_sim(src, N, Hs, Ws, dst, img, row, H, W, sim, 0, feather, lo, k, matte, mf, gain, sigma, weight, out,
                                              ws, wsb, None)

    shared = (dict(src=None), dict(dst=None), dict(sim=None), dict(N=0), dict(Hs=0), dict(Ws=0), dict(H=0), dict(W=0), dict(row=23),
              dict(N=2, img=7 * 24 + 23), dict(N=2, img=0), dict(N=2, img=-192), dict(feather=-0.5), dict(feather=nan), dict(feather=inf),
              dict(k=0.0), dict(lo=nan), dict(k=inf), dict(W=0x7fffffff),
              dict(matte=p, mf=0), dict(matte=p, mf=2), dict(matte=p, mf=-1), dict(N=3, img=192, matte=p, mf=2), dict(mf=1), dict(N=2, img=192, mf=2))
    for f in (blend, match):
        for bad in shared:
            assert f(**bad) == -1, (f.__name__, bad)
            assert lib.spk_last_error(), bad
        assert f(matte=p, mf=3) == -1 and b"matte_frames" in lib.spk_last_error()
        assert f(N=2, img=0) == -1 and b"overlap" in lib.spk_last_error()
        assert f(sim=None) == -1 and b"transform" in lib.spk_last_error()
    for bad in (dict(gain=0.99), dict(gain=nan), dict(gain=inf), dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf), dict(weight=-1.0),
                dict(weight=nan), dict(weight=inf), dict(out=None), dict(ws=None), dict(wsb=per - 1), dict(wsb=0), dict(N=2, wsb=per),
                dict(ws=p + 4)):
        assert match(**bad) == -1, bad
        assert lib.spk_last_error(), bad
    assert match(gain=0.5) == -1 and b"max_gain" in lib.spk_last_error()
    assert match(wsb=8) == -1 and b"workspace" in lib.spk_last_error()


# ---- the launchers and reenact_video: what is refused before a device is touched -----------------------------------------------------
def test_launchers_refuse_bad_mattes_and_rows_before_any_device_use(pkg):
    ops, SpkError = pkg.ops, pkg._lib.SpkError
    x, u8 = torch.zeros(2, 3, 4, 6), torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    good = [[1, 0, 0, 0], [0.5, 0.5, 1, 2]]
    bad_mattes = [torch.zeros(4), torch.zeros(1, 2, 4, 6),                  # rank
                  torch.zeros(6, 4), torch.zeros(4, 5), torch.zeros(3, 4, 6), torch.zeros(1, 4, 6),    # size, frames
                  torch.zeros(4, 6, dtype=torch.float64), torch.zeros(2, 4, 6, dtype=torch.uint8), [[0.0] * 6] * 4]     # dtype, not a tensor
    for bad in bad_mattes:
        with pytest.raises(ValueError, match="matte"):
            ops.frames_paste_u8_aligned(x, u8, good, matte=bad)
        with pytest.raises(ValueError, match="matte"):
            ops.paste_colour_match(x, u8, good, matte=bad)
    for bad in (torch.zeros(2, 3), torch.zeros(2, 2, 3), torch.zeros(3, 3, 2), torch.zeros(2, 3, 2, dtype=torch.float64), [[1.0, 0.0]] * 3):
        with pytest.raises(ValueError, match="colour"):
            ops.frames_paste_u8_aligned(x, u8, good, colour=bad)
    for kw in (dict(max_gain=0.5), dict(max_gain=float("nan")), dict(max_gain=float("inf")), dict(min_sigma=-1), dict(min_sigma=float("nan")),
               dict(min_weight=-0.5), dict(min_weight=float("inf"))):
        with pytest.raises(ValueError, match="max_gain|min_sigma"):
            ops.paste_colour_match(x, u8, good, **kw)
    # the checks of the plain launcher hold for both, in front of the device
    for f in (lambda **kw: ops.frames_paste_u8_aligned(x, u8, good, matte=torch.zeros(4, 6), **kw), lambda **kw: ops.paste_colour_match(x, u8, good, **kw)):
        with pytest.raises(ValueError, match="feather"):
            f(feather=-1)
        with pytest.raises(ValueError):
            f(value_range=(1, 1))
        with pytest.raises(ValueError):
            f(channel_order="gbr")
    with pytest.raises(ValueError, match="sim"):
        ops.paste_colour_match(x, u8, [[1, 0, 0, 0], [float("nan"), 0, 0, 0]])
    with pytest.raises(ValueError):
        ops.paste_colour_match(x, u8[:1], good)
    # well-formed arguments: there is no CPU path
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_paste_u8_aligned(x, u8, good, matte=torch.zeros(4, 6), colour=torch.zeros(2, 3, 2))
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.paste_colour_match(x, u8, good, matte=torch.zeros(2, 4, 6))


def test_reenact_video_blend_argument_errors(pkg):
    import model
    m = model.IRFD()
    ident, video = torch.zeros(48, 64, 3, dtype=torch.uint8), torch.zeros(3, 48, 64, 3, dtype=torch.uint8)
    surf = torch.zeros(3, 72, 64, dtype=torch.uint8)
    good, matte = [[0.25, 0, 3, 4]] * 3, torch.ones(256, 256)
    for blend in (dict(matte=matte), dict(colour_match=True), dict(matte=matte, colour_match=True)):
        with pytest.raises(ValueError, match="align"):                      # without align
            m.reenact_video(ident, video, paste=True, **blend)
        with pytest.raises(ValueError, match="align"):
            m.reenact_video(ident, video, crop=(3, 5, 40, 44), paste=True, **blend)
        with pytest.raises(ValueError, match="paste"):                      # without paste
            m.reenact_video(ident, video, align=good, **blend)
        with pytest.raises(ValueError, match="align|nv12"):                 # NV12 frames take crop boxes
            m.reenact_video(ident, surf, align=good, paste=True, pixel_format="nv12", **blend)
        with pytest.raises(ValueError, match="align"):
            m.reenact_video(ident, surf, crop=(2, 4, 40, 44), paste=True, pixel_format="nv12", **blend)
    for bad in (torch.ones(256), torch.ones(1, 3, 256, 256), torch.ones(256, 256, dtype=torch.float64), torch.ones(2, 256, 256),
                torch.ones(4, 256, 256), [[1.0]]):
        with pytest.raises(ValueError, match="matte"):
            m.reenact_video(ident, video, align=good, paste=True, matte=bad)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="colour_match"):
            m.reenact_video(ident, video, align=good, paste=True, colour_match=bad)
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):          # well-formed: there is no CPU path
        m.reenact_video(ident, video, align=good, paste=True, matte=matte, colour_match=True)
