"""CPU-side checks of the landmark matte (``spk_matte_from_landmarks``): the fp64 model tests/matte_ref.py against a plain loop,
against an analytic ramp and against even-odd parity at hand-picked pixels; what the cases of the GPU tests hold, counted here with
the model alone; the refusals of the entry point (all before a launch, so without a device); and every error of
``ops.matte_from_landmarks`` / ``ops.LandmarkMatte`` / ``IRFD.reenact_video(matte=)`` that is raised before a device is touched."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import landmark_ref as LR
import matte_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPLATE5 = [(44.0, 52.0), (84.0, 52.0), (64.0, 74.0), (48.0, 96.0), (80.0, 96.0)]
IDENTITY = np.array([[1.0, 0.0, 0.0, 0.0]], dtype=np.float32)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")


# ---- the model --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.CASES))
def test_vectorised_model_is_the_plain_loop(name):
    """Per pixel and per edge, as the definition reads: the same numbers (the two differ in nothing but numpy's broadcasting)."""
    c = M.case(name)
    kw = dict(grow=c["grow"], radius=c["radius"])
    fast = M.matte64(c["pts"], c["sim"], c["size"], c["contour"], c["softness"], **kw)[0]
    slow = M.matte64(c["pts"], c["sim"], c["size"], c["contour"], c["softness"], distance=M.signed_distance_loop, **kw)[0]
    assert np.abs(fast - slow).max() <= 1e-12


def test_cases_hold_zeros_ones_and_a_ramp():
    """What tests/test_landmark_matte_gpu.py asserts of its cases, counted with the model alone: per frame, pixels that must be
    exactly 0, pixels that must be exactly 1, and pixels on the ramp."""
    cases = [M.case(name) for name in M.CASES] + [M.big_case()]
    for c in cases:
        dg = M.matte64(c["pts"], c["sim"], c["size"], c["contour"], c["softness"], grow=c["grow"], radius=c["radius"])[0]
        for n in range(len(dg)):
            zero, one, between = M.counts(dg[n], c["softness"])
            assert zero >= M.POPULATED[0] and one >= M.POPULATED[1] and between >= M.POPULATED[2], (c["size"], c["contour"], n, zero, one, between)
    on = M.case("star on pixel centres 16x16")
    p, part = M.mapped(on["pts"], on["sim"], on["contour"])
    assert part.all() and np.array_equal(p, on["generated"]) and np.array_equal(p % 1.0, np.full(p.shape, 0.5))   # to the bit
    dg = M.matte64(on["pts"], on["sim"], on["size"], on["contour"], on["softness"])[0]
    assert all((dg[n] == 0).sum() >= 12 for n in range(M.N))              # every vertex, and more, exactly on the outline


def test_square_outline_is_the_analytic_ramp():
    """An axis-aligned square [3, 13] x [2, 11]: clamp(min(distance to the four sides) / softness, 0, 1) inside, 0 outside."""
    corners = np.array([[(3, 2), (13, 2), (13, 11), (3, 11)]], dtype=np.float32)
    for softness in (1.0, 2.5, 7.0):
        got = M.matte(corners, IDENTITY, (14, 16), [0, 1, 2, 3], softness)
        x, y = M.centres(14, 16)
        inside = (x > 3) & (x < 13) & (y > 2) & (y < 11)
        want = np.where(inside, np.clip(np.minimum(np.minimum(x - 3, 13 - x), np.minimum(y - 2, 11 - y)) / softness, 0, 1), 0.0)
        assert got.shape == (1, 14, 16) and got.dtype == np.float32 and np.array_equal(got[0], want.astype(np.float32))
        assert inside.sum() == 90 and (got[0] > 0).sum() == 90
    # grown by 1.5: the ramp starts 1.5 pixels outside, where the distance to the square is a distance to a side or to a corner
    got = M.matte(corners, IDENTITY, (14, 16), [0, 1, 2, 3], 2.0, grow=1.5)
    assert got[0, 0, 0] == 0.0 and got[0, 1, 2] == np.float32((1.5 - np.hypot(0.5, 0.5)) / 2.0) and got[0, 5, 1] == np.float32(0.0)
    assert got[0, 5, 2] == np.float32(0.5) and got[0, 6, 8] == 1.0


def test_bow_tie_and_star_follow_even_odd_parity():
    # a bow-tie: (2,2) -> (14,12) -> (14,2) -> (2,12) crosses itself at (8, 7); its two triangles are inside, above and below are not
    tie = np.array([[(2, 2), (14, 12), (14, 2), (2, 12)]], dtype=np.float32)
    d = M.matte64(tie, IDENTITY, (14, 16), [0, 1, 2, 3], 1.0)[0][0]
    for (j, i), inside in (((6, 3), True), ((6, 12), True), ((7, 4), True), ((2, 7), False), ((11, 8), False), ((6, 0), False),
                           ((6, 15), False), ((3, 8), False)):
        assert (d[j, i] > 0) == inside, (j, i, d[j, i])
    # a pentagram drawn in one stroke: the five points are inside, the central pentagon is crossed twice and is OUTSIDE
    th = np.pi / 2 + 4 * np.pi * np.arange(5) / 5
    star = np.stack([16 + 14 * np.cos(th), 16 - 14 * np.sin(th)], axis=1)[None].astype(np.float32)
    d = M.matte64(star, IDENTITY, (32, 32), [0, 1, 2, 3, 4], 1.0)[0][0]
    assert d[15, 15] < 0 and d[16, 16] < 0 and d[13, 16] < 0              # the pentagon in the middle
    assert d[5, 15] > 0 and d[6, 16] > 0                                  # the top point
    assert d[12, 6] > 0 and d[12, 25] > 0 and d[24, 9] > 0 and d[24, 22] > 0      # the other four
    assert d[0, 0] < 0 and d[28, 16] < 0 and d[16, 2] < 0
    # the same five points in convex order are a pentagon: the middle is inside
    d = M.matte64(star, IDENTITY, (32, 32), [0, 3, 1, 4, 2], 1.0)[0][0]
    assert d[15, 15] > 0 and d[13, 16] > 0 and d[0, 0] < 0


def test_window_fallback_and_holes_in_the_model():
    c = M.case("crossed 12x20 grown smoothed")
    p, part = M.mapped(c["pts"], c["sim"], c["contour"])
    assert part.all()
    P0, hole = M.outline(c["pts"], c["sim"], c["contour"], radius=0)
    assert np.array_equal(P0, p) and not hole.any()                       # radius = 0: the frame's own points, to the bit
    P2, _ = M.outline(c["pts"], c["sim"], c["contour"], radius=2, sigma=1.0)
    g = np.exp(-np.arange(-2, 3) ** 2 / 2.0)
    assert np.abs(P2[2] - (g[:, None, None] * p).sum(axis=0) / g.sum()).max() <= 1e-12 and np.abs(P2 - p).max() > 1e-3
    # a frame of NaN landmarks is bridged; an invalid row takes its frame out of its neighbours' windows
    pts, sim = c["pts"].copy(), c["sim"].copy()
    pts[2], sim[0] = np.nan, [0.01, 0.0, 5.0, 5.0]
    P, hole = M.outline(pts, sim, c["contour"], radius=1, sigma=1.0)
    assert not hole.any() and np.abs(P[2] - (p[1] + p[3]) / 2).max() <= 1e-12 and np.array_equal(P[0], p[1])
    g1 = np.exp(-0.5)
    assert np.abs(P[1] - p[1]).max() <= 1e-12 and np.abs(P[3] - (p[3] + g1 * p[4]) / (1 + g1)).max() <= 1e-12
    # a window without a point: the fallback's polygon with one, zeros without
    fb = np.array([(3, 2), (13, 2), (13, 9), (8, 5), (8, 5), (3, 9), (2, 5)], dtype=np.float32)
    P, hole = M.outline(pts, sim, c["contour"], radius=0, fallback=fb)
    assert np.array_equal(P[2], fb) and np.array_equal(P[0], fb) and np.array_equal(P[1], p[1]) and not hole.any()
    dg, P, hole = M.matte64(pts, sim, c["size"], c["contour"], 2.0, radius=0)
    assert hole.tolist() == [True, False, True, False, False] and not M.ramp(dg, 2.0)[[0, 2]].any() and M.ramp(dg, 2.0)[1].any()
    pts[1, c["contour"][3]] = np.inf                                      # one point of one frame: that frame alone has a hole
    assert M.outline(pts, sim, c["contour"], radius=0)[1].tolist() == [True, True, True, False, False]


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_new_entry(pkg):
    L = pkg._lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spk.h")).read(), flags=re.S)
    name = "spk_matte_from_landmarks"
    decl = re.search(name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert decl, f"{name} is not declared in include/spk.h"
    params = [p.strip() for p in decl.group(1).split(",")]
    argtypes = getattr(L.lib(), name).argtypes
    assert name in L.exported_symbols() and len(argtypes) == len(params) == 16
    for p, t in zip(params, argtypes):                                    # device pointers travel as void*, scalars by their C type
        want = "LP_c_int" if "int32_t*" in p else "c_void_p" if "*" in p else {"int": "c_int", "double": "c_double"}[p.split()[0]]
        assert t.__name__ == want, (p, t)


def test_entry_refusals_need_no_device(pkg):
    """Every refusal happens before a launch: -1 and a message, on a machine without a GPU."""
    import ctypes
    lib = pkg._lib.lib()
    p = 1 << 20                  # any non-null address: the arguments are refused before anything is read or launched

    def call(pts=p, N=2, K=12, offset=0.0, sim=p, contour=(0, 3, 6, 9), Kc=None, fallback=None, radius=2, sigma=1.0, softness=4.0, grow=0.0,
             matte=p, Hs=16, Ws=16):
        idx = None if contour is None else (ctypes.c_int32 * max(len(contour), 1))(*contour)
        Kc = Kc if Kc is not None else 0 if contour is None else len(contour)
        return lib.spk_matte_from_landmarks(pts, N, K, offset, sim, idx, Kc, fallback, radius, sigma, softness, grow, matte, Hs, Ws, None)

    inf, nan = float("inf"), float("nan")
    for bad in (dict(pts=None), dict(sim=None), dict(contour=None, Kc=4), dict(matte=None), dict(N=0), dict(N=-2), dict(K=0), dict(K=-1),
                dict(K=4097), dict(K=0x7fffffff, contour=(0, 1, -1)), dict(contour=(0, 1)), dict(contour=(0, 1, 2), Kc=2),
                dict(contour=tuple(range(12)) * 11, Kc=129), dict(contour=(0, 1, 2), Kc=0x7fffffff), dict(contour=(0, 1, 2), Kc=-3),
                dict(contour=(0, 3, 12)), dict(contour=(-1, 3, 6)), dict(contour=(0, 3, 6, 0x7fffffff)), dict(Hs=0), dict(Ws=0),
                dict(Hs=4097), dict(Ws=4097), dict(Hs=0x7fffffff), dict(Ws=0x7fffffff), dict(Hs=-16), dict(radius=-1), dict(radius=65),
                dict(radius=0x7fffffff), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf), dict(softness=0.0),
                dict(softness=-2.0), dict(softness=nan), dict(softness=inf), dict(grow=nan), dict(grow=inf), dict(grow=-inf),
                dict(offset=nan), dict(offset=inf), dict(N=0x7fffffff, Hs=4096, Ws=4096, softness=0.0)):
        assert call(**bad) == -1, bad
        assert lib.spk_last_error(), bad
    for bad, word in ((dict(contour=(0, 3, 12)), b"contour[2] = 12"), (dict(contour=(0, 1)), b"Kc must be"), (dict(K=4097), b"K must be"),
                      (dict(Hs=4097), b"Hs and Ws"), (dict(radius=65), b"radius"), (dict(sigma=0.0), b"sigma"),
                      (dict(softness=0.0), b"softness"), (dict(grow=nan), b"grow"), (dict(offset=inf), b"offset"), (dict(matte=None), b"matte")):
        assert call(**bad) == -1 and word in lib.spk_last_error(), (bad, lib.spk_last_error())


# ---- the two Python names and reenact_video: what is refused before a device is touched ----------------------------------------
def test_python_argument_errors(pkg):
    ops, SpkError = pkg.ops, pkg._lib.SpkError
    lm, rows, contour = torch.zeros(3, 12, 2), [[1.0, 0.0, 0.0, 0.0]] * 3, [0, 3, 6, 9]
    f = ops.matte_from_landmarks
    for bad in (torch.zeros(3, 12), torch.zeros(3, 12, 3), torch.zeros(0, 12, 2), torch.zeros(3, 0, 2), [[TEMPLATE5]], None):
        with pytest.raises(ValueError, match="landmarks"):
            f(bad, rows, 16, contour)
        with pytest.raises(ValueError, match="landmarks"):
            ops.LandmarkMatte(contour, landmarks=bad) if bad is not None else f(bad, rows, 16, contour)
    for size in (0, (16, 0), 4097, (4097, 16), -4):
        with pytest.raises(ValueError, match="size"):
            f(lm, rows, size, contour)
    for bad in ([0, 1], list(range(12)) * 11, [0, 3, 12], [0, -1, 5], [0.0, 1.0, 2.0], [[0, 1, 2]], "abc", torch.tensor([True, False, True]), 7):
        with pytest.raises(ValueError, match="contour"):
            f(lm, rows, 16, bad)
        with pytest.raises(ValueError, match="contour"):
            ops.LandmarkMatte(bad, landmarks=lm)
    for name in ("softness", "grow", "offset"):
        for v in (float("nan"), float("inf"), "x") + ((0.0, -1.0) if name == "softness" else ()):
            with pytest.raises(ValueError, match=name):
                f(lm, rows, 16, contour, **{name: v})
            with pytest.raises(ValueError, match=name):
                ops.LandmarkMatte(contour, **{name: v})
    for radius in (-1, 65, 1.5, True):
        with pytest.raises(ValueError, match="radius"):
            f(lm, rows, 16, contour, smooth=radius)
        with pytest.raises(ValueError, match="radius"):
            ops.LandmarkMatte(contour, smooth=radius)
    for sigma in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            f(lm, rows, 16, contour, smooth=2, sigma=sigma)
        with pytest.raises(ValueError, match="sigma"):
            ops.LandmarkMatte(contour, smooth=2, sigma=sigma)
    with pytest.raises(ValueError, match="sigma comes with smooth"):
        ops.LandmarkMatte(contour, sigma=1.0)
    for sim in (rows[:2], [[1.0, 0.0, 0.0]] * 3, [[0.0, 0.0, 1.0, 1.0]] * 3, [[float("nan"), 0, 0, 0]] * 3, [[32.0, 0, 0, 0]] * 3):
        with pytest.raises(ValueError, match="sim"):
            f(lm, sim, 16, contour)
    for fallback in ([(1.0, 2.0)] * 3, [(1.0, 2.0, 3.0)] * 4, [(float("nan"), 2.0)] * 4, "abcd", torch.zeros(4)):
        with pytest.raises(ValueError, match="fallback"):
            f(lm, rows, 16, contour, fallback=fallback)
        with pytest.raises(ValueError, match="fallback"):
            ops.LandmarkMatte(contour, fallback=fallback)
    # the arguments are in order: what is left is the device
    for kw in (dict(), dict(fallback=[(1.0, 2.0)] * 4, smooth=2, sigma=0.7, grow=-1.0, softness=0.5, offset=0.5)):
        with pytest.raises(SpkError, match="HIP|device|CPU"):
            f(lm, rows, (12, 20), contour, **kw)
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        f(lm.double(), torch.tensor(rows), 16, torch.tensor(contour))


def test_landmark_matte_binds_to_its_call(pkg):
    """``LandmarkMatte.bind``: what the carrier takes from ``align=LandmarkAlign(...)``, and what it refuses, all on the host."""
    ops = pkg.ops
    lm5, lm12 = torch.zeros(3, 5, 2), torch.zeros(3, 12, 2)
    la = ops.LandmarkAlign(lm5, TEMPLATE5, offset=0.5, smooth=2, sigma=0.8)
    rows = [[0.25, 0, 3, 4]] * 3
    with pytest.raises(ValueError, match="LandmarkAlign"):                # no landmarks of its own, and none to borrow
        ops.LandmarkMatte([0, 1, 4, 3]).bind(rows, 3)
    with pytest.raises(ValueError, match="LandmarkAlign"):
        ops.LandmarkMatte([0, 1, 4, 3]).bind(None, 3)
    with pytest.raises(ValueError, match="template"):                     # landmarks of its own, but the default fallback is the template
        ops.LandmarkMatte([0, 1, 4, 3], landmarks=lm5).bind(rows, 3)
    with pytest.raises(ValueError, match="contour"):                      # an index the borrowed landmarks do not have
        ops.LandmarkMatte([0, 1, 5]).bind(la, 3)
    with pytest.raises(ValueError, match="template"):                     # own landmarks with more points than the template
        ops.LandmarkMatte([0, 1, 11], landmarks=lm12).bind(la, 3)
    with pytest.raises(ValueError, match="3 frames for 4"):
        ops.LandmarkMatte([0, 1, 4, 3]).bind(la, 4)
    with pytest.raises(ValueError, match="3 frames for 2"):
        ops.LandmarkMatte([0, 1, 4], landmarks=lm12, fallback=None).bind(rows[:2], 2)
    for lmk, kw in ((ops.LandmarkMatte([0, 1, 4, 3]), {}), (ops.LandmarkMatte([0, 1, 11], landmarks=lm12, fallback=None), {}),
                    (ops.LandmarkMatte([0, 1, 4], fallback=[(1.0, 2.0)] * 3, smooth=0, offset=0.0), {})):
        assert callable(lmk.bind(la, 3))
    assert callable(ops.LandmarkMatte([0, 1, 11], landmarks=lm12, fallback=None).bind(rows, 3))


def test_reenact_video_argument_errors(pkg):
    import model
    ops = pkg.ops
    m = model.IRFD()
    ident, video = torch.zeros(48, 64, 3, dtype=torch.uint8), torch.zeros(3, 48, 64, 3, dtype=torch.uint8)
    surf = torch.zeros(3, 72, 64, dtype=torch.uint8)
    good, la = [[0.25, 0, 3, 4]] * 3, ops.LandmarkAlign(torch.zeros(3, 5, 2), TEMPLATE5)
    lmk = ops.LandmarkMatte([0, 1, 4, 3])
    with pytest.raises(ValueError, match="LandmarkAlign"):                 # landmarks=None without a LandmarkAlign
        m.reenact_video(ident, video, align=good, paste=True, matte=lmk)
    with pytest.raises(ValueError, match="2 frames for 3"):
        m.reenact_video(ident, video, align=la, paste=True, matte=ops.LandmarkMatte([0, 1, 4], landmarks=torch.zeros(2, 5, 2)))
    with pytest.raises(ValueError, match="contour"):
        m.reenact_video(ident, video, align=la, paste=True, matte=ops.LandmarkMatte([0, 1, 7]))
    # everything else about matte= stays: it needs align=, paste=True and packed RGB
    for kw in (dict(paste=True), dict(align=la), dict(crop=(0, 0, 48, 64), paste=True)):
        with pytest.raises(ValueError, match="matte / colour_match apply to align= with paste=True only"):
            m.reenact_video(ident, video, matte=lmk, **kw)
    with pytest.raises(ValueError, match="align applies to pixel_format='rgb24' only"):
        m.reenact_video(ident, surf, align=la, paste=True, matte=lmk, pixel_format="nv12")
    for bad in ("template", [[1.0]], torch.zeros(4, 4, dtype=torch.float64)):
        with pytest.raises(ValueError, match="matte must be a float32 tensor"):
            m.reenact_video(ident, video, align=la, paste=True, matte=bad)
    # the arguments are in order: what is left is the device
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        m.reenact_video(ident, video, align=la, paste=True, matte=lmk)


def test_apply_and_mapped_are_inverse():
    """``mapped`` undoes ``landmark_ref.apply`` (the transform of include/spk.h) to the rounding of the fp32 landmarks."""
    c = M.case("star 16x16")
    p, part = M.mapped(c["pts"], c["sim"], c["contour"])
    scale = np.abs(c["pts"]).max(axis=(1, 2))[:, None, None] / np.hypot(c["sim"][:, 0], c["sim"][:, 1])[:, None, None]
    assert part.all() and (np.abs(p - c["generated"]) <= 1.2e-7 * scale + 1e-12).all()
    assert np.abs(LR.apply(c["sim"], [(0.0, 0.0)])[:, 0] - c["sim"][:, 2:]).max() == 0
