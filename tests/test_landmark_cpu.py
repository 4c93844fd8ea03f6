"""CPU-side checks of landmarks -> rows (``spk_sim_fit_landmarks``, ``spk_sim_smooth``): the fp64 model tests/landmark_ref.py
against an independent least-squares solver and against the transforms it must give back, the smoothing model against what its
definition promises, the refusals of the two entry points (all before a launch, so without a device), and every error of
``ops.similarity_from_landmarks`` / ``ops.smooth_similarity_rows`` / ``ops.LandmarkAlign`` / ``IRFD.reenact_video`` that is raised
before a device is touched."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import landmark_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [2, 5, 68, 130]
TEMPLATE5 = [(44.0, 52.0), (84.0, 52.0), (64.0, 74.0), (48.0, 96.0), (80.0, 96.0)]      # eyes, nose, mouth corners in a 128 image


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")


# ---- the fit model ---------------------------------------------------------------------------------------------------------------
def lstsq_fit(w, u, v, x, y):
    """The same minimiser from the 2K x 4 system with rows sqrt(w) [u, -v, 1, 0 | x], sqrt(w) [v, u, 0, 1 | y]"""
    q = np.sqrt(w)
    one, zero = np.ones_like(u), np.zeros_like(u)
    A = np.concatenate([np.stack([u, -v, one, zero], 1) * q[:, None], np.stack([v, u, zero, one], 1) * q[:, None]])
    b = np.concatenate([x * q, y * q])
    return np.linalg.lstsq(A, b, rcond=None)[0]


@pytest.mark.parametrize("K", KS)
def test_fit_model_against_lstsq(K):
    """Scales 0.07 ... 15, any angle, translations -500 ... 4000, 2 pixels of noise, zero / negative / NaN / Inf weights and
    NaN / Inf landmarks among them: every number within 1e-7 of ``np.linalg.lstsq`` on the participants."""
    worst, fitted = 0.0, 0
    for seed in range(8):
        c = R.case(K, N=6, seed=seed)
        for weights, offset in ((None, 0.0), (c["w_bcast"], 0.5), (c["w_frames"], 0.0)):
            got = R.fit64(c["pts"], c["tmpl"], weights, offset)
            for n in range(6):
                w, x, y, mask = R.participants(c["pts"], weights, n, offset)
                if mask.sum() < 2:
                    assert np.isnan(got[n]).all()
                    continue
                tm = c["tmpl"].astype(np.float64)[mask]
                want = lstsq_fit(w[mask], tm[:, 0], tm[:, 1], x[mask], y[mask])
                worst, fitted = max(worst, float(np.abs(got[n] - want).max())), fitted + 1
    print(f"fit model, K = {K}: largest |model - lstsq| over {fitted} frames = {worst:.3e} (bound 1e-7)")
    assert fitted >= (60 if K > 2 else 20) and worst <= 1e-7


def test_fit_model_gives_back_the_rows_it_was_made_from(pkg):
    """Landmarks made by applying ``ops.similarity_rows`` rows to a template, rounded to fp32, come back as those rows to 1e-5
    relative: (a, c) relative to the scale s, (tx, ty) relative to the largest coordinate of the landmarks, the size of the
    numbers the translation is a difference of.  (An fp32 landmark carries 6e-8 of its coordinate, here <= 1.3e-4 pixels; over a
    template 40 wide that is <= 4e-6 of s in (a, c), and <= 1e-3 pixels in (tx, ty) against coordinates of ~2000.)"""
    rows = pkg.ops.similarity_rows([(540.2, 960.7), (300.5, 1500.25), (900.0, 420.0), (77.7, 88.8)], [400.0, 90.0, 777.0, 128.0],
                                   [0.0, 0.4, -2.9, 1.5707], 128).numpy()
    pts = R.apply(rows, TEMPLATE5).astype(np.float32)
    got = R.fit(pts, TEMPLATE5).astype(np.float64)
    s = np.hypot(rows[:, 0], rows[:, 1]).astype(np.float64)
    L = np.abs(pts).max(axis=(1, 2)).astype(np.float64)
    rel = np.abs(got - rows) / np.stack([s, s, L, L], axis=1)
    print(f"round trip: largest relative difference {rel.max():.3e} (bound 1e-5)")
    assert rel.max() <= 1e-5


def test_fit_model_drop_outs_are_nan_rows():
    tmpl = np.array([(50, 60), (50, 60), (50, 60), (120, 130), (200, 90)], dtype=np.float32)
    pts = R.apply([[1.5, 0.2, 30, 40]] * 4, tmpl).astype(np.float32)
    w = np.array([[0, 0, 0, 1, 0], [0, 0, 0, 0, 0], [1, 1, 1, 0, 0], [1, 1, 1, 1, 0]], dtype=np.float32)
    got = R.fit(pts, tmpl, w)
    assert np.isnan(got[:3]).all()                      # one participant; none; participants on one template point (D = 0)
    assert np.allclose(got[3], [1.5, 0.2, 30, 40], atol=1e-4)
    pts[3, :4, 0] = [np.nan, np.inf, -np.inf, 7.0]      # and with landmarks that are not finite: one participant left
    assert np.isnan(R.fit(pts, tmpl, w)[3]).all()
    big = R.apply([[1.0, 0.0, 3e38, 0.0]], tmpl[3:]).astype(np.float32)
    assert np.isnan(R.fit(big, tmpl[3:], None, 3e38)).all()      # a result that does not fit fp32: four NaNs, not an Inf


# ---- the smoothing model ---------------------------------------------------------------------------------------------------------
def some_rows(N, seed=0):
    rng = np.random.default_rng(seed)
    s, th = rng.uniform(0.3, 3.0, N), rng.uniform(-0.5, 0.5, N)
    return np.stack([s * np.cos(th), s * np.sin(th), rng.uniform(0, 900, N), rng.uniform(0, 500, N)], axis=1).astype(np.float32)


def test_smooth_model_constant_rows_gaps_and_copy():
    row = np.array([0.8125, -0.3333, 412.75, 96.1], dtype=np.float32)
    const = np.tile(row, (9, 1))
    const[3] = np.nan                                                      # a drop-out among them: bridged
    got = R.smooth(const, 2, 1.0)
    assert got.dtype == np.float32 and got.tobytes() == np.tile(row, (9, 1)).tobytes()
    rows = some_rows(14)
    rows[4:10] = np.nan                                                    # six frames: longer than 2 * 2 + 1
    got = R.smooth(rows, 2, 1.0)
    assert np.isnan(got[6:8]).all() and not np.isnan(got[:6]).any() and not np.isnan(got[8:]).any()
    rows = some_rows(7, 1)
    rows[2, 3], rows[5], rows[1, 1] = np.nan, np.inf, -0.0
    got = R.smooth(rows, 0, 0.5)
    part = np.isfinite(rows).all(axis=1)
    assert got[part].tobytes() == rows[part].tobytes() and np.isnan(got[~part]).all() and part.sum() == 5


def test_smooth_model_is_the_mean_of_the_neighbours_maps():
    """The smoothed row sends a network point to the weighted mean of where the neighbouring frames send it (1e-9)."""
    rows, radius, sigma = some_rows(9, 2), 3, 1.7
    rows[5] = np.nan
    got = R.smooth64(rows, radius, sigma)
    points = np.array([(0.0, 0.0), (127.5, 31.25), (256.0, 200.0)])
    images = R.apply(rows.astype(np.float64), points)
    for n in range(9):
        d = np.array([k for k in range(-radius, radius + 1) if 0 <= n + k < 9 and n + k != 5])
        g = np.exp(-d.astype(np.float64) ** 2 / (2 * sigma ** 2))
        want = (g[:, None, None] * images[n + d]).sum(axis=0) / g.sum()
        assert np.abs(R.apply(got[n:n + 1], points)[0] - want).max() <= 1e-9


# ---- the C boundary --------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_new_entries(pkg):
    L = pkg._lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spk.h")).read(), flags=re.S)
    lib = L.lib()
    for name in ("spk_sim_fit_landmarks", "spk_sim_smooth"):
        decl = re.search(name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert decl, f"{name} is not declared in include/spk.h"
        params = [p.strip() for p in decl.group(1).split(",")]
        assert name in L.exported_symbols() and len(getattr(lib, name).argtypes) == len(params), name
        for p, t in zip(params, getattr(lib, name).argtypes):         # pointers travel as void*, scalars by their C type
            want = "c_void_p" if "*" in p else {"int": "c_int", "int64_t": "c_long", "float": "c_float", "double": "c_double"}[p.split()[0]]
            assert t.__name__ == want, (name, p, t)


def test_entry_refusals_need_no_device(pkg):
    """Every refusal of the two entry points happens before a launch: -1 and a message, on a machine without a GPU."""
    lib = pkg._lib.lib()
    p = 1 << 20                  # any non-null address: the arguments are refused before anything is read or launched

    def fit(pts=p, weights=None, stride=0, tmpl=p, N=1, K=5, offset=0.0, sim=p):
        return lib.spk_sim_fit_landmarks(pts, weights, stride, tmpl, N, K, offset, sim, None)

    for bad in (dict(pts=None), dict(tmpl=None), dict(sim=None), dict(N=0), dict(N=-3), dict(K=1), dict(K=0), dict(K=4097),
                dict(K=0x7fffffff), dict(stride=-1), dict(stride=-5, weights=p), dict(stride=4, weights=p), dict(stride=1),
                dict(N=0x7fffffff, stride=4), dict(offset=float("nan")), dict(offset=float("inf")), dict(offset=float("-inf"))):
        assert fit(**bad) == -1, bad
        assert lib.spk_last_error(), bad
    assert fit(sim=None) == -1 and b"transform" in lib.spk_last_error()
    assert fit(K=4097) == -1 and b"K must be" in lib.spk_last_error()
    assert fit(stride=3) == -1 and b"weight stride" in lib.spk_last_error()
    assert fit(offset=float("nan")) == -1 and b"offset" in lib.spk_last_error()

    def smooth(src=p, N=4, radius=2, sigma=1.0, dst=p + 4096):
        return lib.spk_sim_smooth(src, N, radius, sigma, dst, None)

    for bad in (dict(src=None), dict(dst=None), dict(N=0), dict(N=-1), dict(radius=-1), dict(radius=65), dict(radius=0x7fffffff),
                dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
                dict(dst=p), dict(dst=p + 16 * 3), dict(dst=p - 16 * 3), dict(dst=p + 4), dict(N=0x7fffffff),
                dict(N=0x7fffffff, dst=p + 16 * 0x7fffffff - 16), dict(N=0x7fffffff, src=p + 16 * 0x7fffffff - 16, dst=p)):
        assert smooth(**bad) == -1, bad
        assert lib.spk_last_error(), bad
    assert smooth(dst=p + 16 * 3) == -1 and b"overlap" in lib.spk_last_error()
    assert smooth(radius=65) == -1 and b"radius" in lib.spk_last_error()
    assert smooth(sigma=0.0) == -1 and b"sigma" in lib.spk_last_error()


# ---- the three Python names and reenact_video: what is refused before a device is touched --------------------------------------
def test_python_argument_errors(pkg):
    ops, SpkError = pkg.ops, pkg._lib.SpkError
    lm = torch.zeros(3, 5, 2)
    for make in (ops.similarity_from_landmarks, ops.LandmarkAlign):
        for template in (TEMPLATE5[:4], [list(t) + [0.0] for t in TEMPLATE5], torch.zeros(5), "abcde",       # the wrong shape
                         [(float("nan"), 1.0)] + TEMPLATE5[1:], [(float("inf"), 1.0)] + TEMPLATE5[1:],           # not finite
                         [(3.0, 4.0)] * 5, torch.zeros(5, 2)):                                                # coincident points
            with pytest.raises(ValueError, match="template"):
                make(lm, template)
        for weights in ([1.0] * 4, torch.ones(3, 5), torch.ones(5, 1), [[1.0] * 5]):
            with pytest.raises(ValueError, match="weights"):
                make(lm, TEMPLATE5, weights=weights)
        for bad in (torch.zeros(3, 5), torch.zeros(3, 5, 3), torch.zeros(3, 1, 2), torch.zeros(0, 5, 2), [[TEMPLATE5]]):
            with pytest.raises(ValueError, match="landmarks"):
                make(bad, TEMPLATE5)
        with pytest.raises(ValueError, match="offset"):
            make(lm, TEMPLATE5, offset=float("nan"))
    for radius in (-1, 65, 1.5, None):
        with pytest.raises(ValueError, match="radius"):
            ops.smooth_similarity_rows(torch.zeros(3, 4), radius)
        with pytest.raises(ValueError, match="radius"):
            ops.LandmarkAlign(lm, TEMPLATE5, smooth=radius)
    for sigma in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            ops.smooth_similarity_rows(torch.zeros(3, 4), 2, sigma)
        with pytest.raises(ValueError, match="sigma"):
            ops.LandmarkAlign(lm, TEMPLATE5, smooth=2, sigma=sigma)
    for rows in (torch.zeros(3, 3), torch.zeros(4), [[1.0, 0.0, 0.0]], torch.zeros(0, 4)):
        with pytest.raises(ValueError, match="rows"):
            ops.smooth_similarity_rows(rows, 1)
    # the arguments are in order: what is left is the device
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.similarity_from_landmarks(lm, TEMPLATE5, weights=[1.0] * 5, offset=0.5)
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.similarity_from_landmarks(lm.double(), torch.tensor(TEMPLATE5))
    la = ops.LandmarkAlign(lm, TEMPLATE5, weights=torch.ones(5), smooth=2)
    assert la.smooth == 2 and la.sigma == 1.0 and ops.LandmarkAlign(lm, TEMPLATE5).smooth == 0
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        la.rows(3)
    with pytest.raises(ValueError, match="3 frames for 4"):
        la.rows(4)


def test_reenact_video_argument_errors(pkg):
    import model
    ops = pkg.ops
    m = model.IRFD()
    ident, video = torch.zeros(48, 64, 3, dtype=torch.uint8), torch.zeros(3, 48, 64, 3, dtype=torch.uint8)
    surf = torch.zeros(3, 72, 64, dtype=torch.uint8)
    good, la3, la1 = [[0.25, 0, 3, 4]] * 3, ops.LandmarkAlign(torch.zeros(3, 5, 2), TEMPLATE5), ops.LandmarkAlign(torch.zeros(1, 5, 2), TEMPLATE5)
    with pytest.raises(ValueError, match="align"):                          # a LandmarkAlign of another frame count
        m.reenact_video(ident, video, align=ops.LandmarkAlign(torch.zeros(2, 5, 2), TEMPLATE5))
    with pytest.raises(ValueError, match="align"):
        m.reenact_video(ident, video, align=la1, paste=True)
    with pytest.raises(ValueError, match="identity_align"):
        m.reenact_video(ident, video, align=good, identity_align=la3)
    for rows in ([[1, 0, 0, float("nan")]], [[0, 0, 3, 4]], [[32, 0, 0, 0]], [[1, 0, 0]], good, [1, 0, 0, 0]):
        for form in (rows, torch.tensor(rows, dtype=torch.float64)):
            with pytest.raises(ValueError, match="identity_align"):
                m.reenact_video(ident, video, identity_align=form)
            with pytest.raises(ValueError, match="identity_align"):
                m.reenact_video(ident, surf, identity_align=form, pixel_format="nv12", crop=(0, 0, 48, 64))
    # the existing rules hold as they were, a LandmarkAlign included
    with pytest.raises(ValueError, match="crop and align"):
        m.reenact_video(ident, video, crop=(3, 5, 40, 44), align=la3)
    with pytest.raises(ValueError, match="align applies to pixel_format='rgb24' only"):
        m.reenact_video(ident, surf, align=la3, pixel_format="nv12")
    # the arguments are in order: what is left is the device
    for kw in (dict(align=la3), dict(align=good, identity_align=la1), dict(identity_align=[[0.25, 0, 3, 4]])):
        with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
            m.reenact_video(ident, video, **kw)
