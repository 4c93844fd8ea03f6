"""A numpy fp64 model of the two definitions of csrc/landmark_sim.hip, written from their text in include/spk.h and not from the
kernels: the weighted least-squares similarity of a template onto a frame's landmarks (``fit``), and the Gaussian window over the
rows of neighbouring frames (``smooth``).  Inputs are rounded to fp32 first, as the kernels receive them; every sum is a plain
``np.sum``.  ``fit64`` / ``smooth64`` return the numbers in front of the final rounding to fp32.  Also here: the cases the CPU and
the GPU tests share (``case``), and the bound of the GPU tests (``bound``)."""
import numpy as np

NAN4 = np.full(4, np.nan)


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def apply(rows, points):
    """rows [N,4] applied to points [K,2] of (u, v) -> [N,K,2] of (x, y), fp64: x = a u - c v + tx, y = c u + a v + ty"""
    r, p = np.asarray(rows, dtype=np.float64), np.asarray(points, dtype=np.float64)
    a, c, tx, ty = (r[:, i:i + 1] for i in range(4))
    u, v = p[None, :, 0], p[None, :, 1]
    return np.stack([a * u - c * v + tx, c * u + a * v + ty], axis=2)


def participants(pts, weights, n, offset=0.0):
    """-> (w, x, y, mask) of frame n in fp64: a landmark takes part when its weight is finite and > 0 and its x, y are finite"""
    return _participants(_f32(pts), None if weights is None else _f32(weights), n, offset)


def _participants(pts, weights, n, offset):                               # the same of arrays that are fp64 already
    x, y = pts[n, :, 0] + offset, pts[n, :, 1] + offset
    w = np.ones(pts.shape[1]) if weights is None else weights if weights.ndim == 1 else weights[n]
    with np.errstate(invalid="ignore"):
        mask = np.isfinite(w) & (w > 0) & np.isfinite(x) & np.isfinite(y)
    return w, x, y, mask


def fit64(pts, tmpl, weights=None, offset=0.0):
    """-> float64 [N,4]: (a, c, tx, ty) per frame in front of the rounding to fp32; four NaNs with fewer than two participants or
    when D > 0 does not hold"""
    pts, tmpl, weights = _f32(pts), _f32(tmpl), None if weights is None else _f32(weights)
    N = pts.shape[0]
    out = np.empty((N, 4))
    for n in range(N):
        w, x, y, mask = _participants(pts, weights, n, offset)
        out[n] = NAN4
        if mask.sum() < 2:
            continue
        w, x, y, u, v = w[mask], x[mask], y[mask], tmpl[mask, 0], tmpl[mask, 1]
        W = np.sum(w)
        um, vm, xm, ym = np.sum(w * u) / W, np.sum(w * v) / W, np.sum(w * x) / W, np.sum(w * y) / W
        du, dv, dx, dy = u - um, v - vm, x - xm, y - ym
        with np.errstate(all="ignore"):
            D = np.sum(w * (du * du + dv * dv))
            if not D > 0:
                continue
            a, c = np.sum(w * (du * dx + dv * dy)) / D, np.sum(w * (du * dy - dv * dx)) / D
            out[n] = a, c, xm - (a * um - c * vm), ym - (c * um + a * vm)
    return out


def _store(rows64):
    """the rows as the kernels store them: rounded to fp32, and four NaNs where one of the four is not finite"""
    with np.errstate(over="ignore"):
        rows = rows64.astype(np.float32)
    rows[~np.isfinite(rows).all(axis=1)] = np.nan
    return rows


def fit(pts, tmpl, weights=None, offset=0.0):
    """-> float32 [N,4], the rows ``spk_sim_fit_landmarks`` stores"""
    return _store(fit64(pts, tmpl, weights, offset))


def smooth64(rows, radius, sigma):
    """-> float64 [N,4]: the window d = -radius ... radius over the rows that exist and are finite, in front of the rounding"""
    r = _f32(rows)
    N = r.shape[0]
    part = np.isfinite(r).all(axis=1)
    out = np.empty((N, 4))
    for n in range(N):
        idx = np.array([n + d for d in range(-radius, radius + 1) if 0 <= n + d < N and part[n + d]], dtype=np.int64)
        if idx.size == 0:
            out[n] = NAN4
            continue
        d = (idx - n).astype(np.float64)
        g = np.exp(-(d * d) / (2.0 * sigma * sigma))
        terms = g[:, None] * r[idx]
        # a sum of one term is that term: np.sum starts from +0 and would turn a -0 into +0, and radius = 0 copies bit for bit
        out[n] = (terms[0] if idx.size == 1 else np.sum(terms, axis=0)) / np.sum(g)
    return out


def smooth(rows, radius, sigma):
    """-> float32 [N,4], the rows ``spk_sim_smooth`` stores"""
    return _store(smooth64(rows, radius, sigma))


def bound(want):
    """The bound of the GPU tests on every number: one spacing of fp32 at the model's value -- one rounding to fp32 is half of it, a
    tie the model rounds the other way the other half -- plus 1e-9 for the order of the fp64 sums."""
    return np.spacing(np.abs(np.asarray(want, dtype=np.float32))).astype(np.float64) + 1e-9


def compare(got, want):
    """got, want float32 [N,4] -> the largest ratio of |got - want| to ``bound``; the NaN patterns must be equal"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)) / bound(want[ok])).max())


def case(K, N=6, seed=0, bad=True):
    """A batch of frames: a template of K points in a 256 network image, a transform per frame with a scale in 0.07 ... 15, any
    angle and translations in -500 ... 4000, 2 pixels of noise on every landmark, all in fp32; weights per frame and one
    broadcast set.  ``bad``: a NaN and an Inf coordinate, and zero, negative, NaN and Inf weights are planted (see the code for
    where); with K = 2 a frame that holds one of them has one participant left."""
    rng = np.random.default_rng(1000 * K + seed)
    tmpl = rng.uniform(16.0, 240.0, (K, 2)).astype(np.float32)
    s = np.exp(rng.uniform(np.log(0.07), np.log(15.0), N))
    th = rng.uniform(-np.pi, np.pi, N)
    rows = np.stack([s * np.cos(th), s * np.sin(th), rng.uniform(-500.0, 4000.0, N), rng.uniform(-500.0, 4000.0, N)], axis=1)
    pts = (apply(rows, tmpl) + 2.0 * rng.standard_normal((N, K, 2))).astype(np.float32)
    w_frames = rng.uniform(0.1, 1.0, (N, K)).astype(np.float32)
    w_bcast = rng.uniform(0.1, 1.0, K).astype(np.float32)
    if bad:
        pts[2 % N, 1, 0] = np.nan
        pts[4 % N, 0, 1] = np.inf
        w_frames[1 % N, 0], w_frames[1 % N, K - 1] = 0.0, -1.0
        w_frames[3 % N, 1] = np.nan
        w_frames[5 % N, 0] = np.inf
        if K >= 5:
            w_bcast[0], w_bcast[2] = 0.0, np.nan
        if K >= 68:
            w_bcast[3], w_bcast[4] = -2.0, np.inf
    return dict(tmpl=tmpl, rows=rows, pts=pts, w_frames=w_frames, w_bcast=w_bcast)
