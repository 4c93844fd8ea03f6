"""The numpy fp64 model of the two causal filters (csrc/causal_filter.hip; the definitions are in include/spk.h), written from the
definitions: a Python loop per frame and group, plain ``*`` and ``+`` (no fma), the state a plain array that a call reads and
writes.  The colour rows use the row formula of ``blend_ref.colour_rows`` (what tests/colour_window_ref.py builds on).  Also the
series the CPU and GPU tests share, built by name, computed once, never written into."""
import functools

import numpy as np

import blend_ref as B
import colour_window_ref as CW

SUMS = CW.SUMS
DEFAULTS = dict(rate=30.0, min_cutoff=1.0, beta=0.05, d_cutoff=1.0, hold=5)


def alpha(cutoff, Te):
    return 1.0 / (1.0 + 1.0 / (2.0 * np.pi * cutoff * Te))


def empty_state(D, group):
    return np.zeros((D // group, 2 + 2 * group))


def causal_filter(x, state, weights=None, group=2, rate=30.0, min_cutoff=1.0, beta=0.05, d_cutoff=1.0, hold=5):
    """``x`` [N,D] (fp32 values), ``weights`` None, [G] or [N,G]; ``state`` fp64 [G, 2 + 2 group], UPDATED IN PLACE.
    -> (y fp64 [N,D], NaN where the definition says so and NOT rounded to fp32; wy fp64 [N,G])"""
    x = np.asarray(x, dtype=np.float64)
    N, D = x.shape
    G = D // group
    assert G * group == D and state.shape == (G, 2 + 2 * group)
    w = np.ones((N, G)) if weights is None else np.broadcast_to(np.asarray(weights, dtype=np.float64), (N, G))
    y, wy = np.full((N, D), np.nan), np.zeros((N, G))
    for n in range(N):
        for g in range(G):
            k, w_last = state[g, 0], state[g, 1]
            xh, dh = state[g, 2:2 + group].copy(), state[g, 2 + group:].copy()
            xs = x[n, g * group:(g + 1) * group]
            part = bool(np.isfinite(w[n, g]) and w[n, g] > 0 and np.isfinite(xs).all())
            if part:
                if k == 0 or k - 1 > hold:
                    xh, dh = xs.copy(), np.zeros(group)
                else:
                    Te = k / rate
                    a_d = alpha(d_cutoff, Te)
                    dh = a_d * ((xs - xh) / Te) + (1.0 - a_d) * dh
                    a_x = alpha(min_cutoff + beta * np.sqrt(np.sum(dh * dh)), Te)
                    xh = a_x * xs + (1.0 - a_x) * xh
                k, w_last = 1.0, w[n, g]
                y[n, g * group:(g + 1) * group], wy[n, g] = xh, w[n, g]
            else:
                if 1 <= k <= hold:
                    y[n, g * group:(g + 1) * group], wy[n, g] = xh, w_last
                if k >= 1:
                    k += 1
            state[g, 0], state[g, 1], state[g, 2:2 + group], state[g, 2 + group:] = k, w_last, xh, dh
    return y, wy


def colour_rows_causal(sums, state, decay, max_gain=2.0, min_sigma=1.0, min_weight=16.0):
    """``sums`` fp64 [N,13]; ``state`` fp64 [13], UPDATED IN PLACE.  -> dict(rows [N,3,2] fp64, NOT rounded to fp32; P [N,13]: the pooled
    sums after each frame; part bool [N])"""
    sums = np.asarray(sums, dtype=np.float64)
    N = sums.shape[0]
    P, part = np.zeros((N, SUMS)), np.zeros(N, dtype=bool)
    for n in range(N):
        with np.errstate(invalid="ignore"):
            part[n] = bool(sums[n, 0] > min_weight and np.isfinite(sums[n]).all())
        if part[n]:
            state[:] = decay * state + sums[n]
        P[n] = state
    with np.errstate(invalid="ignore", divide="ignore"):
        rows, _, _ = B.colour_rows(P, np.ones(N, dtype=bool), max_gain, min_sigma, min_weight)
    return dict(rows=rows, P=P, part=part)


def same(a, b):
    """``array_equal`` with NaNs equal"""
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


# ---- the series the tests share --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def series(name):
    """-> (x fp32 [N,D], weights fp32 [N,G] or None, group), read-only.
    ``landmarks``: N = 9 frames of K = 5 moving landmarks (D = 10, group 2).  The drop-out pattern, for hold = 2: point 1 is lost
    for 2 frames (3, 4: bridged), point 2 for 4 frames (2 ... 5: held, held, NaN, NaN, then the sample itself), point 3 is never
    valid, point 4 has a zero weight in frame 1 and a NaN weight in frame 6; frame 7 is NaN in every point.
    ``features``: N = 9 frames of D = 257 components, group 1, frame 4 NaN throughout and a few NaN entries.
    ``triples``: N = 9 frames of D = 6, group 3, one group lost for three frames through one component."""
    rng = np.random.default_rng({"landmarks": 41, "features": 42, "triples": 43}[name])
    N = 9
    t = np.arange(N, dtype=np.float64)[:, None]
    if name == "landmarks":
        base = 40.0 + 60.0 * rng.random((1, 10))
        x = base + t * rng.normal(0.0, 1.5, (1, 10)) + rng.normal(0.0, 0.5, (N, 10))
        w = 0.5 + rng.random((N, 5))
        x[3:5, 2:4] = np.nan
        x[2:6, 4] = np.nan                                                  # one component is enough
        x[:, 6:8] = np.inf
        w[1, 4], w[6, 4] = 0.0, np.nan
        x[7] = np.nan
        group = 2
    elif name == "features":
        x = rng.normal(0.0, 1.0, (1, 257)) + 0.1 * t * rng.normal(0.0, 1.0, (1, 257)) + rng.normal(0.0, 0.05, (N, 257))
        x[4] = np.nan
        x[1, 256], x[2:8, 64], x[8, 0] = np.nan, np.nan, -np.inf
        w, group = None, 1
    else:
        x = 10.0 * rng.random((1, 6)) + t * rng.normal(0.0, 0.3, (1, 6)) + rng.normal(0.0, 0.1, (N, 6))
        x[3:6, 4] = np.nan
        w, group = None, 3
    x = x.astype(np.float32)
    x.setflags(write=False)
    if w is not None:
        w = w.astype(np.float32)
        w.setflags(write=False)
    return x, w, group


@functools.lru_cache(maxsize=None)
def still_point(N=200, sigma=0.5, seed=7):
    """A landmark that stands still at (120, 80) under N(0, sigma) tracker noise -> fp32 [N,2], read-only"""
    x = (np.array([[120.0, 80.0]]) + np.random.default_rng(seed).normal(0.0, sigma, (N, 2))).astype(np.float32)
    x.setflags(write=False)
    return x
