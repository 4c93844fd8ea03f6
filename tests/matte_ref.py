"""A numpy fp64 model of ``spk_matte_from_landmarks`` (csrc/landmark_matte.hip), written from its definition in include/spk.h and
not from the kernel: the contour landmarks mapped back through their frame's row (``mapped``), the Gaussian window over the frames
with its fallback (``outline``), the signed distance to the closed outline with even-odd parity (``signed_distance``, vectorised over
edges; ``signed_distance_loop``, a plain loop per point and per edge) and the ramp (``matte64`` / ``matte``).  Inputs are rounded to
fp32 first, as the kernel receives them.  Also here: the cases the CPU and the GPU tests share (``CASES``, ``case``, ``big_case``)."""
import numpy as np

import landmark_ref as LR

S_MIN, S_MAX = 1.0 / 16.0, 16.0


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def mapped(pts, sim, contour, offset=0.0):
    """-> (p [N,Kc,2] fp64 in generated-image coordinates, part [N,Kc]): the point of frame n and contour index k takes part when
    row n is valid (finite, 1/16 <= s <= 16) and its x, y are finite"""
    pts, sim = _f32(pts), _f32(sim)
    xy = pts[:, list(contour), :] + offset
    a, c, tx, ty = (sim[:, i:i + 1] for i in range(4))
    with np.errstate(all="ignore"):
        s = np.sqrt(a * a + c * c)
        valid = np.isfinite(sim).all(axis=1, keepdims=True) & (s >= S_MIN) & (s <= S_MAX)
        part = valid & np.isfinite(xy).all(axis=2)
        dx, dy, s2 = xy[:, :, 0] - tx, xy[:, :, 1] - ty, a * a + c * c
        p = np.stack([(a * dx + c * dy) / s2, (-c * dx + a * dy) / s2], axis=2)
    return p, part


def outline(pts, sim, contour, offset=0.0, radius=0, sigma=1.0, fallback=None):
    """-> (P [N,Kc,2], hole [N]): the window d = -radius ... radius over the points that take part; a point without one comes from
    ``fallback`` [Kc,2]; ``hole[n]``: such a point is needed and there is no (finite) fallback -- the matte of frame n is zeros"""
    p, part = mapped(pts, sim, contour, offset)
    N, Kc, _ = p.shape
    P, hole = np.zeros((N, Kc, 2)), np.zeros(N, dtype=bool)
    fb = None if fallback is None else _f32(fallback)
    for n in range(N):
        for k in range(Kc):
            ds = [d for d in range(-radius, radius + 1) if 0 <= n + d < N and part[n + d, k]]
            g = np.exp(-np.array(ds, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
            if ds and g.sum() > 0:
                P[n, k] = p[n + ds[0], k] if len(ds) == 1 else (g[:, None] * p[[n + d for d in ds], k]).sum(axis=0) / g.sum()
            elif fb is not None and np.isfinite(fb[k]).all():
                P[n, k] = fb[k]
            else:
                hole[n] = True
    return P, hole


def signed_distance(P, x, y):
    """The signed distance of the points (x, y) (arrays of one shape) to the closed outline P [Kc,2]: the smallest point-segment
    distance over the edges (P[e], P[(e + 1) % Kc]), positive where the crossing number is odd"""
    P = np.asarray(P, dtype=np.float64)
    x, y = np.asarray(x, dtype=np.float64)[..., None], np.asarray(y, dtype=np.float64)[..., None]
    A, B = P, np.roll(P, -1, axis=0)
    ex, ey = B[:, 0] - A[:, 0], B[:, 1] - A[:, 1]
    len2 = ex * ex + ey * ey
    with np.errstate(all="ignore"):
        t = np.where(len2 > 0, np.clip(((x - A[:, 0]) * ex + (y - A[:, 1]) * ey) / len2, 0.0, 1.0), 0.0)
        dist = np.sqrt((x - (A[:, 0] + t * ex)) ** 2 + (y - (A[:, 1] + t * ey)) ** 2).min(axis=-1)
        cross = ((A[:, 1] > y) != (B[:, 1] > y)) & (x < A[:, 0] + (y - A[:, 1]) * ex / ey)
    inside = cross.sum(axis=-1) % 2 == 1
    return np.where(inside, dist, -dist)


def signed_distance_loop(P, x, y):
    """``signed_distance`` as its definition reads: a loop per point and per edge"""
    P = np.asarray(P, dtype=np.float64)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = np.empty(x.shape)
    for at in np.ndindex(x.shape):
        px, py, best, inside = x[at], y[at], np.inf, False
        for e in range(len(P)):
            (ax, ay), (bx, by) = P[e], P[(e + 1) % len(P)]
            len2 = (bx - ax) ** 2 + (by - ay) ** 2
            t = min(max(((px - ax) * (bx - ax) + (py - ay) * (by - ay)) / len2, 0.0), 1.0) if len2 > 0 else 0.0
            best = min(best, np.sqrt((px - (ax + t * (bx - ax))) ** 2 + (py - (ay + t * (by - ay))) ** 2))
            if (ay > py) != (by > py) and px < ax + (py - ay) * (bx - ax) / (by - ay):
                inside = not inside
        out[at] = best if inside else -best
    return out


def centres(Hs, Ws):
    """-> (x, y) [Hs,Ws]: the centre of pixel (j, i) is (i + 0.5, j + 0.5)"""
    return np.meshgrid(np.arange(Ws) + 0.5, np.arange(Hs) + 0.5)


def matte64(pts, sim, size_hw, contour, softness=4.0, grow=0.0, offset=0.0, fallback=None, radius=0, sigma=None, distance=signed_distance):
    """-> (dg [N,Hs,Ws] = d + grow in fp64, -inf in a frame of zeros; P; hole)"""
    Hs, Ws = size_hw
    sigma = max(radius, 1) / 2.0 if sigma is None else sigma
    P, hole = outline(pts, sim, contour, offset, radius, sigma, fallback)
    x, y = centres(Hs, Ws)
    dg = np.stack([np.full((Hs, Ws), -np.inf) if hole[n] else distance(P[n], x, y) + grow for n in range(len(P))])
    return dg, P, hole


def ramp(dg, softness):
    """-> float32: what the kernel stores"""
    return np.clip(dg / softness, 0.0, 1.0).astype(np.float32)


def matte(pts, sim, size_hw, contour, softness=4.0, **kw):
    return ramp(matte64(pts, sim, size_hw, contour, softness, **kw)[0], softness)


POPULATED = (50, 1, 20)         # what a frame of a test case holds at least: pixels that must be 0, that must be 1, on the ramp


def counts(dg, softness):
    """-> (pixels that must be exactly 0, pixels that must be exactly 1, pixels on the ramp) by the rule of the GPU tests"""
    zero, one = dg <= -1e-6, dg >= softness + 1e-6
    return int(zero.sum()), int(one.sum()), int(((dg > 0) & (dg < softness)).sum())


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------------
N, K, SOFTNESS = 5, 12, 1.5
# the identity, a rotation, s < 1, s > 2, a large rotation: rows that map the generated image into the frames
ROWS = np.array([[1.0, 0.0, 0.0, 0.0]] + [[s * np.cos(th), s * np.sin(th), tx, ty] for s, th, tx, ty in
                                          ((1.1, 0.4, 30.5, 12.25), (0.6, -0.3, 7.0, 40.0), (2.7, 1.2, 90.0, -15.5), (1.0, 2.5, 64.0, 70.0))],
                dtype=np.float32)
# rows whose arithmetic is exact, so that a vertex put on a pixel centre comes back there to the bit: the identity, s = 2, s = 1/2,
# a quarter turn, a quarter turn the other way at s = 4
EXACT_ROWS = np.array([[1, 0, 0, 0], [2, 0, 3, 5], [0.5, 0, 1, 2], [0, 1, 20, 0], [0, -4, -8, 64]], dtype=np.float32)
STAR = list(range(12))                                                    # concave: the radii alternate
CROSSED = [0, 4, 8, 2, 2, 6, 10]                                          # self-crossing, and one index twice: a degenerate edge
TRIANGLE = [0, 4, 8]
CASES = {                                                                 # name: (Hs, Ws), contour, grow, radius, vertices on pixel centres
    "star 16x16": ((16, 16), STAR, 0.0, 0, False),
    "crossed 12x20 grown smoothed": ((12, 20), CROSSED, 1.5, 2, False),
    "triangle 16x16 shrunk smoothed": ((16, 16), TRIANGLE, -1.0, 2, False),
    "star on pixel centres 16x16": ((16, 16), STAR, 0.0, 0, True),
    "crossed 16x16 smoothed": ((16, 16), CROSSED, 0.0, 2, False),
    "star 12x20 shrunk": ((12, 20), STAR, -1.0, 0, False),
}


def base_points(Hs, Ws, K=K):
    """K points around the image's centre, radii alternating between 0.44 and 0.24 of the size"""
    th = 2.0 * np.pi * np.arange(K) / K
    r = np.where(np.arange(K) % 2 == 0, 0.44, 0.24)
    return np.stack([Ws * (0.5 + r * np.cos(th)), Hs * (0.5 + r * np.sin(th))], axis=1)


def case(name, seed=0):
    """-> dict: pts float32 [N,K,2] in frame coordinates, sim float32 [N,4], and the arguments of the call"""
    (Hs, Ws), contour, grow, radius, on_centres = CASES[name]
    rng = np.random.default_rng(seed)
    base = base_points(Hs, Ws)
    if on_centres:
        g = np.tile(np.floor(base) + 0.5, (N, 1, 1))
        g[1:, 1::2] += rng.integers(-1, 2, (N - 1, K // 2, 2))            # the inner points move by whole pixels from frame to frame
        rows = EXACT_ROWS
    else:
        g = base[None] + 0.4 * rng.standard_normal((N, K, 2))
        rows = ROWS
    pts = np.stack([LR.apply(rows[n:n + 1], g[n])[0] for n in range(N)]).astype(np.float32)
    return dict(pts=pts, sim=rows.copy(), size=(Hs, Ws), contour=contour, grow=grow, radius=radius, softness=SOFTNESS, generated=g)


def big_case():
    """One frame, 64 x 64, Kc = 128 of K = 130 landmarks on a wobbling circle: the contour's upper bound, several workgroups"""
    K = 130
    rng = np.random.default_rng(7)
    th = 2.0 * np.pi * np.arange(K) / K
    r = 22.0 + 3.0 * np.sin(5 * th) + 0.3 * rng.standard_normal(K)
    g = np.stack([32.0 + r * np.cos(th), 32.0 + r * np.sin(th)], axis=1)
    row = np.array([[1.3 * np.cos(0.7), 1.3 * np.sin(0.7), 11.0, 5.5]], dtype=np.float32)
    return dict(pts=LR.apply(row, g).astype(np.float32), sim=row, size=(64, 64), contour=list(range(1, 129)), grow=0.5, radius=0,
                softness=3.0, generated=g[None])
