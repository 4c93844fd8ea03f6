"""The numpy fp64 model of the colour rows pooled over a frame window (csrc/colour_window.hip; the definitions are in include/spk.h),
written from the definitions on top of ``blend_ref.colour_rows``: the 13 sums of a clip, a Gaussian window over the frames that take
part, then that function's row formula on the pooled sums.  Plain Python loops, ``k * S`` and ``+=`` (no fma): nothing here is
shaped after the kernel.  Also the fixtures the CPU and GPU tests share, built by name, computed once, never written into."""
import functools

import numpy as np

import blend_ref as B

SUMS = B.SUMS
RADIUS_MAX = 64


def default_sigma(radius):
    return max(radius, 1) / 2.0


def takes_part(sums, j, d, min_weight):
    """Frame ``j`` in the window of frame ``j - d``"""
    if not 0 <= j < sums.shape[0] or not sums[j, 0] > min_weight:          # a NaN S0 fails the comparison
        return False
    return d == 0 or bool(np.isfinite(sums[j]).all())


def pooled(sums, radius=0, sigma=None, min_weight=16.0, start=0, stop=None):
    """-> (P fp64 [n,13], any bool [n], terms int [n]): the pooled sums of frames ``start ... stop - 1``, whether a frame took
    part, and how many did"""
    sums = np.asarray(sums, dtype=np.float64)
    T = sums.shape[0]
    stop = T if stop is None else stop
    sigma = default_sigma(radius) if sigma is None else float(sigma)
    P, hit, terms = np.zeros((stop - start, SUMS)), np.zeros(stop - start, dtype=bool), np.zeros(stop - start, dtype=int)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(start, stop):
            for d in range(-radius, radius + 1):
                if takes_part(sums, t + d, d, min_weight):
                    P[t - start] += np.exp(-(d * d) / (2.0 * sigma * sigma)) * sums[t + d]
                    hit[t - start] = True
                    terms[t - start] += 1
    return P, hit, terms


def window_rows(sums, radius=0, sigma=None, max_gain=2.0, min_sigma=1.0, min_weight=16.0, start=0, stop=None):
    """The rows of include/spk.h, in fp64 and NOT rounded to fp32.  -> dict(rows [n,3,2], var_q [n,3], var_b [n,3] (NaN where the row
    is (1, 0) by rule), P [n,13], any [n], terms [n]).  ``blend_ref.colour_rows`` applies the row formula to P; its own
    ``S0 <= min_weight`` rule is switched off, since the window's rule is about the frames, not about P."""
    P, hit, terms = pooled(sums, radius, sigma, min_weight, start, stop)
    with np.errstate(invalid="ignore", divide="ignore"):
        rows, var_q, var_b = B.colour_rows(P, hit, max_gain, min_sigma, -np.inf)
    return dict(rows=rows, var_q=var_q, var_b=var_b, P=P, any=hit, terms=terms)


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
def sums_of(S0, mu_q, sd_q, mu_b, sd_b):
    """The 13 sums of a frame of weight ``S0`` whose channels have the given means and standard deviations (3 each)"""
    out = [float(S0)]
    for c in range(3):
        out += [S0 * mu_q[c], S0 * (sd_q[c] ** 2 + mu_q[c] ** 2), S0 * mu_b[c], S0 * (sd_b[c] ** 2 + mu_b[c] ** 2)]
    return np.array(out)


@functools.lru_cache(maxsize=None)
def flicker_clip(T=9, drop=1, swing=12.0):
    """A steady generated face over a background whose mean alternates by +-``swing`` levels from frame to frame; frame ``drop``
    has no statistics (13 zeros: an invalid row, or a matte that is all zero).  The drop-out sits next to the clip's start: in the
    interior of a strictly alternating clip its two neighbours are in the same phase and have, by symmetry, the same pooled row,
    so "between its neighbours" could only mean "equal to both"; at frame 1 the windows of frames 0, 1 and 2 reach one, two and
    three frames further into the alternation, the share of the other phase grows from frame to frame, and "between" says
    something.  -> fp64 [T,13], read-only"""
    rng = np.random.default_rng(5)
    clip = np.zeros((T, SUMS))
    for t in range(T):
        if t == drop:
            continue
        sign = 1.0 if t % 2 == 0 else -1.0
        clip[t] = sums_of(900.0 + 40.0 * rng.random(), [118.0, 96.0, 84.0], [31.0, 28.0, 26.0],
                          [130.0 + sign * swing, 104.0 + sign * swing, 90.0 + sign * swing], [36.0, 33.0, 29.0])
    clip.setflags(write=False)
    return clip


@functools.lru_cache(maxsize=None)
def window_clip(name):
    """The clips of the GPU window test, T = 7 -> fp64 [7,13], read-only.  ``plain``: seven usable frames of different weights,
    means and spreads.  ``holes``: frame 2 has a NaN S0, frame 3 is all zero, frame 5 has a finite S0 and a NaN Sq (a neighbour to
    nobody, but itself served).  ``gap``: frames 1 ... 5 are unusable (zeros, a NaN S0, a weight of exactly min_weight, a weight below it, S0 = -inf),
    so that at radius 1 and 2 the frames in the middle see no frame at all."""
    rng = np.random.default_rng({"plain": 11, "holes": 12, "gap": 13}[name])
    clip = np.zeros((7, SUMS))
    for t in range(7):
        clip[t] = sums_of(300.0 + 900.0 * rng.random(), 60.0 + 120.0 * rng.random(3), 12.0 + 30.0 * rng.random(3), 50.0 + 140.0 * rng.random(3),
                          10.0 + 40.0 * rng.random(3))
    if name == "holes":
        clip[2, 0] = np.nan
        clip[3] = 0.0
        clip[5, 1] = np.nan
    if name == "gap":
        clip[1] = 0.0
        clip[2, 0] = np.nan
        clip[3] *= 16.0 / clip[3, 0]
        clip[3, 0] = 16.0                                                   # S0 == min_weight exactly: not above it
        clip[4] *= 3.0 / clip[4, 0]                                         # a weight below min_weight
        clip[5, 0] = -np.inf
    clip.setflags(write=False)
    return clip
