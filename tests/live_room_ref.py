"""Models for the live room's two kernels, in numpy fp64.

``colour_rows_feeds``: the rule of ``spk_colour_rows_causal_feeds`` (include/spk.h) written over all feeds at once -- the
participation mask, the pooled sums and the row formula as array operations over the feed axis -- so that it is not
``causal_ref.colour_rows_causal`` in a loop; tests/test_live_room_cpu.py holds the two equal column by column.  ``pattern``: which
feed has what in the checks (one frame under ``min_weight``, one NaN sum, clean), for any number of feeds.  ``noise_rows``: what
``spk_noise_fill_rows`` writes, from ``philox_ref``."""
import numpy as np

import blend_ref as B
import colour_window_ref as CW
import philox_ref as PR

SUMS = B.SUMS
N = 7                                                                     # frames per feed in the checks
DECAYS = (0.8, 1.0, 0.0)


def colour_rows_feeds(sums, state, decay, max_gain=2.0, min_sigma=1.0, min_weight=16.0):
    """``sums`` fp64 [N,S,13]; ``state`` fp64 [S,13], UPDATED IN PLACE.  -> dict(rows [N,S,3,2] fp64, not rounded to fp32; P [N,S,13]: the
    pooled sums of every feed after each frame; part bool [N,S])"""
    sums = np.asarray(sums, dtype=np.float64)
    n_frames, S, _ = sums.shape
    assert state.shape == (S, SUMS)
    with np.errstate(invalid="ignore"):
        part = (sums[:, :, 0] > min_weight) & np.isfinite(sums).all(axis=2)
    P = np.zeros((n_frames, S, SUMS))
    for n in range(n_frames):
        with np.errstate(invalid="ignore"):
            state[:] = np.where(part[n][:, None], decay * state + sums[n], state)
        P[n] = state
    with np.errstate(invalid="ignore", divide="ignore"):
        rows, _, _ = B.colour_rows(P.reshape(n_frames * S, SUMS), np.ones(n_frames * S, dtype=bool), max_gain, min_sigma, min_weight)
    return dict(rows=rows.reshape(n_frames, S, 3, 2), P=P, part=part)


def pattern(S):
    """-> (the feed with a frame under ``min_weight``: frame 2; the feed with a NaN sum: frame 5, sum 7; a clean feed) -- three
    different feeds where there are three, the first feed for all where there is one"""
    return (0, 0, 0) if S < 3 else (S - 1, 1, 0)


def spoil(sums):
    """``sums`` [N,S,13] of frames that all take part, numpy or torch -> a copy with the pattern in it"""
    out = sums.copy() if isinstance(sums, np.ndarray) else sums.clone()
    low, nan, _ = pattern(out.shape[1])
    out[2, low] = out[2, low] * (3.0 / float(out[2, low, 0]))
    out[5, nan, 7] = float("nan")
    return out


def takes_part(S):
    """What ``spoil`` leaves of the participation: bool [N,S]"""
    part = np.ones((N, S), dtype=bool)
    low, nan, _ = pattern(S)
    part[2, low] = part[5, nan] = False
    return part


def synthetic_sums(S, seed=5):
    """[N,S,13] sums of plausible frames that all take part: weights of a few hundred, means and deviations in levels"""
    rng = np.random.default_rng(seed)
    out = np.zeros((N, S, SUMS))
    for n in range(N):
        for s in range(S):
            out[n, s] = CW.sums_of(rng.uniform(120.0, 900.0), rng.uniform(60.0, 190.0, 3), rng.uniform(8.0, 50.0, 3), rng.uniform(60.0, 190.0, 3),
                                   rng.uniform(8.0, 50.0, 3))
    return out


def noise_rows(seeds, frames, hw, layer0=0):
    """What ``spk_noise_fill_rows`` writes: per layer an fp64 array [B, hw[l]]; row b is the plane of ``(seeds[b], frames[b])``"""
    return [np.stack([PR.noise_plane(s, f, layer0 + l, v) for s, f in zip(seeds, frames)]) for l, v in enumerate(hw)]
