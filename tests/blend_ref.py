"""The numpy fp64 model of the seamless paste-back (csrc/frame_blend.hip; the definitions are in include/spk.h), written from the
definitions on the geometry of ``sim_ref.paste_out``: every generated pixel takes part in every sum, there is no tap window.
Rows are rounded to fp32 first, as the kernels read them; everything after that is fp64 -- with ONE deliberate departure: in the
STATISTICS ``q`` is the kernel's fp32 quantise chain, ``clip((float32(val) - float32(lo)) * float32(k), 0, 255)`` evaluated in
numpy float32 and then promoted.  An fp64 ``q`` differs from it by up to about 5e-5 byte units, systematically enough to move a
mean by more than an fp32 ulp.  In the PASTE ``q`` stays fp64, as in ``sim_ref``."""
import numpy as np

import sim_ref as R

SUMS = 13           # S0, then (Sq, Sqq, Sb, Sbb) for each network channel


def blend(x, bg_u8, sim, feather=0.0, value_range=(-1.0, 1.0), swap_rb=False, matte=None, colour=None):
    """x fp32 [N,3,Hs,Ws], bg_u8 uint8 [N,H,W,3], matte None / [Hs,Ws] / [N,Hs,Ws], colour None / [N,3,2] rows (g, o).
    -> dict: ``z`` fp64 [N,H,W,3], the value in front of the final rounding inside the region and the background byte outside;
    ``region`` bool [N,H,W]; ``margin`` as ``sim_ref.paste_out``; ``Mt`` fp64 [N,H,W] (1 without a matte, 0 outside the region);
    ``sums`` fp64 [N,13] in the order of include/spk.h, per NETWORK channel; ``valid`` bool [N].  The sums do not depend on
    ``colour``."""
    x32 = np.asarray(x, dtype=np.float32)
    x = x32.astype(np.float64)
    bg = np.asarray(bg_u8).astype(np.float64)
    N, _, Hs, Ws = x.shape
    _, H, W, _ = bg.shape
    sim = R.rows64(sim)
    lo, k = float(value_range[0]), 255.0 / (float(value_range[1]) - float(value_range[0]))
    lo32, k32 = np.float32(lo), np.float32(k)
    if matte is not None:
        matte = np.asarray(matte, dtype=np.float32).astype(np.float64).reshape(-1, Hs, Ws)
        assert matte.shape[0] in (1, N)
        matte = np.where(np.isnan(matte), 0.0, matte)                                    # a NaN sample counts as 0
    if colour is not None:
        colour = np.asarray(colour, dtype=np.float32).astype(np.float64).reshape(N, 3, 2)
    z = bg.copy()
    region = np.zeros((N, H, W), dtype=bool)
    Mt_all = np.zeros((N, H, W))
    sums = np.zeros((N, SUMS))
    valid = np.zeros(N, dtype=bool)
    margin = np.inf
    X, Y = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    ci, cj = np.arange(Ws) + 0.5, np.arange(Hs) + 0.5
    for n in range(N):
        if not R.is_valid(sim[n]):
            continue
        valid[n] = True
        a, c, tx, ty = sim[n]
        s = R.scale_of(sim[n])
        dx, dy = X - tx, Y - ty
        u, v = (a * dx + c * dy) / (s * s), (-c * dx + a * dy) / (s * s)
        inside = (u >= 0) & (u < Ws) & (v >= 0) & (v < Hs)
        depth = np.minimum(np.minimum(u, Ws - u), np.minimum(v, Hs - v))
        away = np.maximum(np.maximum(-u, u - Ws), np.maximum(-v, v - Hs))
        margin = min(margin, float(np.where(inside, depth, away).min()))
        r = max(1.0, 1.0 / s)
        wu = R.tri((ci[None, None, :] - u[:, :, None]) / r)                              # [H,W,Ws]
        wv = R.tri((cj[None, None, :] - v[:, :, None]) / r)                              # [H,W,Hs]
        norm = np.where(inside, wu.sum(2) * wv.sum(2), 1.0)
        val = np.einsum("yxj,yxi,cji->yxc", wv, wu, x[n]) / norm[:, :, None]             # by network channel
        q = np.clip((val - lo) * k, 0.0, 255.0)
        a_u = np.minimum(1.0, (s * np.minimum(u, Ws - u) + 0.5) / (feather + 1.0))
        a_v = np.minimum(1.0, (s * np.minimum(v, Hs - v) + 0.5) / (feather + 1.0))
        m = a_u * a_v
        Mt = np.ones((H, W))
        if matte is not None:
            Mt = np.einsum("yxj,yxi,ji->yx", wv, wu, matte[n if matte.shape[0] > 1 else 0]) / norm
            Mt = np.where(np.isnan(Mt), 0.0, np.clip(Mt, 0.0, 1.0))
            m = m * Mt
        # the statistics: q through the kernel's fp32 chain, b by network channel
        q32 = np.clip((val.astype(np.float32) - lo32) * k32, np.float32(0), np.float32(255)).astype(np.float64)
        bn = bg[n][:, :, ::-1] if swap_rb else bg[n]
        w = np.where(inside, m, 0.0)
        sums[n, 0] = w.sum()
        for ch in range(3):
            sums[n, 1 + 4 * ch:5 + 4 * ch] = [(w * q32[:, :, ch]).sum(), (w * q32[:, :, ch] ** 2).sum(),
                                              (w * bn[:, :, ch]).sum(), (w * bn[:, :, ch] ** 2).sum()]
        # the paste: q in fp64, the rows applied per network channel, then into the frame's channel order
        if colour is not None:
            g = np.where(np.isfinite(colour[n]).all(1), colour[n, :, 0], 1.0)
            o = np.where(np.isfinite(colour[n]).all(1), colour[n, :, 1], 0.0)
            q = np.clip(g[None, None, :] * q + o[None, None, :], 0.0, 255.0)
        if swap_rb:
            q = q[:, :, ::-1]
        m = m[:, :, None]
        z[n] = np.where(inside[:, :, None], bg[n] + m * (q - bg[n]), bg[n])
        region[n] = inside
        Mt_all[n] = np.where(inside, Mt, 0.0)
    return dict(z=z, region=region, margin=margin, Mt=Mt_all, sums=sums, valid=valid)


def colour_rows(sums, valid, max_gain=2.0, min_sigma=1.0, min_weight=16.0):
    """The rows of include/spk.h from the 13 sums, in fp64 and NOT rounded to fp32.
    -> (rows [N,3,2], var_q [N,3], var_b [N,3]); a frame with ``(1, 0)`` by rule has NaN variances."""
    N = sums.shape[0]
    rows = np.tile(np.array([1.0, 0.0]), (N, 3, 1))
    var_q, var_b = np.full((N, 3), np.nan), np.full((N, 3), np.nan)
    for n in range(N):
        S0 = sums[n, 0]
        if not valid[n] or S0 <= min_weight:
            continue
        for c in range(3):
            Sq, Sqq, Sb, Sbb = sums[n, 1 + 4 * c:5 + 4 * c]
            mu_q, mu_b = Sq / S0, Sb / S0
            var_q[n, c], var_b[n, c] = max(Sqq / S0 - mu_q * mu_q, 0.0), max(Sbb / S0 - mu_b * mu_b, 0.0)
            g = 1.0 if var_q[n, c] <= min_sigma * min_sigma else float(np.clip(np.sqrt(var_b[n, c] / var_q[n, c]), 1.0 / max_gain, max_gain))
            rows[n, c] = [g, mu_b - g * mu_q]
    return rows, var_q, var_b
