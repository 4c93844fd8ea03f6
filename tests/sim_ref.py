"""The numpy fp64 model of the aligned video edge (csrc/frame_sim.hip; the definitions are in include/spk.h), written from the
definitions and not from the kernels: every frame pixel takes part in every sum, there is no footprint, no interval and no tap
window.  Rows are rounded to fp32 first, as the kernels read them, and everything after that is fp64."""
import numpy as np

S_MIN, S_MAX = 1.0 / 16.0, 16.0


def rows64(sim):
    """The rows as the kernels see them: rounded to fp32, promoted to fp64.  -> [N,4]"""
    return np.asarray(sim, dtype=np.float64).astype(np.float32).astype(np.float64).reshape(-1, 4)


def scale_of(row):
    return float(np.sqrt(row[0] * row[0] + row[1] * row[1]))


def is_valid(row):
    return bool(np.all(np.isfinite(row))) and S_MIN <= scale_of(row) <= S_MAX


def tri(t):
    return np.maximum(0.0, 1.0 - np.abs(t))


def rows(centre_yx, side, angle, size_hw):
    """Closed form of a row: the ``size_hw`` network image onto the rectangle whose width is ``side`` frame pixels, centred at
    ``centre_yx``, rotated by ``angle``.  fp64, not rounded."""
    s = side / size_hw[1]
    a, c = s * np.cos(angle), s * np.sin(angle)
    u0, v0 = size_hw[1] / 2.0, size_hw[0] / 2.0
    return [a, c, centre_yx[1] - (a * u0 - c * v0), centre_yx[0] - (c * u0 + a * v0)]


def warp_in(frames_u8, sim, Hout, Wout, scale=(2 / 255.0,) * 3, shift=(-1.0,) * 3, swap_rb=False):
    """The way in.  frames_u8 uint8 [N,H,W,3] -> (dst fp64 [N,3,Hout,Wout], the value in front of the cast to fp32;
    hit bool [N,Hout,Wout], False where V = 0 by rule: an invalid row or Wt <= 0, whose outputs are shift_c exactly)."""
    src = np.asarray(frames_u8).astype(np.float64)
    N, H, W, _ = src.shape
    sim = rows64(sim)
    dst = np.empty((N, 3, Hout, Wout))
    hit = np.zeros((N, Hout, Wout), dtype=bool)
    u, v = np.meshgrid(np.arange(Wout) + 0.5, np.arange(Hout) + 0.5)
    qx, qy = np.arange(W) + 0.5, np.arange(H) + 0.5
    for n in range(N):
        V = np.zeros((3, Hout, Wout))
        if is_valid(sim[n]):
            a, c, tx, ty = sim[n]
            s = scale_of(sim[n])
            S = max(s, 1.0)
            px, py = a * u - c * v + tx, c * u + a * v + ty
            dx = qx[None, None, None, :] - px[:, :, None, None]
            dy = qy[None, None, :, None] - py[:, :, None, None]
            w = tri((a * dx + c * dy) / s / S) * tri((-c * dx + a * dy) / s / S)          # [Hout,Wout,H,W]
            Wt = w.sum((2, 3))
            hit[n] = Wt > 0
            acc = np.einsum("opyx,yxc->cop", w, src[n])
            V = np.where(hit[n], acc / np.where(hit[n], Wt, 1.0), 0.0)
        for c_ in range(3):
            dst[n, c_] = scale[c_] * V[2 - c_ if swap_rb else c_] + shift[c_]
    return dst, hit


def paste_out(x, bg_u8, sim, feather=0.0, value_range=(-1.0, 1.0), swap_rb=False):
    """The way out.  x fp32 [N,3,Hs,Ws], bg_u8 uint8 [N,H,W,3] -> (z fp64 [N,H,W,3]: the value in front of the final rounding
    inside the region, the background byte outside; region bool [N,H,W]; margin: the smallest distance, in (u, v), of any pixel
    centre of any valid frame from the edges of its region).  The quantise chain is evaluated in fp64 here."""
    x = np.asarray(x).astype(np.float64)
    bg = np.asarray(bg_u8).astype(np.float64)
    N, _, Hs, Ws = x.shape
    _, H, W, _ = bg.shape
    sim = rows64(sim)
    lo, k = float(value_range[0]), 255.0 / (float(value_range[1]) - float(value_range[0]))
    z = bg.copy()
    region = np.zeros((N, H, W), dtype=bool)
    margin = np.inf
    X, Y = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    ci, cj = np.arange(Ws) + 0.5, np.arange(Hs) + 0.5
    for n in range(N):
        if not is_valid(sim[n]):
            continue
        a, c, tx, ty = sim[n]
        s = scale_of(sim[n])
        dx, dy = X - tx, Y - ty
        u, v = (a * dx + c * dy) / (s * s), (-c * dx + a * dy) / (s * s)
        inside = (u >= 0) & (u < Ws) & (v >= 0) & (v < Hs)
        depth = np.minimum(np.minimum(u, Ws - u), np.minimum(v, Hs - v))                 # > 0 inside
        away = np.maximum(np.maximum(-u, u - Ws), np.maximum(-v, v - Hs))                # > 0 outside
        margin = min(margin, float(np.where(inside, depth, away).min()))
        r = max(1.0, 1.0 / s)
        wu = tri((ci[None, None, :] - u[:, :, None]) / r)                                # [H,W,Ws]
        wv = tri((cj[None, None, :] - v[:, :, None]) / r)                                # [H,W,Hs]
        norm = wu.sum(2) * wv.sum(2)
        val = np.einsum("yxj,yxi,cji->yxc", wv, wu, x[n]) / np.where(inside, norm, 1.0)[:, :, None]
        q = np.clip((val - lo) * k, 0.0, 255.0)
        if swap_rb:
            q = q[:, :, ::-1]
        a_u = np.minimum(1.0, (s * np.minimum(u, Ws - u) + 0.5) / (feather + 1.0))
        a_v = np.minimum(1.0, (s * np.minimum(v, Hs - v) + 0.5) / (feather + 1.0))
        m = (a_u * a_v)[:, :, None]
        z[n] = np.where(inside[:, :, None], bg[n] + m * (q - bg[n]), bg[n])
        region[n] = inside
    return z, region, margin
