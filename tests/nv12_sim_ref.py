"""The numpy fp64 model of the aligned NV12 edge (csrc/frame_sim_nv12.hip; the definitions are in include/spk.h), written from the
definitions on top of ``sim_ref`` (the geometry of the way in), ``blend_ref`` (the geometry, matte, colour rows and sums of the way
out) and ``nv12_ref`` (the replicated fields and the 3 x 4 maps).  None of them is restated here:

* way in: ``sim_ref.warp_in`` with scale 1 and shift 0 on the three replicated fields IS the three weighted means; the matrix,
  the clamp and the normalisation follow.
* way out: ``blend_ref.blend`` is affine in its background, ``z = (1 - m) b + m q'``.  Over a background of zeros it returns
  ``m q'``, over a background of ones ``1 - m + m q'``; their difference gives ``m``.  ``from_rgb`` is affine too, so
  ``m e = F (m q') + m offset`` needs no division by a small ``m``.  The sums of the statistics are ``blend_ref``'s over the
  background ``clamp(to_rgb . (Y, U, V, 1))`` in fp64 (with its fp32 ``q``, as there)."""
import numpy as np
import torch

import blend_ref as B
import nv12_ref as NR
import sim_ref as R


def fields(y, uv):
    """uint8 planes y [N,H,W], uv [N,H/2,W/2,2] -> the three component fields by replication, fp64 [N,H,W,3] (Y, U, V)."""
    f = NR.fields(torch.as_tensor(np.asarray(y)), torch.as_tensor(np.asarray(uv)))
    return f.permute(0, 2, 3, 1).numpy()


def background(y, uv, to_rgb):
    """What the way in makes of every pixel: clamp(to_rgb . (Y, U, V, 1)), fp64 [N,H,W,3] (R, G, B)."""
    M = np.asarray(to_rgb, dtype=np.float64)
    return np.clip(fields(y, uv) @ M[:, :3].T + M[:, 3], 0.0, 255.0)


def warp_in(y, uv, sim, Hout, Wout, to_rgb, scale=(2 / 255.0,) * 3, shift=(-1.0,) * 3, swap_rb=False):
    """-> (dst fp64 [N,3,Hout,Wout] in front of the cast to fp32; hit bool [N,Hout,Wout], False where the output is shift exactly)"""
    M = np.asarray(to_rgb, dtype=np.float64)
    mean, hit = R.warp_in(fields(y, uv), sim, Hout, Wout, scale=(1.0,) * 3, shift=(0.0,) * 3)       # [N,3,Hout,Wout]: (Y, U, V) / Wt
    rgb = np.clip(np.einsum("cj,njyx->ncyx", M[:, :3], mean) + M[:, 3].reshape(1, 3, 1, 1), 0.0, 255.0)
    rgb = np.where(hit[:, None], rgb, 0.0)
    dst = np.empty_like(rgb)
    for c in range(3):
        dst[:, c] = scale[c] * rgb[:, 2 - c if swap_rb else c] + shift[c]
    return dst, hit


def blocks(t):
    """[N,H,W,...] -> [N,H/2,W/2,4,...]: the four pixels of every chroma block"""
    N, H, W = t.shape[:3]
    t = t.reshape(N, H // 2, 2, W // 2, 2, *t.shape[3:])
    return np.moveaxis(t, 2, 3).reshape(N, H // 2, W // 2, 4, *t.shape[5:])


def paste_out(x, y, uv, sim, from_rgb, to_rgb, feather=0.0, value_range=(-1.0, 1.0), matte=None, colour=None, sums=True):
    """x fp32 [N,3,Hs,Ws]; y, uv uint8 planes.  -> dict: ``z_y`` fp64 [N,H,W] and ``z_uv`` fp64 [N,H/2,W/2,2], the value of every
    byte in front of the rounding (the background where nothing is pasted); ``region`` bool [N,H,W]; ``touched_uv`` bool
    [N,H/2,W/2], blocks with a region pixel; ``count`` int [N,H/2,W/2], region pixels per block; ``m`` fp64 [N,H,W] (0 outside the
    region); ``margin``, ``sums`` [N,13] (None without ``sums``), ``valid`` as ``blend_ref.blend``.  The sums do not depend on ``colour``."""
    F = np.asarray(from_rgb, dtype=np.float64)
    yb, uvb = np.asarray(y).astype(np.float64), np.asarray(uv).astype(np.float64)
    N, H, W = yb.shape
    zeros = np.zeros((N, H, W, 3))
    kw = dict(feather=feather, value_range=value_range, matte=matte)
    r0 = B.blend(x, zeros, sim, colour=colour, **kw)
    r1 = B.blend(x, zeros + 1.0, sim, colour=colour, **kw)
    region = r0["region"]
    mq = np.where(region[..., None], r0["z"], 0.0)                                       # m q'
    m = np.where(region, 1.0 + r0["z"][..., 0] - r1["z"][..., 0], 0.0)
    me = mq @ F[:, :3].T + m[..., None] * F[:, 3]                                        # m e: (y, u, v)
    z_y = np.where(region, np.clip((1.0 - m) * yb + me[..., 0], 0.0, 255.0), yb)
    S = 0.25 * blocks(m).sum(3)
    acc = 0.25 * blocks(me[..., 1:]).sum(3)
    count = blocks(region).sum(3)
    touched = count > 0
    z_uv = np.where(touched[..., None], np.clip((1.0 - S)[..., None] * uvb + acc, 0.0, 255.0), uvb)
    stats = B.blend(x, background(y, uv, to_rgb), sim, **kw)["sums"] if sums else None
    return dict(z_y=z_y, z_uv=z_uv, region=region, touched_uv=touched, count=count, m=m, margin=r0["margin"], sums=stats,
                valid=r0["valid"])
