"""fp64 CPU references of the NV12 video edge (csrc/frame_nv12.hip), written from the definitions in include/spk.h with dense
copies of ``ops.resize_tables`` and the fp32 ramps of ``ops.feather_tables``.  Used by tests/test_nv12_cpu.py (which checks this
file against a brute-force loop per pixel) and tests/test_nv12_gpu.py."""
import torch

F64 = torch.float64


def dense(ops, n_in, n_out):
    """One axis of the resize as a dense fp64 matrix [n_out, n_in]."""
    first, count, w = ops.resize_tables(n_in, n_out)
    M = torch.zeros(n_out, n_in, dtype=F64)
    for o in range(n_out):
        f, c = int(first[o]), int(count[o])
        M[o, f:f + c] = w[o, :c]
    return M


def fields(y, uv):
    """The three component fields at luma resolution: chroma sited by replication.  -> fp64 [N,3,H,W]."""
    c = uv.to(F64).repeat_interleave(2, 1).repeat_interleave(2, 2)
    return torch.stack([y.to(F64), c[..., 0], c[..., 1]], 1)


def affine(M, p):
    """A 3 x 4 map in byte units applied to the three planes of ``p`` [..., 3, h, w]."""
    return torch.einsum("cj,...jhw->...chw", M[:, :3], p) + M[:, 3].view(3, 1, 1)


def from_nv12_ref(ops, y, uv, boxes, h, w, size, to_rgb, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), bgr=False):
    """``ops.frames_from_nv12`` in fp64: ``boxes`` one in-frame ``(y0, x0)`` per frame.  -> fp64 [N,3,Hout,Wout]."""
    Hout, Wout = (size, size) if isinstance(size, int) else size
    My, Mx = dense(ops, h, Hout), dense(ops, w, Wout)
    f = fields(y, uv)
    box = torch.stack([f[n, :, y0:y0 + h, x0:x0 + w] for n, (y0, x0) in enumerate(boxes)])
    yuv = My @ box @ Mx.T
    rgb = affine(to_rgb, yuv).clamp(0, 255)
    m, s = torch.tensor(mean, dtype=F64).view(1, 3, 1, 1), torch.tensor(std, dtype=F64).view(1, 3, 1, 1)
    out = (rgb / 255 - m) / s
    return out.flip(1) if bgr else out


def paste_nv12_ref(ops, x, y, uv, boxes, h, w, from_rgb, feather=0, rng=(-1, 1)):
    """``ops.frames_paste_nv12`` in fp64, before the final rounding: the value of every byte of both planes (the background where
    nothing is pasted).  ``boxes``: one ``(y0, x0)`` per frame, clipped to the frame.  -> fp64 ``(val_y [N,H,W], val_uv [N,H/2,W/2,2])``."""
    lo, hi = rng
    N, _, Hs, Ws = x.shape
    H, W = y.shape[1:]
    v = x.to(F64)
    if (Hs, Ws) != (h, w):                      # (the tables of an equal size are the identity: a NaN stays in its pixel)
        v = dense(ops, Hs, h) @ v @ dense(ops, Ws, w).T
    q = ((v - lo) * (255.0 / (hi - lo))).clamp(0, 255)
    q = torch.where(torch.isnan(q), torch.zeros_like(q), q)
    e = affine(from_rgb, q)
    m = ops.feather_tables(h, feather).to(F64).view(h, 1) * ops.feather_tables(w, feather).to(F64).view(1, w)
    val_y, val_uv = y.to(F64).clone(), uv.to(F64).clone()
    for n, (y0, x0) in enumerate(boxes):
        ya, yb, xa, xb = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
        if ya >= yb or xa >= xb:
            continue
        Mf, Ef = torch.zeros(H, W, dtype=F64), torch.zeros(3, H, W, dtype=F64)
        Mf[ya:yb, xa:xb] = m[ya - y0:yb - y0, xa - x0:xb - x0]
        Ef[:, ya:yb, xa:xb] = e[n, :, ya - y0:yb - y0, xa - x0:xb - x0]
        val_y[n] = ((1 - Mf) * val_y[n] + Mf * Ef[0]).clamp(0, 255)
        blocks = lambda t: t.view(*t.shape[:-2], H // 2, 2, W // 2, 2)
        S = 0.25 * blocks(Mf).sum((-3, -1))
        acc = 0.25 * blocks(Mf * Ef[1:]).sum((-3, -1))                  # [2, H/2, W/2]
        val_uv[n] = ((1 - S).unsqueeze(-1) * val_uv[n] + acc.permute(1, 2, 0)).clamp(0, 255)
    return val_y, val_uv


def to_nv12_ref(ops, x, from_rgb, rng=(-1, 1)):
    """``ops.frames_to_nv12`` in fp64 before the rounding: Y = clamp(e_y), C = clamp(mean of the block's four e_c)."""
    N, _, H, W = x.shape
    zy, zuv = torch.zeros(N, H, W, dtype=torch.uint8), torch.zeros(N, H // 2, W // 2, 2, dtype=torch.uint8)
    return paste_nv12_ref(ops, x, zy, zuv, [(0, 0)] * N, H, W, from_rgb, 0, rng)
