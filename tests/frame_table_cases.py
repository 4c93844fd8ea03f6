"""The mixed-size inputs of tests/test_frame_table_kernels_gpu.py, built on the CPU so that the host can assert what the GPU case
relies on: five frames in five allocations -- 40 x 56; a 33 x 47 view at offset (3, 5) of a 40 x 60 buffer (pitch 180, not 3 W);
64 x 48; a 9 x 11 frame that the region box overhangs on all four sides; 1 x 1 -- each buffer with 64 guard bytes in front of it and
behind it.  The rows, generated images, mattes and the rest are those of a case of tests/blend_cases.py, taken cyclically for the
five frames, the rows re-centred on each frame."""
import functools

import numpy as np
import torch

import blend_cases as BC

GUARD = 64
# (buffer H, buffer W, view offset y, x, frame H, W)
LAYOUT = [(40, 56, 0, 0, 40, 56), (40, 60, 3, 5, 33, 47), (64, 48, 0, 0, 64, 48), (9, 11, 0, 0, 9, 11), (1, 1, 0, 0, 1, 1)]
SIZES = [(h, w) for *_, h, w in LAYOUT]
CLIPPED = 3                                                                 # the frame the region overhangs on all four sides


def buffers(seed):
    """-> the five flat uint8 buffers (guards included), random bytes"""
    return [BC.frames(seed + n, 2 * GUARD + bh * bw * 3) for n, (bh, bw, *_) in enumerate(LAYOUT)]


def frame_of(flat, n):
    """Frame ``n`` as a view of its flat buffer: [h, w, 3] with the buffer's pitch"""
    bh, bw, y0, x0, h, w = LAYOUT[n]
    return flat[GUARD:GUARD + bh * bw * 3].view(bh, bw, 3)[y0:y0 + h, x0:x0 + w]


def region_corners(row, net):
    a, c, tx, ty = (float(v) for v in row)
    Hs, Ws = net
    xs = [tx, a * Ws + tx, -c * Hs + tx, a * Ws - c * Hs + tx]
    ys = [ty, c * Ws + ty, a * Hs + ty, c * Ws + a * Hs + ty]
    return min(xs), max(xs), min(ys), max(ys)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(x [5,3,Hs,Ws], rows [5,4], matte (None, [Hs,Ws] or [5,Hs,Ws]), feather, bgr, net): CPU tensors.  Frame ``n`` takes
    the case's inputs ``n % N``; its row is moved so that the region sits on its own frame as it sat on the 40 x 56 one."""
    c = BC.case(name)
    N = c["x"].size(0)
    pick = [n % N for n in range(len(LAYOUT))]
    rows = c["rows"][pick].clone()
    for n, (h, w) in enumerate(SIZES):
        rows[n, 2] += (w - BC.W) / 2.0
        rows[n, 3] += (h - BC.H) / 2.0
    matte = c["matte"]
    if matte is not None and matte.dim() == 3:
        matte = matte[pick].contiguous()
    out = dict(x=c["x"][pick].contiguous(), rows=rows, matte=matte, feather=c["feather"], bgr=c["bgr"], net=c["net"])
    # the clipped branch has a frame that takes it: the region of the 9 x 11 frame is valid, reaches beyond all four edges of the
    # frame, so its bounding box is the whole frame -- non-empty, and cut on every side
    row = rows[CLIPPED].double().numpy()
    assert np.all(np.isfinite(row)), name
    x_lo, x_hi, y_lo, y_hi = region_corners(row, c["net"])
    h, w = SIZES[CLIPPED]
    assert x_lo < 0 and x_hi > w and y_lo < 0 and y_hi > h, (name, x_lo, x_hi, y_lo, y_hi)
    return out
