"""The mixed-size inputs of tests/test_surface_table_kernels_gpu.py, built on the CPU so that the host can assert what the GPU case
relies on: five NV12 surfaces, each PLANE in an allocation of its own between 64 guard bytes of 0xA5 -- 40 x 56 at pitch 64; a
32 x 46 region of interest at luma offset (4, 6) of a 40 x 60 surface (the Y view has pitch 60, the UV view starts at chroma row 2,
byte 6, pitch 60); 64 x 48; a 10 x 12 surface that the region overhangs on all four sides; 2 x 2, the smallest surface there is.
The rows, generated images, mattes and the colour are those of a case of tests/nv12_sim_cases.py, taken cyclically for the five
surfaces, the rows re-centred on each surface.  While a case is built the region function of tests/nv12_sim_ref.py says, on the host,
that the 10 x 12 surface is clipped on four sides, that some surface's region box begins at an odd x and an odd y, that some surface has
chroma blocks with 1, 2, 3 and 4 region pixels, and that every surface meant to be pasted has a region."""
import functools

import numpy as np
import torch

import nv12_sim_cases as NS
import nv12_sim_ref as M

GUARD = 64
# (buffer H, buffer W, pitch, view offset y, x, surface H, W)
LAYOUT = [(40, 56, 64, 0, 0, 40, 56), (40, 60, 60, 4, 6, 32, 46), (64, 48, 48, 0, 0, 64, 48), (10, 12, 12, 0, 0, 10, 12), (2, 2, 2, 0, 0, 2, 2)]
SIZES = [(h, w) for *_, h, w in LAYOUT]
CLIPPED, SMALLEST = 3, 4
MIXED = ["generic 601", "wide 709", "matte frames 709", "invalid and zero"]


def buffers(seed, colour):
    """-> per surface the two flat uint8 buffers (Y, UV), guards and pitch padding 0xA5, the surface's bytes from random RGB"""
    out = []
    for n, (bh, bw, pitch, *_) in enumerate(LAYOUT):
        y, uv = NS.surface_from_rgb(seed + n, 1, bh, bw, **colour)
        flats = []
        for plane, rows in ((y[0], bh), (uv[0].reshape(bh // 2, bw), bh // 2)):
            flat = torch.full((2 * GUARD + rows * pitch,), 0xA5, dtype=torch.uint8)
            flat[GUARD:GUARD + rows * pitch].view(rows, pitch)[:, :bw] = plane
            flats.append(flat)
        out.append(tuple(flats))
    return out


def planes_of(flats, n):
    """Surface ``n`` as views of its two flat buffers: (y [h,w], uv [h/2,w/2,2]) with the buffer's pitch"""
    bh, bw, pitch, y0, x0, h, w = LAYOUT[n]
    y = flats[0][GUARD:GUARD + bh * pitch].view(bh, pitch)[y0:y0 + h, x0:x0 + w]
    uv = flats[1][GUARD:GUARD + bh // 2 * pitch].view(bh // 2, pitch)[y0 // 2:(y0 + h) // 2, x0:x0 + w].unflatten(1, (w // 2, 2))
    return y, uv


def box_of(region):
    """The bounding box of a region mask [H,W] -> (x_lo, x_hi, y_lo, y_hi), or None when it is empty"""
    ys, xs = np.nonzero(region)
    return None if ys.size == 0 else (int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max()))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(x [5,3,Hs,Ws], rows [5,4], matte (None, [Hs,Ws] or [5,Hs,Ws]), feather, net, colour, flats, pasted): CPU tensors.  Surface
    ``n`` takes the case's inputs ``n % N``; its row is moved so that the region sits on its own surface as it sat on the 40 x 56 one.
    ``pasted``: the surfaces with a valid row and a matte that is not all zero."""
    c = NS.case(name)
    N = c["x"].size(0)
    pick = [n % N for n in range(len(LAYOUT))]
    rows = c["rows"][pick].clone()
    for n, (h, w) in enumerate(SIZES):
        rows[n, 2] += (w - NS.W) / 2.0
        rows[n, 3] += (h - NS.H) / 2.0
    rows[0, 3] += 1.0                                                       # one pixel down: where its box began at an odd x, it now begins at an odd y too
    matte = c["matte"]
    if matte is not None and matte.dim() == 3:
        matte = matte[pick].contiguous()
    x = c["x"][pick].contiguous()
    flats = buffers(500, c["colour"])
    pasted = [n for n in range(len(LAYOUT)) if bool(torch.isfinite(rows[n]).all()) and
              (matte is None or bool((matte if matte.dim() == 2 else matte[n]).any()))]
    # ---- what the GPU case relies on, asserted on the host with the model's region
    to_rgb, from_rgb = NS.coeffs(c["colour"]["standard"], c["colour"]["full_range"])
    boxes, counts = {}, {}
    for n in range(len(LAYOUT)):
        if not bool(torch.isfinite(rows[n]).all()):
            continue
        y, uv = planes_of(flats[n], n)
        ref = M.paste_out(x[n:n + 1].numpy(), y.unsqueeze(0).numpy(), uv.unsqueeze(0).numpy(), rows[n:n + 1].numpy(), from_rgb, to_rgb,
                          feather=c["feather"], sums=False)
        boxes[n], counts[n] = box_of(ref["region"][0]), set(np.unique(ref["count"][0]).tolist())
    assert all(boxes.get(n) is not None for n in pasted), (name, boxes)                     # every surface that is pasted has a region
    h, w = SIZES[CLIPPED]
    assert CLIPPED in boxes and boxes[CLIPPED] == (0, w - 1, 0, h - 1), (name, boxes.get(CLIPPED))       # the whole surface: cut on four sides
    a, cc, tx, ty = (float(v) for v in rows[CLIPPED])
    xs = [tx, a * c["net"][1] + tx, -cc * c["net"][0] + tx, a * c["net"][1] - cc * c["net"][0] + tx]
    ys = [ty, cc * c["net"][1] + ty, a * c["net"][0] + ty, cc * c["net"][1] + a * c["net"][0] + ty]
    assert min(xs) < 0 and max(xs) > w and min(ys) < 0 and max(ys) > h, (name, xs, ys)
    assert any(b is not None and b[0] % 2 == 1 and b[2] % 2 == 1 for b in boxes.values()), (name, boxes)    # an odd x_lo and an odd y_lo
    assert any({1, 2, 3, 4} <= k for k in counts.values()), (name, counts)                  # blocks with 1, 2, 3 and 4 region pixels
    return dict(x=x, rows=rows, matte=matte, feather=c["feather"], net=c["net"], colour=c["colour"], flats=flats, pasted=pasted)
