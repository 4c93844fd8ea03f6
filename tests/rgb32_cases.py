"""The inputs of the RGB32 tests (tests/test_rgb32_cpu.py, tests/test_rgb32_align_gpu.py, tests/test_rgb32_table_kernels_gpu.py),
built on the CPU from tests/blend_cases.py and tests/frame_table_cases.py, which are imported and not edited: an RGB32 frame holds the
case's three colour bytes, in their memory order, at the offset its channel order gives them (0 for ``rgba`` / ``bgra``, 1 for
``argb`` / ``abgr``) and a random fourth byte per pixel that is never 255, so the packed case IS the RGB32 one with the fourth byte
stripped and the rgb24 launchers on it (``channel_order`` ``rgb`` / ``bgr``) are the reference, bit for bit.

A set of frames is a flat uint8 buffer: 64 guard bytes, the frames at row pitch ``4 W + 16``, 64 guard bytes, every byte that is no
pixel's 0xA5.  ``Surface`` says where the pixels lie, gives the views of the CPU buffer and of its copy on a device, and answers what
the GPU cases ask: the colour bytes as a packed tensor, the fourth bytes, and whether every guard and pitch byte is what it was.
While a case is built the host asserts what the GPU cases rely on: no fourth byte is 255; the pitch and the first pixel are multiples
of 4; the region-of-interest view starts at an address that is 4-aligned and NOT 16-aligned (relative to its allocation, which an
allocator aligns to more than 16); the clipped frame of the mixed table still overhangs on all four sides (asserted by
``frame_table_cases.case``)."""
import functools

import torch

import blend_cases as BC
import frame_table_cases as FC

GUARD, PAD = 64, 0xA5
ORDERS = ("rgba", "bgra", "argb", "abgr")
NAMES = ["generic", "generic wide", "matte frames", "feather and matte", "invalid and zero", "gain cap"]
ROI = (40, 60, 3, 5, 33, 47)                                               # a 33 x 47 view at offset (3, 5) of a 40 x 60 surface


def colour_of(order):
    """-> (the rgb24 order of the colour bytes, the offset of the first of them in a pixel, the offset of the fourth byte)"""
    assert order in ORDERS
    first = 1 if order[0] == "a" else 0
    return order.replace("a", ""), first, 3 - 3 * first


def pitch_of(bw):
    return 4 * bw + 16


class Surface:
    """``N`` surfaces of ``bh x bw`` pixels in one flat buffer, of which the frames are the ``h x w`` views at pixel offset ``(y0, x0)``"""

    def __init__(self, N, bh, bw, y0=0, x0=0, h=None, w=None):
        self.N, self.bh, self.bw, self.y0, self.x0 = N, bh, bw, y0, x0
        self.h, self.w = bh if h is None else h, bw if w is None else w
        self.pitch = pitch_of(bw)
        self.size = 2 * GUARD + N * bh * self.pitch
        self.offset = GUARD + y0 * self.pitch + 4 * x0
        assert self.pitch % 4 == 0 and self.offset % 4 == 0

    def view(self, flat, whole=False):
        """The frames [N,h,w,4] (``whole``: the surfaces [N,bh,bw,4]) as a view of ``flat``, on any device"""
        if whole:
            return flat.as_strided((self.N, self.bh, self.bw, 4), (self.bh * self.pitch, self.pitch, 4, 1), GUARD)
        return flat.as_strided((self.N, self.h, self.w, 4), (self.bh * self.pitch, self.pitch, 4, 1), self.offset)

    def fill(self, colour, order, seed):
        """``colour``: uint8 [N,bh,bw,3], the colour bytes of the WHOLE surfaces in memory order -> the flat CPU buffer"""
        _, first, fourth = colour_of(order)
        flat = torch.full((self.size,), PAD, dtype=torch.uint8)
        px = self.view(flat, whole=True)
        px[..., first:first + 3] = colour
        px[..., fourth] = torch.randint(0, 255, (self.N, self.bh, self.bw), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
        assert int(px[..., fourth].max()) < 255
        return flat

    def rest_intact(self, flat, before):
        """Every byte that is no pixel's of the WHOLE surfaces -- guards and pitch padding -- is what it was in ``before``"""
        mask = torch.ones(self.size, dtype=torch.bool)
        self.view(mask, whole=True).fill_(False)
        mask = mask.to(flat.device)
        return torch.equal(flat[mask], before.to(flat.device)[mask])

    def outside_intact(self, flat, before):
        """Every byte that is not a pixel of the frames -- the surroundings of a region of interest included -- is what it was"""
        mask = torch.ones(self.size, dtype=torch.bool)
        self.view(mask).fill_(False)
        mask = mask.to(flat.device)
        return torch.equal(flat[mask], before.to(flat.device)[mask])


def packed(frames, order):
    """RGB32 frames [...,4] -> a contiguous packed copy of their colour bytes [...,3], in memory order"""
    _, first, _ = colour_of(order)
    return frames[..., first:first + 3].contiguous()


def fourth(frames, order):
    return frames[..., colour_of(order)[2]]


# ---- N frames of one size: the cases of tests/blend_cases.py ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name, order):
    """The case ``name`` of tests/blend_cases.py with its frames as RGB32 in ``order``: -> its dict plus ``surface``, ``flat`` and
    ``order``; ``bg`` stays the packed frames [N,40,56,3], which are the reference's input"""
    c = dict(BC.case(name))
    assert not c["bgr"]                                                     # the order is this file's to choose
    N = c["bg"].size(0)
    s = Surface(N, BC.H, BC.W)
    c["surface"], c["order"] = s, order
    c["flat"] = s.fill(c["bg"], order, 700 + ORDERS.index(order))
    assert s.pitch == 4 * BC.W + 16 and torch.equal(packed(s.view(c["flat"]), order), c["bg"])
    return c


@functools.lru_cache(maxsize=None)
def roi_case(order):
    """One 33 x 47 frame at offset (3, 5) of a 40 x 60 surface: the first frame of ``generic``, its row re-centred on the view"""
    c = BC.case("generic")
    bh, bw, y0, x0, h, w = ROI
    s = Surface(1, bh, bw, y0, x0, h, w)
    assert s.offset % 4 == 0 and s.offset % 16 != 0                         # 4-aligned, not 16-aligned
    rows = c["rows"][:1].clone()
    rows[0, 2] += (w - BC.W) / 2.0
    rows[0, 3] += (h - BC.H) / 2.0
    whole = BC.frames(811, 1, bh, bw, 3)
    flat = s.fill(whole, order, 750 + ORDERS.index(order))
    return dict(x=c["x"][:1].contiguous(), rows=rows, net=c["net"], surface=s, flat=flat, order=order,
                bg=whole[:, y0:y0 + h, x0:x0 + w].contiguous())


# ---- five frames of five sizes: the mixed table of tests/frame_table_cases.py -------------------------------------------------------
SIZES = FC.SIZES


@functools.lru_cache(maxsize=None)
def mixed(name, order):
    """The case ``name`` of tests/frame_table_cases.py (which asserts that the clipped frame overhangs on all four sides) with five
    RGB32 surfaces in five buffers: -> its dict plus ``surfaces`` (a ``Surface`` per frame, N = 1), ``flats``, ``bg`` (the packed
    frames [h,w,3] per frame) and ``order``"""
    c = dict(FC.case(name))
    theirs = FC.buffers(900 + sorted(BC.SPECS).index(name))
    surfaces, flats, bg = [], [], []
    for n, (bh, bw, y0, x0, h, w) in enumerate(FC.LAYOUT):
        s = Surface(1, bh, bw, y0, x0, h, w)
        whole = theirs[n][FC.GUARD:FC.GUARD + bh * bw * 3].view(1, bh, bw, 3)
        surfaces.append(s), flats.append(s.fill(whole, order, 950 + 10 * n + ORDERS.index(order)))
        bg.append(FC.frame_of(theirs[n], n).contiguous())
        assert torch.equal(packed(s.view(flats[n])[0], order), bg[n])
    assert [tuple(b.shape[:2]) for b in bg] == SIZES
    assert surfaces[1].offset % 16 != 0 and surfaces[1].pitch != 4 * SIZES[1][1]
    c["surfaces"], c["flats"], c["bg"], c["order"] = surfaces, flats, bg, order
    return c
