"""The inputs of the I420 tests (tests/test_i420_cpu.py, tests/test_i420_align_gpu.py, tests/test_planar_table_kernels_gpu.py), built
on the CPU from tests/nv12_sim_cases.py and tests/surface_table_cases.py, which are imported and not edited: an I420 surface's U and
V planes are the de-interleaved UV plane of the existing case, so the NV12 case IS the interleave of the I420 one and the NV12
launchers on it are the reference, bit for bit.

A set of surfaces is a list of flat uint8 buffers (``flats``) and a ``Layout`` that says where every plane lies in them; the same
layout gives the views of the CPU buffers, of their copies on a device, and of a mask that says which bytes are no plane's (guards
and pitch padding, 0xA5: ``rest_intact``).  Every plane sits in an allocation of its own between at least 64 guard bytes -- except
the chroma planes of the one surface that shows V BEFORE U in memory, which share an allocation (guard, V, guard, U, guard): the
order of two allocations is the allocator's, and the order inside one is not.

While a case is built the host asserts what the GPU cases rely on: some surface has an odd W / 2 with an odd PACKED ``u_row_stride``
(the 32 x 46 region of ``surface_table_cases.LAYOUT``: chroma width 23 at pitch 23); some U plane starts at an odd offset of its
allocation (which is aligned to more than two bytes, so at an odd address); ``u_row_stride != v_row_stride`` for some surface; V lies
before U for some surface; there are chroma blocks with 1, 2, 3 and 4 region pixels (the region function of tests/nv12_sim_ref.py)."""
import functools

import numpy as np
import torch

import nv12_sim_cases as NS
import nv12_sim_ref as M
import surface_table_cases as SC

GUARD = 64


class Plane:
    """Where a plane of ``N`` frames of ``rows x width`` bytes lies: buffer ``buf``, first byte ``offset``, strides in bytes"""

    def __init__(self, buf, offset, rows, width, pitch, N=None, image_stride=0):
        self.buf, self.offset, self.rows, self.width, self.pitch, self.N, self.image_stride = buf, offset, rows, width, pitch, N, image_stride

    def view(self, flats):
        if self.N is None:
            return flats[self.buf].as_strided((self.rows, self.width), (self.pitch, 1), self.offset)
        return flats[self.buf].as_strided((self.N, self.rows, self.width), (self.image_stride, self.pitch, 1), self.offset)

    @property
    def end(self):
        return self.offset + ((self.N or 1) - 1) * self.image_stride + (self.rows - 1) * self.pitch + self.width


class Layout:
    """``surfaces``: per surface a triple of ``Plane`` (Y, U, V); ``sizes``: the buffers' lengths"""

    def __init__(self, surfaces):
        self.surfaces = surfaces
        ends = {}
        for planes in surfaces:
            for p in planes:
                ends[p.buf] = max(ends.get(p.buf, 0), p.end)
        self.sizes = [ends[b] + GUARD for b in range(len(ends))]
        for planes in surfaces:                                             # at least GUARD bytes in front of every plane
            assert all(p.offset >= GUARD for p in planes)

    def planes(self, flats, n):
        return tuple(p.view(flats) for p in self.surfaces[n])

    def fill(self, content):
        """``content``: per surface (y, u, v) CPU uint8 tensors -> flats, every other byte 0xA5"""
        flats = [torch.full((size,), 0xA5, dtype=torch.uint8) for size in self.sizes]
        for n, triple in enumerate(content):
            for view, plane in zip(self.planes(flats, n), triple):
                view.copy_(plane)
        return flats

    def rest_intact(self, flats, before):
        """Every byte that is no plane's is what it was in ``before`` (flats on any device)"""
        mask = [torch.ones(size, dtype=torch.bool) for size in self.sizes]
        for n in range(len(self.surfaces)):
            for view in self.planes(mask, n):
                view.fill_(False)
        return all(torch.equal(f[m.to(f.device)], b.to(f.device)[m.to(f.device)]) for f, b, m in zip(flats, before, mask))


def split(uv):
    """uv [..., W/2, 2] -> (u, v)"""
    return uv[..., 0], uv[..., 1]


def interleave(u, v):
    """(u, v) -> the UV plane of the NV12 surface with the same chroma: [..., W/2, 2], contiguous"""
    return torch.stack([u, v], -1).contiguous()


def counts_of(c, y, uv, rows, x):
    """The region pixels per chroma block of every frame (tests/nv12_sim_ref.py) -> the set of counts that occur"""
    to_rgb, from_rgb = NS.coeffs(c["colour"]["standard"], c["colour"]["full_range"])
    ok = torch.isfinite(rows).all(1)
    ref = M.paste_out(x[ok].numpy(), y[ok].numpy(), uv[ok].numpy(), rows[ok].numpy(), from_rgb, to_rgb, feather=c["feather"], sums=False)
    return set(np.unique(ref["count"]).tolist())


# ---- N surfaces of one size behind three pointers: the cases of tests/nv12_sim_cases.py -------------------------------------------
H, W, Y_PITCH, U_PITCH, V_PITCH = NS.H, NS.W, 64, 29, 32


def strided_layout(N):
    """Y at pitch 64; U at the odd pitch 29 from the odd offset 65, its frames an odd 583 bytes apart; V at pitch 32"""
    return Layout([(Plane(0, GUARD, H, W, Y_PITCH, N, H * Y_PITCH), Plane(1, GUARD + 1, H // 2, W // 2, U_PITCH, N, H // 2 * U_PITCH + 3),
                    Plane(2, GUARD, H // 2, W // 2, V_PITCH, N, H // 2 * V_PITCH))])


@functools.lru_cache(maxsize=None)
def case(name):
    """The case ``name`` of tests/nv12_sim_cases.py with its surfaces as I420: -> its dict plus ``u``, ``v`` [N,H/2,W/2] (CPU,
    contiguous), ``layout`` and ``flats`` (the pitched planes between guard bytes)"""
    c = dict(NS.case(name))
    c["u"], c["v"] = (t.contiguous() for t in split(c["uv"]))
    layout = strided_layout(c["y"].size(0))
    c["layout"], c["flats"] = layout, layout.fill([(c["y"], c["u"], c["v"])])
    y, u, v = layout.surfaces[0]
    assert u.offset % 2 == 1 and u.pitch % 2 == 1 and u.image_stride % 2 == 1 and u.pitch != v.pitch
    if name in NS.ROTATED:
        assert {1, 2, 3, 4} <= counts_of(c, c["y"], c["uv"], c["rows"], c["x"]), name
    return c


# ---- five surfaces of five sizes: the mixed table of tests/surface_table_cases.py --------------------------------------------------
SIZES = SC.SIZES
ROI, V_FIRST = 1, 2


def mixed_layout():
    """0: 40 x 56, Y pitch 64, U pitch 29 from an odd offset, V pitch 32.  1: the 32 x 46 region of interest at luma offset (4, 6)
    of a 40 x 60 surface: Y a view at pitch 60, U PACKED at the odd pitch 23, V a view at chroma offset (2, 3) of a 20 x 30 plane --
    an odd first byte.  2: 64 x 48, V FIRST and U behind it in one allocation.  3: the clipped 10 x 12, pitches 12 / 6 / 7.
    4: 2 x 2, the smallest, U at an odd offset."""
    s0 = (Plane(0, GUARD, 40, 56, 64), Plane(1, GUARD + 1, 20, 28, 29), Plane(2, GUARD, 20, 28, 32))
    s1 = (Plane(3, GUARD + 4 * 60 + 6, 32, 46, 60), Plane(4, GUARD, 16, 23, 23), Plane(5, GUARD + 2 * 30 + 3, 16, 23, 30))
    s2 = (Plane(6, GUARD, 64, 48, 48), Plane(7, GUARD + 32 * 24 + GUARD, 32, 24, 24), Plane(7, GUARD, 32, 24, 24))
    s3 = (Plane(8, GUARD, 10, 12, 12), Plane(9, GUARD, 5, 6, 6), Plane(10, GUARD, 5, 6, 7))
    s4 = (Plane(11, GUARD, 2, 2, 2), Plane(12, GUARD + 1, 1, 1, 1), Plane(13, GUARD, 1, 1, 1))
    return Layout([s0, s1, s2, s3, s4])


@functools.lru_cache(maxsize=None)
def mixed(name):
    """The case ``name`` of tests/surface_table_cases.py with its five surfaces as I420: -> its dict without the NV12 ``flats``, plus
    ``nv12``: per surface the CPU planes (y [h,w], uv [h/2,w/2,2]) of the NV12 case (contiguous copies), ``layout`` and ``flats``"""
    c = dict(SC.case(name))
    theirs = c.pop("flats")
    nv12 = [tuple(t.contiguous() for t in SC.planes_of(theirs[n], n)) for n in range(len(SC.LAYOUT))]
    layout = mixed_layout()
    c["nv12"], c["layout"] = nv12, layout
    c["flats"] = layout.fill([(y, *split(uv)) for y, uv in nv12])
    assert [tuple(layout.planes(c["flats"], n)[0].shape) for n in range(len(nv12))] == SIZES
    s = layout.surfaces
    assert SIZES[ROI][1] // 2 % 2 == 1 and s[ROI][1].pitch == SIZES[ROI][1] // 2 == 23           # an odd W / 2, packed: an odd pitch
    assert any(p[1].offset % 2 == 1 for p in s) and s[ROI][2].offset % 2 == 1                    # odd first bytes
    assert any(p[1].pitch != p[2].pitch for p in s)
    assert s[V_FIRST][1].buf == s[V_FIRST][2].buf and s[V_FIRST][2].offset < s[V_FIRST][1].offset  # V before U
    counts = set()
    for n, (y, uv) in enumerate(nv12):
        if bool(torch.isfinite(c["rows"][n]).all()):
            counts |= counts_of(c, y[None], uv[None], c["rows"][n:n + 1], c["x"][n:n + 1])
    assert {1, 2, 3, 4} <= counts, (name, counts)
    return c
