"""GPU checks of the aligned I420 edge over a planar table (csrc/frame_table_i420.hip): ``ops.PlanarTable`` through
``ops.frames_from_i420_aligned``, ``ops.paste_colour_sums_i420``, ``ops.paste_colour_match_i420`` and ``ops.frames_paste_i420_aligned``.
Every criterion is equality of bits or bytes: entry ``n`` of a table of mixed sizes gives what the strided I420 launcher gives at
``N = 1`` on that surface with row, matte and colour row ``n``, and what the NV12 table launcher gives on the interleaved surfaces.
Inputs: tests/i420_cases.py over tests/surface_table_cases.py -- five sizes, an odd packed chroma pitch, odd chroma addresses, pitches
that differ, V before U -- every byte that is no plane's checked after every paste."""
import importlib

import pytest
import torch

import i420_cases as IC
import nv12_sim_cases as NS
import surface_table_cases as SC

pytestmark = pytest.mark.gpu
N = len(SC.LAYOUT)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


class On:
    """A mixed case on the device: ``planes[n]`` the I420 views of surface ``n``, ``nv12[n]`` the NV12 planes they de-interleave"""

    def __init__(self, c, dev):
        self.c, self.layout = c, c["layout"]
        self.flats = [f.to(dev) for f in c["flats"]]
        self.planes = [self.layout.planes(self.flats, n) for n in range(N)]
        self.nv12 = [(y.to(dev), uv.to(dev)) for y, uv in c["nv12"]]
        self.x, self.rows = c["x"].to(dev), c["rows"].to(dev)
        self.matte = None if c["matte"] is None else c["matte"].to(dev)
        self.colour, self.net, self.feather = c["colour"], c["net"], c["feather"]

    def matte_of(self, n, matte):
        return None if matte is None else matte if matte.dim() == 2 else matte[n:n + 1]

    def one(self, n):                                                       # what the strided launchers take for surface n alone
        return self.x[n:n + 1], tuple(p.unsqueeze(0) for p in self.planes[n]), self.rows[n:n + 1]

    def intact(self):
        return self.layout.rest_intact(self.flats, self.c["flats"])

    def unwritten(self):
        return all(torch.equal(a.cpu(), b) for a, b in zip(self.flats, self.c["flats"]))


@pytest.mark.parametrize("name", SC.MIXED)
def test_mixed_sizes_entry_by_entry(pkg, dev, name):
    ops, s = pkg.ops, On(IC.mixed(name), dev)
    x, rows, kw, net = s.x, s.rows, s.colour, s.net
    y1, u1, v1 = s.planes[IC.ROI]
    assert u1.stride(0) == 23 and v1.data_ptr() % 2 == 1 and s.planes[0][1].data_ptr() % 2 == 1 and y1.stride(0) == 60
    vf = s.planes[IC.V_FIRST]
    assert vf[2].data_ptr() < vf[1].data_ptr()                             # V before U in memory
    table, theirs = ops.PlanarTable(s.planes), ops.SurfaceTable(s.nv12)
    assert table.N == N and table.sizes == SC.SIZES and table.dev.numel() == 56 * N
    got = ops.frames_from_i420_aligned(table, net, rows, **kw)
    assert torch.equal(got, ops.frames_from_nv12_aligned(theirs, net, rows, **kw))
    assert torch.equal(ops.frames_from_i420_aligned(table, net, rows, channel_order="bgr", **kw), got.flip(1))
    for n in range(N):
        assert torch.equal(got[n:n + 1], ops.frames_from_i420_aligned(s.one(n)[1], net, s.one(n)[2], **kw)), n
    stat = dict(feather=s.feather, **kw)
    sums = ops.paste_colour_sums_i420(x, table, rows, matte=s.matte, **stat)
    colour = ops.paste_colour_match_i420(x, table, rows, matte=s.matte, **stat)
    assert torch.equal(sums.view(torch.int64), ops.paste_colour_sums_nv12(x, theirs, rows, matte=s.matte, **stat).view(torch.int64))
    assert torch.equal(colour.view(torch.int32), ops.paste_colour_match_nv12(x, theirs, rows, matte=s.matte, **stat).view(torch.int32))
    for n in range(N):
        assert torch.equal(sums[n:n + 1], ops.paste_colour_sums_i420(*s.one(n), matte=s.matte_of(n, s.matte), **stat)), n
        assert torch.equal(colour[n:n + 1], ops.paste_colour_match_i420(*s.one(n), matte=s.matte_of(n, s.matte), **stat)), n
    assert all(float(sums[n, 0]) > 0 for n in s.c["pasted"])                 # the clipped and the smallest surface have region pixels
    assert s.unwritten()                                                    # nothing was written so far
    for how, matte, col in (("plain", None, None), ("matte", s.matte, None), ("colour", None, colour), ("both", s.matte, colour)):
        pkw = dict(feather=s.feather, **kw)
        t = On(s.c, dev)
        strided = [ops.i420_planes(ops.frames_paste_i420_aligned(*t.one(n), matte=t.matte_of(n, matte), colour=None if col is None else col[n:n + 1],
                                                                 **pkw)) for n in range(N)]
        assert t.unwritten()                                                # (the strided launcher pasted into clones)
        nv = On(s.c, dev)
        into = ops.SurfaceTable(nv.nv12)
        ops.frames_paste_nv12_aligned(x, into, rows, matte=matte, colour=col, **pkw)
        mine = ops.PlanarTable(t.planes)
        assert ops.frames_paste_i420_aligned(x, mine, rows, matte=matte, colour=col, **pkw) is mine
        for n in range(N):
            y, u, v = t.planes[n]
            assert torch.equal(y, strided[n][0][0]) and torch.equal(u, strided[n][1][0]) and torch.equal(v, strided[n][2][0]), (how, n)
            assert torch.equal(y, nv.nv12[n][0]) and torch.equal(IC.interleave(u, v), nv.nv12[n][1]), (how, n)
        assert t.intact(), how                                              # pitch padding, the surroundings of the ROI, the guards
        for n in s.c["pasted"] if matte is None else ():                    # (a matte may be zero where it likes)
            assert not torch.equal(t.planes[n][0].cpu(), s.c["nv12"][n][0]), (how, n)


def test_an_absent_entry_behaves_as_an_invalid_row(pkg, dev):
    ops, s = pkg.ops, On(IC.mixed("invalid and zero"), dev)
    x, rows, matte, kw = s.x, s.rows, s.matte, s.colour
    bad = int((~torch.isfinite(rows).all(1)).nonzero()[0])
    absent = 0
    assert bad != absent
    table, whole = ops.PlanarTable([None if n == absent else p for n, p in enumerate(s.planes)]), ops.PlanarTable(s.planes)
    assert table.sizes[absent] == (0, 0) and table.planes[absent] is None and table.surfaces[absent] is None
    got, want = ops.frames_from_i420_aligned(table, s.net, rows, **kw), ops.frames_from_i420_aligned(whole, s.net, rows, **kw)
    assert bool((got[absent] == -1.0).all()) and bool((got[bad] == -1.0).all())       # shift = -mean / std
    sums, colour = ops.paste_colour_sums_i420(x, table, rows, matte=matte, **kw), ops.paste_colour_match_i420(x, table, rows, matte=matte, **kw)
    want_sums, want_colour = ops.paste_colour_sums_i420(x, whole, rows, matte=matte, **kw), ops.paste_colour_match_i420(x, whole, rows, matte=matte, **kw)
    one = torch.tensor([[1.0, 0.0]] * 3, device=dev)
    for n in (absent, bad):
        assert not sums[n].any() and torch.equal(colour[n], one), n
    assert want_sums[absent].any()                                          # the surface itself would have counted
    others = [n for n in range(N) if n != absent]
    assert torch.equal(got[others], want[others]) and torch.equal(sums[others], want_sums[others]) and torch.equal(colour[others], want_colour[others])
    t = On(s.c, dev)
    ops.frames_paste_i420_aligned(x, ops.PlanarTable(t.planes), rows, matte=matte, colour=want_colour, **kw)
    ops.frames_paste_i420_aligned(x, table, rows, matte=matte, colour=colour, **kw)
    for n in (absent, bad):                                                 # no entry: nothing written; a NaN row: as ever
        assert all(torch.equal(p.cpu(), q) for p, q in zip(s.planes[n], s.c["layout"].planes(s.c["flats"], n))), n
    for n in others:
        assert all(torch.equal(p, q) for p, q in zip(s.planes[n], t.planes[n])), n
    assert s.intact() and not s.unwritten()
    # every surface absent: nothing is read and nothing is written
    nothing = ops.PlanarTable([None] * N)
    assert bool((ops.frames_from_i420_aligned(nothing, s.net, rows, **kw) == -1.0).all())
    assert not ops.paste_colour_sums_i420(x, nothing, rows, **kw).any()
    assert ops.frames_paste_i420_aligned(x, nothing, rows, **kw) is nothing


def test_a_table_over_one_tensor_and_clone_planar(pkg, dev):
    """A table over one packed tensor or one triple of planes gives views of their frames; ``clone_planar`` packs every surface"""
    ops, c = pkg.ops, IC.case("matte frames 709")
    rows, net, kw = c["rows"].to(dev), c["net"], c["colour"]
    apart = (c["y"].to(dev), c["u"].to(dev), c["v"].to(dev))
    packed = torch.cat([t.flatten(1) for t in apart], 1).view(-1, 3 * IC.H // 2, IC.W)
    want = ops.frames_from_i420_aligned(apart, net, rows, **kw)
    for whole in (packed, apart):
        assert torch.equal(ops.frames_from_i420_aligned(ops.PlanarTable(whole), net, rows, **kw), want)
    s = On(IC.mixed("generic 601"), dev)
    table = ops.PlanarTable(s.planes)
    clone = ops.clone_planar(table)
    assert clone.sizes == table.sizes and all(t.is_contiguous() and tuple(t.shape) == (3 * h // 2, w) for t, (h, w) in zip(clone.surfaces, clone.sizes))
    assert all(torch.equal(a, b) for p, q in zip(clone.planes, table.planes) for a, b in zip(p, q))
    assert torch.equal(ops.clone_planar(apart), packed)
    x = s.x
    ops.frames_paste_i420_aligned(x, clone, s.rows, **s.colour)
    assert s.unwritten()                                                    # the clones were written, the table's surfaces were not


def test_refusals_come_before_a_launch(pkg, dev):
    ops, L = pkg.ops, pkg._lib
    s = On(IC.mixed("generic 601"), dev)
    table = ops.PlanarTable(s.planes)
    other = On(s.c, dev)
    for out in (other.planes[0], ops.PlanarTable(other.planes)):
        with pytest.raises(L.SpkError, match="in place"):
            ops.frames_paste_i420_aligned(s.x, table, s.rows, out=out)
    with pytest.raises(ValueError, match="5 generated frames, a table of 3"):
        ops.frames_paste_i420_aligned(s.x, ops.PlanarTable(s.planes[:3]), s.rows)
    with pytest.raises(ValueError):
        ops.frames_from_i420_aligned(table, s.net, s.rows[:3])
    # overlapping planes: fine where the surfaces are read, refused where they are written.  Chroma halves side by side on one pitch
    # share no byte, and their RANGES do
    y0, u0, v0 = s.planes[0]
    side = torch.zeros(20, 56, dtype=torch.uint8, device=dev)
    halves = ops.PlanarTable([(y0, side[:, :28], side[:, 28:])] + s.planes[1:])
    assert ops.frames_from_i420_aligned(halves, s.net, s.rows, **s.colour).shape[0] == N
    with pytest.raises(L.SpkError, match=r"entries 0 \(U\) and 0 \(V\) overlap"):
        ops.frames_paste_i420_aligned(s.x, halves, s.rows, **s.colour)
    fresh = (torch.zeros(40, 56, dtype=torch.uint8, device=dev), u0, torch.zeros(20, 28, dtype=torch.uint8, device=dev))
    twice = ops.PlanarTable([s.planes[0], s.planes[1], fresh] + s.planes[3:])               # the U plane of entry 0 once more
    with pytest.raises(L.SpkError, match=r"entries 0 \(U\) and 2 \(U\) overlap"):
        ops.frames_paste_i420_aligned(s.x, twice, s.rows, **s.colour)
    torch.cuda.synchronize()
    assert s.unwritten() and other.unwritten()                              # no refusal wrote a byte
