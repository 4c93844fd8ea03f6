"""GPU checks of the aligned NV12 edge over a surface table (csrc/frame_table_nv12.hip): ``ops.SurfaceTable`` through
``ops.frames_from_nv12_aligned``, ``ops.paste_colour_sums_nv12``, ``ops.paste_colour_match_nv12`` and ``ops.frames_paste_nv12_aligned``.
Every criterion is equality of bits or bytes with the strided NV12 launchers, which tests/test_nv12_align_gpu.py holds to the fp64
model of tests/nv12_sim_ref.py: a table over the frames of pitched surfaces gives what the surfaces give, and surface ``n`` of a table
of mixed sizes gives what the strided launcher gives at ``N = 1`` on that surface with row, matte and colour row ``n``.  Tables are
built from live tensors only.  Inputs: tests/nv12_sim_cases.py (40 x 56 surfaces at pitch 64 between 256 guard bytes) and
tests/surface_table_cases.py (five sizes, every plane an allocation of its own)."""
import importlib

import pytest
import torch

import nv12_sim_cases as NS
import surface_table_cases as SC

pytestmark = pytest.mark.gpu
ONE_SIZE = ["generic 601", "wide 709", "full range", "matte frames 709", "raw bytes", "invalid and zero"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


def on(dev, c):
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in c.items()}


def paste_variants(c, colour):
    """(name, matte, colour) of the four pastes: plain, matte only, colour only, both"""
    return [("plain", None, None), ("matte", c["matte"], None), ("colour", None, colour), ("both", c["matte"], colour)]


def surfaces_of(p):
    """The frames of a ``Pitched`` surface as what a table takes: a pair of plane views per frame"""
    return [(p.y[n], p.uv[n]) for n in range(p.y.size(0))]


@pytest.mark.parametrize("name", ONE_SIZE)
def test_a_table_over_pitched_surfaces_is_the_surfaces(pkg, dev, name):
    ops, c = pkg.ops, on(dev, NS.case(name))
    x, rows, kw, net = c["x"], c["rows"], c["colour"], c["net"]
    p = NS.Pitched(c["y"], c["uv"], dev)
    table = ops.SurfaceTable(surfaces_of(p))
    assert table.N == x.size(0) and table.sizes == [(NS.H, NS.W)] * table.N and table.dev.numel() == 40 * table.N
    keep = [t.clone() for t in p.raw]
    assert torch.equal(ops.frames_from_nv12_aligned(table, net, rows, **kw), ops.frames_from_nv12_aligned(p.planes, net, rows, **kw))
    assert torch.equal(ops.frames_from_nv12_aligned(table, net, rows, channel_order="bgr", **kw),
                       ops.frames_from_nv12_aligned(p.planes, net, rows, channel_order="bgr", **kw))
    stat = dict(matte=c["matte"], feather=c["feather"], **kw)
    assert torch.equal(ops.paste_colour_sums_nv12(x, table, rows, **stat), ops.paste_colour_sums_nv12(x, p.planes, rows, **stat))
    colour = ops.paste_colour_match_nv12(x, p.planes, rows, **stat)
    assert torch.equal(ops.paste_colour_match_nv12(x, table, rows, **stat), colour)
    assert all(torch.equal(a, b) for a, b in zip(p.raw, keep))              # the way in and the statistics only read
    for how, matte, col in paste_variants(c, colour):
        want = ops.nv12_planes(ops.frames_paste_nv12_aligned(x, p.planes, rows, feather=c["feather"], matte=matte, colour=col, **kw))
        q = NS.Pitched(c["y"], c["uv"], dev)
        into = ops.SurfaceTable(surfaces_of(q))
        got = ops.frames_paste_nv12_aligned(x, into, rows, feather=c["feather"], matte=matte, colour=col, **kw)
        assert got is into and torch.equal(q.y, want[0]) and torch.equal(q.uv, want[1]), how
        assert q.intact(), how
        if not torch.isfinite(rows).all():
            bad = int((~torch.isfinite(rows).all(1)).nonzero()[0])
            assert torch.equal(q.y[bad], p.y[bad]) and torch.equal(q.uv[bad], p.uv[bad])     # a NaN row with a usable entry: untouched, as ever
    assert not torch.equal(want[0], p.y) and not torch.equal(want[1], p.uv)
    # a table over one [N,3H/2,W] tensor, and over one pair of planes, gives views of their frames
    packed = torch.cat([c["y"], c["uv"].flatten(2)], 1)
    for whole in (packed, (c["y"], c["uv"])):
        assert torch.equal(ops.frames_from_nv12_aligned(ops.SurfaceTable(whole), net, rows, **kw), ops.frames_from_nv12_aligned(whole, net, rows, **kw))


@pytest.mark.parametrize("name", SC.MIXED)
def test_mixed_sizes_with_every_plane_its_own_allocation(pkg, dev, name):
    ops, c = pkg.ops, on(dev, SC.case(name))
    x, rows, kw, net = c["x"], c["rows"], c["colour"], c["net"]
    N = len(SC.LAYOUT)
    flats = [tuple(f.to(dev) for f in pair) for pair in c["flats"]]
    planes = [SC.planes_of(flats[n], n) for n in range(N)]
    assert planes[1][0].stride(0) == 60 and planes[1][1].stride(0) == 60 and planes[1][1].storage_offset() == SC.GUARD + 2 * 60 + 6
    assert [tuple(y.shape) for y, _ in planes] == SC.SIZES
    before = [tuple(f.clone() for f in pair) for pair in flats]
    table = ops.SurfaceTable(planes)
    assert table.sizes == SC.SIZES

    def matte_of(n):
        return None if c["matte"] is None else c["matte"] if c["matte"].dim() == 2 else c["matte"][n:n + 1]

    def one(n):                                                             # what the strided launchers take for surface n alone
        return x[n:n + 1], (planes[n][0].unsqueeze(0), planes[n][1].unsqueeze(0)), rows[n:n + 1]

    def unwritten():
        return all(torch.equal(a, b) for pair, kept in zip(flats, before) for a, b in zip(pair, kept))

    got = ops.frames_from_nv12_aligned(table, net, rows, **kw)
    for n in range(N):
        assert torch.equal(got[n:n + 1], ops.frames_from_nv12_aligned(one(n)[1], net, one(n)[2], **kw)), n
    stat = dict(feather=c["feather"], **kw)
    sums = ops.paste_colour_sums_nv12(x, table, rows, matte=c["matte"], **stat)
    colour = ops.paste_colour_match_nv12(x, table, rows, matte=c["matte"], **stat)
    for n in range(N):
        assert torch.equal(sums[n:n + 1], ops.paste_colour_sums_nv12(*one(n), matte=matte_of(n), **stat)), n
        assert torch.equal(colour[n:n + 1], ops.paste_colour_match_nv12(*one(n), matte=matte_of(n), **stat)), n
    assert all(float(sums[n, 0]) > 0 for n in c["pasted"])                   # the clipped and the smallest surface have region pixels
    assert unwritten()                                                      # nothing was written so far
    for how, matte, col in paste_variants(c, colour):
        for pair, kept in zip(flats, before):
            for a, b in zip(pair, kept):
                a.copy_(b)
        want = [ops.nv12_planes(ops.frames_paste_nv12_aligned(*one(n), feather=c["feather"], matte=None if matte is None else matte_of(n),
                                                              colour=None if col is None else col[n:n + 1], **kw)) for n in range(N)]
        assert unwritten()                                                  # (the strided launcher pasted into clones)
        assert ops.frames_paste_nv12_aligned(x, table, rows, feather=c["feather"], matte=matte, colour=col, **kw) is table
        for n in range(N):
            assert torch.equal(planes[n][0], want[n][0][0]) and torch.equal(planes[n][1], want[n][1][0]), (how, n)
            # every byte outside the surface's own pixels is as it was: pitch padding, the surroundings of the ROI, the guards
            rest = tuple(f.clone() for f in flats[n])
            for mine, kept in zip(SC.planes_of(rest, n), SC.planes_of(before[n], n)):
                mine.copy_(kept)
            assert torch.equal(rest[0], before[n][0]) and torch.equal(rest[1], before[n][1]), (how, n)
        for n in c["pasted"] if matte is None else ():                      # (a matte may be zero where it likes)
            assert not torch.equal(planes[n][0], SC.planes_of(before[n], n)[0]), (how, n)


def test_absent_and_invalid_surfaces(pkg, dev):
    ops, c = pkg.ops, on(dev, NS.case("invalid and zero"))
    x, rows, matte, kw = c["x"], c["rows"], c["matte"], c["colour"]
    p = NS.Pitched(c["y"], c["uv"], dev)
    N, bad, absent = x.size(0), 2, 0
    assert not torch.isfinite(rows[bad]).all() and torch.isfinite(rows[absent]).all()
    keep_y, keep_uv = p.y.clone(), p.uv.clone()
    table = ops.SurfaceTable([None if n == absent else s for n, s in enumerate(surfaces_of(p))])
    assert table.sizes[absent] == (0, 0) and table.planes[absent] is None and table.surfaces[absent] is None
    got = ops.frames_from_nv12_aligned(table, c["net"], rows, mean=0.5, std=0.5, **kw)
    want = ops.frames_from_nv12_aligned(p.planes, c["net"], rows, mean=0.5, std=0.5, **kw)
    assert bool((got[absent] == -1.0).all()) and bool((got[bad] == -1.0).all())       # shift = -mean / std
    sums, colour = ops.paste_colour_sums_nv12(x, table, rows, matte=matte, **kw), ops.paste_colour_match_nv12(x, table, rows, matte=matte, **kw)
    want_sums = ops.paste_colour_sums_nv12(x, p.planes, rows, matte=matte, **kw)
    want_colour = ops.paste_colour_match_nv12(x, p.planes, rows, matte=matte, **kw)
    one = torch.tensor([[1.0, 0.0]] * 3, device=dev)
    for n in (absent, bad):
        assert not sums[n].any() and torch.equal(colour[n], one), n
    assert want_sums[absent].any() and not torch.equal(want_colour[absent], one)      # the surface itself would have counted
    others = [n for n in range(N) if n != absent]
    assert torch.equal(got[others], want[others]) and torch.equal(sums[others], want_sums[others]) and torch.equal(colour[others], want_colour[others])
    pasted = ops.nv12_planes(ops.frames_paste_nv12_aligned(x, p.planes, rows, matte=matte, colour=want_colour, **kw))
    ops.frames_paste_nv12_aligned(x, table, rows, matte=matte, colour=colour, **kw)
    for n in (absent, bad):                                                 # no entry: nothing written; a NaN row: as ever
        assert torch.equal(p.y[n], keep_y[n]) and torch.equal(p.uv[n], keep_uv[n]), n
    assert torch.equal(p.y[others], pasted[0][others]) and torch.equal(p.uv[others], pasted[1][others])
    assert not torch.equal(p.y[3], keep_y[3]) and not torch.equal(p.uv[3], keep_uv[3]) and p.intact()
    # every surface absent: nothing is read and nothing is written
    nothing = ops.SurfaceTable([None] * N)
    assert bool((ops.frames_from_nv12_aligned(nothing, c["net"], rows, **kw) == -1.0).all())
    assert not ops.paste_colour_sums_nv12(x, nothing, rows, **kw).any()
    assert ops.frames_paste_nv12_aligned(x, nothing, rows, **kw) is nothing


def test_permuting_the_entries_permutes_the_results(pkg, dev):
    ops, c = pkg.ops, on(dev, NS.case("matte frames 709"))
    x, rows, matte, net = c["x"], c["rows"], c["matte"], c["net"]
    kw = dict(feather=c["feather"], **c["colour"])
    perm = [2, 0, 1]
    pa, pb = NS.Pitched(c["y"], c["uv"], dev), NS.Pitched(c["y"], c["uv"], dev)
    a, b = ops.SurfaceTable(surfaces_of(pa)), ops.SurfaceTable([surfaces_of(pb)[n] for n in perm])
    xp, rp, mp = x[perm].contiguous(), rows[perm].contiguous(), matte[perm].contiguous()
    assert torch.equal(ops.frames_from_nv12_aligned(b, net, rp, **c["colour"]), ops.frames_from_nv12_aligned(a, net, rows, **c["colour"])[perm])
    sums, colour = ops.paste_colour_sums_nv12(x, a, rows, matte=matte, **kw), ops.paste_colour_match_nv12(x, a, rows, matte=matte, **kw)
    assert torch.equal(ops.paste_colour_sums_nv12(xp, b, rp, matte=mp, **kw), sums[perm])
    assert torch.equal(ops.paste_colour_match_nv12(xp, b, rp, matte=mp, **kw), colour[perm])
    ops.frames_paste_nv12_aligned(x, a, rows, matte=matte, colour=colour, **kw)
    ops.frames_paste_nv12_aligned(xp, b, rp, matte=mp, colour=colour[perm].contiguous(), **kw)
    assert torch.equal(pb.y, pa.y) and torch.equal(pb.uv, pa.uv) and not torch.equal(pa.y[0], c["y"][0])     # b's entries were permuted, not its surfaces


def test_the_sums_of_a_table_are_deterministic(pkg, dev):
    ops, c = pkg.ops, on(dev, SC.case("matte frames 709"))
    flats = [tuple(f.to(dev) for f in pair) for pair in c["flats"]]
    table = ops.SurfaceTable([SC.planes_of(flats[n], n) for n in range(len(SC.LAYOUT))])
    kw = dict(matte=c["matte"], feather=c["feather"], **c["colour"])
    first = ops.paste_colour_sums_nv12(c["x"], table, c["rows"], **kw).clone()
    second = ops.paste_colour_sums_nv12(c["x"], table, c["rows"], **kw)
    assert first.any() and torch.equal(first.view(torch.int64), second.view(torch.int64))


def test_refusals_come_before_a_launch(pkg, dev):
    ops, L, c = pkg.ops, pkg._lib, on(dev, NS.case("generic 601"))
    x, rows, net = c["x"], c["rows"], c["net"]
    p = NS.Pitched(c["y"], c["uv"], dev)
    keep = [t.clone() for t in p.raw]
    table = ops.SurfaceTable(surfaces_of(p))
    # the table on another device than x
    for call in (lambda: ops.frames_paste_nv12_aligned(x.cpu(), table, rows), lambda: ops.paste_colour_sums_nv12(x.cpu(), table, rows),
                 lambda: ops.paste_colour_match_nv12(x.cpu(), table, rows)):
        with pytest.raises(L.SpkError, match="expected a HIP device tensor"):    # x is judged first; one GPU cannot show more
            call()
    # the paste is in place
    other = NS.Pitched(c["y"], c["uv"], dev)
    for out in (other.planes, ops.SurfaceTable(surfaces_of(other))):
        with pytest.raises(L.SpkError, match="in place"):
            ops.frames_paste_nv12_aligned(x, table, rows, out=out)
    # a count that differs from x's
    with pytest.raises(ValueError, match="4 generated frames, a table of 3"):
        ops.frames_paste_nv12_aligned(x, ops.SurfaceTable(surfaces_of(p)[:3]), rows)
    with pytest.raises(ValueError, match="4 generated frames, a table of 3"):
        ops.paste_colour_sums_nv12(x, ops.SurfaceTable(surfaces_of(p)[:3]), rows)
    with pytest.raises(ValueError):
        ops.frames_from_nv12_aligned(table, net, rows[:3])
    # overlapping planes: fine where the surfaces are read, refused where they are written -- two entries in one surface, and an
    # entry whose UV view lies in its own Y plane
    s = surfaces_of(p)
    inner = (p.y[1, 4:20, 6:30], p.uv[1, 2:10, 3:15])
    twice = ops.SurfaceTable([s[0], s[1], inner, s[3]])
    got = ops.frames_from_nv12_aligned(twice, net, rows)
    assert torch.equal(got[1], ops.frames_from_nv12_aligned((p.y[1:2], p.uv[1:2]), net, rows[1:2])[0])
    assert ops.paste_colour_sums_nv12(x, twice, rows).shape == (4, 13)
    # (both planes of entry 2 lie in entry 1's, and the check names the pair it meets first in address order: which of the two
    # allocations lies lower is the allocator's)
    with pytest.raises(L.SpkError, match=r"entries 1 \((Y|UV)\) and 2 \(\1\) overlap"):
        ops.frames_paste_nv12_aligned(x, twice, rows)
    # ... and with one plane of the inner entry in an allocation of its own, the plane that is left is the one that is named
    only_y = ops.SurfaceTable([s[0], s[1], (inner[0], inner[1].clone()), s[3]])
    with pytest.raises(L.SpkError, match=r"entries 1 \(Y\) and 2 \(Y\) overlap"):
        ops.frames_paste_nv12_aligned(x, only_y, rows)
    only_uv = ops.SurfaceTable([s[0], s[1], (inner[0].clone(), inner[1]), s[3]])
    with pytest.raises(L.SpkError, match=r"entries 1 \(UV\) and 2 \(UV\) overlap"):
        ops.frames_paste_nv12_aligned(x, only_uv, rows)
    own =ops.SurfaceTable([s[0], s[1], s[2], (p.y[3], p.y[3, 8:28, :56].unflatten(1, (28, 2)))])
    with pytest.raises(L.SpkError, match=r"entries 3 \(Y\) and 3 \(UV\) overlap"):
        ops.frames_paste_nv12_aligned(x, own, rows)
    assert all(torch.equal(a, b) for a, b in zip(p.raw, keep)) and other.intact()        # no refusal wrote a byte
    assert torch.equal(other.y, p.y) and torch.equal(other.uv, p.uv)
