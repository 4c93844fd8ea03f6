"""GPU checks of the aligned edge over a frame table (csrc/frame_table.hip): ``ops.FrameTable`` through ``ops.frames_from_u8_aligned``,
``ops.paste_colour_sums``, ``ops.paste_colour_match`` and ``ops.frames_paste_u8_aligned``.  Every criterion is equality of bits or
bytes with the strided launchers: a table over the frames of one tensor gives what the tensor gives, and frame ``n`` of a table of
mixed sizes gives what the strided launcher gives at ``N = 1`` on that frame with row, matte and colour row ``n``.  Tables are built
from live tensors only.  Inputs: tests/blend_cases.py (40 x 56 frames, 16^2 / 12 x 20 generated images) and
tests/frame_table_cases.py (five sizes in five allocations)."""
import importlib

import pytest
import torch

import blend_cases as BC
import frame_table_cases as FC

pytestmark = pytest.mark.gpu
ONE_SIZE = ["generic", "bgr", "feather and matte", "matte frames", "invalid and zero", "strided"]
MIXED = ["generic", "bgr", "matte frames", "invalid and zero"]


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


def order(c):
    return dict(channel_order="bgr" if c["bgr"] else "rgb")


def paste_variants(c, colour):
    """(name, matte, colour) of the four pastes: plain, matte only, colour only, both"""
    return [("plain", None, None), ("matte", c["matte"], None), ("colour", None, colour), ("both", c["matte"], colour)]


@pytest.mark.parametrize("name", ONE_SIZE)
def test_a_table_over_one_tensor_is_the_tensor(pkg, dev, name):
    ops, c = pkg.ops, on(dev, BC.case(name))
    x, bg, rows, kw = c["x"], c["bg"], c["rows"], order(c)
    if name == "strided":                                                   # a strided background at an odd address, read in place
        big = BC.frames(77, x.size(0), BC.H + 9, BC.W + 13, 3).to(dev)
        big[:, 4:4 + BC.H, 5:5 + BC.W] = bg
        bg = big[:, 4:4 + BC.H, 5:5 + BC.W]
        assert not bg.is_contiguous() and bg.data_ptr() % 2 == 1
    table = ops.FrameTable(bg)
    assert table.N == x.size(0) and table.sizes == [(BC.H, BC.W)] * table.N and table.dev.numel() == 24 * table.N
    keep = bg.clone()
    assert torch.equal(ops.frames_from_u8_aligned(table, c["net"], rows, **kw), ops.frames_from_u8_aligned(bg, c["net"], rows, **kw))
    stat = dict(matte=c["matte"], feather=c["feather"], **kw)
    assert torch.equal(ops.paste_colour_sums(x, table, rows, **stat), ops.paste_colour_sums(x, bg, rows, **stat))
    colour = ops.paste_colour_match(x, bg, rows, **stat)
    assert torch.equal(ops.paste_colour_match(x, table, rows, **stat), colour)
    assert torch.equal(bg, keep)                                            # the way in and the statistics only read
    for how, matte, col in paste_variants(c, colour):
        want = ops.frames_paste_u8_aligned(x, bg, rows, feather=c["feather"], matte=matte, colour=col, **kw)
        into = ops.FrameTable(bg.clone())
        got = ops.frames_paste_u8_aligned(x, into, rows, feather=c["feather"], matte=matte, colour=col, **kw)
        assert got is into and torch.equal(torch.stack(into.frames), want), how
        if not torch.isfinite(rows).all():
            bad = int((~torch.isfinite(rows).all(1)).nonzero()[0])
            assert torch.equal(into.frames[bad], keep[bad])                 # a NaN row with a usable entry: untouched, as ever
    assert not torch.equal(want, keep)


@pytest.mark.parametrize("name", MIXED)
def test_mixed_sizes_in_separate_allocations(pkg, dev, name):
    ops, c = pkg.ops, on(dev, FC.case(name))
    x, rows, kw, net = c["x"], c["rows"], order(c), c["net"]
    N = len(FC.LAYOUT)
    flats = [f.to(dev) for f in FC.buffers(300)]
    frames = [FC.frame_of(flat, n) for n, flat in enumerate(flats)]
    assert frames[1].stride(0) == 180 != 3 * frames[1].size(1) and [tuple(f.shape[:2]) for f in frames] == FC.SIZES
    before = [flat.clone() for flat in flats]
    table = ops.FrameTable(frames)
    assert table.sizes == FC.SIZES

    def matte_of(n):
        return None if c["matte"] is None else c["matte"] if c["matte"].dim() == 2 else c["matte"][n:n + 1]

    def one(n):                                                             # what the strided launchers take for frame n alone
        return x[n:n + 1], frames[n].unsqueeze(0), rows[n:n + 1]

    got = ops.frames_from_u8_aligned(table, net, rows, **kw)
    for n in range(N):
        assert torch.equal(got[n:n + 1], ops.frames_from_u8_aligned(one(n)[1], net, one(n)[2], **kw)), n
    stat = dict(feather=c["feather"], **kw)
    sums = ops.paste_colour_sums(x, table, rows, matte=c["matte"], **stat)
    colour = ops.paste_colour_match(x, table, rows, matte=c["matte"], **stat)
    for n in range(N):
        assert torch.equal(sums[n:n + 1], ops.paste_colour_sums(*one(n), matte=matte_of(n), **stat)), n
        assert torch.equal(colour[n:n + 1], ops.paste_colour_match(*one(n), matte=matte_of(n), **stat)), n
    if torch.isfinite(rows[FC.CLIPPED]).all():
        assert float(sums[FC.CLIPPED, 0]) > 0                               # the clipped frame has region pixels
    assert all(torch.equal(a, b) for a, b in zip(flats, before))            # nothing was written so far
    for how, matte, col in paste_variants(c, colour):
        for flat, keep in zip(flats, before):
            flat.copy_(keep)
        want = [ops.frames_paste_u8_aligned(*one(n), feather=c["feather"], matte=None if matte is None else matte_of(n),
                                            colour=None if col is None else col[n:n + 1], **kw)[0] for n in range(N)]
        assert ops.frames_paste_u8_aligned(x, table, rows, feather=c["feather"], matte=matte, colour=col, **kw) is table
        for n in range(N):
            assert torch.equal(frames[n], want[n]), (how, n)
            # every byte outside the frame's own pixels is as it was: padding columns, surrounding rows, the guards
            rest = flats[n].clone()
            FC.frame_of(rest, n).copy_(FC.frame_of(before[n], n))
            assert torch.equal(rest, before[n]), (how, n)
        assert not torch.equal(frames[0], FC.frame_of(before[0], 0)) and not torch.equal(frames[FC.CLIPPED], FC.frame_of(before[FC.CLIPPED], FC.CLIPPED))


def test_absent_and_invalid_frames(pkg, dev):
    ops, c = pkg.ops, on(dev, BC.case("invalid and zero"))
    x, bg, rows, matte = c["x"], c["bg"].clone(), c["rows"], c["matte"]
    N, bad, absent = x.size(0), 2, 0
    assert not torch.isfinite(rows[bad]).all() and torch.isfinite(rows[absent]).all()
    keep = bg.clone()
    table = ops.FrameTable([None if n == absent else bg[n] for n in range(N)])
    assert table.sizes[absent] == (0, 0) and table.frames[absent] is None
    got = ops.frames_from_u8_aligned(table, c["net"], rows, mean=0.5, std=0.5)
    want = ops.frames_from_u8_aligned(bg, c["net"], rows, mean=0.5, std=0.5)
    assert bool((got[absent] == -1.0).all()) and bool((got[bad] == -1.0).all())       # shift = -mean / std
    sums, colour = ops.paste_colour_sums(x, table, rows, matte=matte), ops.paste_colour_match(x, table, rows, matte=matte)
    want_sums, want_colour = ops.paste_colour_sums(x, bg, rows, matte=matte), ops.paste_colour_match(x, bg, rows, matte=matte)
    one = torch.tensor([[1.0, 0.0]] * 3, device=dev)
    for n in (absent, bad):
        assert not sums[n].any() and torch.equal(colour[n], one), n
    assert want_sums[absent].any() and not torch.equal(want_colour[absent], one)      # the frame itself would have counted
    others = [n for n in range(N) if n != absent]
    assert torch.equal(got[others], want[others]) and torch.equal(sums[others], want_sums[others]) and torch.equal(colour[others], want_colour[others])
    pasted = ops.frames_paste_u8_aligned(x, bg, rows, matte=matte, colour=want_colour)
    ops.frames_paste_u8_aligned(x, table, rows, matte=matte, colour=colour)
    assert torch.equal(bg[absent], keep[absent]) and torch.equal(bg[bad], keep[bad])  # no entry: nothing written; a NaN row: as today
    assert torch.equal(bg[others], pasted[others]) and not torch.equal(bg[3], keep[3])


def test_permuting_the_entries_permutes_the_results(pkg, dev):
    ops, c = pkg.ops, on(dev, BC.case("matte frames"))
    x, bg, rows, matte, kw = c["x"], c["bg"], c["rows"], c["matte"], dict(feather=c["feather"])
    perm = [2, 0, 1]
    a, b = ops.FrameTable(bg.clone()), ops.FrameTable(bg.clone()[perm])
    xp, rp, mp = x[perm].contiguous(), rows[perm].contiguous(), matte[perm].contiguous()
    assert torch.equal(ops.frames_from_u8_aligned(b, c["net"], rp), ops.frames_from_u8_aligned(a, c["net"], rows)[perm])
    sums, colour = ops.paste_colour_sums(x, a, rows, matte=matte, **kw), ops.paste_colour_match(x, a, rows, matte=matte, **kw)
    assert torch.equal(ops.paste_colour_sums(xp, b, rp, matte=mp, **kw), sums[perm])
    assert torch.equal(ops.paste_colour_match(xp, b, rp, matte=mp, **kw), colour[perm])
    ops.frames_paste_u8_aligned(x, a, rows, matte=matte, colour=colour, **kw)
    ops.frames_paste_u8_aligned(xp, b, rp, matte=mp, colour=colour[perm].contiguous(), **kw)
    assert torch.equal(torch.stack(b.frames), torch.stack(a.frames)[perm]) and not torch.equal(a.frames[0], bg[0])


def test_the_sums_of_a_table_are_deterministic(pkg, dev):
    ops, c = pkg.ops, on(dev, FC.case("matte frames"))
    frames = [FC.frame_of(flat.to(dev), n) for n, flat in enumerate(FC.buffers(300))]
    table = ops.FrameTable(frames)
    first = ops.paste_colour_sums(c["x"], table, c["rows"], matte=c["matte"], feather=c["feather"]).clone()
    second = ops.paste_colour_sums(c["x"], table, c["rows"], matte=c["matte"], feather=c["feather"])
    assert torch.equal(first, second) and first.any()
    assert torch.equal(first.view(torch.int64), second.view(torch.int64))


def test_refusals_come_before_a_launch(pkg, dev):
    ops, L, c = pkg.ops, pkg._lib, on(dev, BC.case("generic"))
    x, bg, rows = c["x"], c["bg"].clone(), c["rows"]
    keep = bg.clone()
    table = ops.FrameTable(bg)
    # the table on another device than x
    for call in (lambda: ops.frames_paste_u8_aligned(x.cpu(), table, rows), lambda: ops.paste_colour_sums(x.cpu(), table, rows),
                 lambda: ops.paste_colour_match(x.cpu(), table, rows)):
        with pytest.raises(L.SpkError, match="expected a HIP device tensor"):    # x is judged first; one GPU cannot show more
            call()
    # the paste is in place
    other = bg.clone()
    for out in (other, ops.FrameTable(other)):
        with pytest.raises(L.SpkError, match="in place"):
            ops.frames_paste_u8_aligned(x, table, rows, out=out)
    assert ops.frames_paste_u8_aligned(x[:1], ops.FrameTable(other[:1]), rows[:1], out=None) is not None      # (and None is fine)
    other.copy_(keep)
    # N mismatch with x
    with pytest.raises(ValueError, match="4 generated frames, a table of 3"):
        ops.frames_paste_u8_aligned(x, ops.FrameTable(bg[:3]), rows)
    with pytest.raises(ValueError, match="4 generated frames, a table of 3"):
        ops.paste_colour_sums(x, ops.FrameTable(bg[:3]), rows)
    with pytest.raises(ValueError):
        ops.frames_from_u8_aligned(table, c["net"], rows[:3])
    # overlapping entries: fine where the frames are read, refused where they are written
    twice = ops.FrameTable([bg[0], bg[1], bg[1, 5:30, 7:40], bg[3]])
    got = ops.frames_from_u8_aligned(twice, c["net"], rows)
    assert torch.equal(got[1], ops.frames_from_u8_aligned(bg[1:2], c["net"], rows[1:2])[0])
    assert ops.paste_colour_sums(x, twice, rows).shape == (4, 13)
    with pytest.raises(L.SpkError, match="entries 1 and 2 overlap"):
        ops.frames_paste_u8_aligned(x, twice, rows)
    assert torch.equal(bg, keep) and torch.equal(other, keep)               # no refusal wrote a byte
