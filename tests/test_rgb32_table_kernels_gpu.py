"""GPU checks of the aligned RGB32 edge over an ``ops.Rgb32Table`` (csrc/frame_table_rgb32.hip).  The defining property is the
criterion: entry ``n`` of a table gives, bit for bit, what the strided launch at ``N = 1`` gives on entry ``n`` -- the way in, both
statistics and the four pastes -- ``torch.equal``, no tolerance (the strided launchers are held to the rgb24 ones by
tests/test_rgb32_align_gpu.py).  The frames are the five-size layout of tests/frame_table_cases.py as tests/rgb32_cases.py lays it out:
40 x 56; a 33 x 47 view at pixel offset (3, 5) of a 40 x 60 surface (4-aligned, not 16-aligned); 64 x 48; the 9 x 11 frame the region
overhangs on all four sides; 1 x 1 -- five allocations at pitch 4 W + 16 between guard bytes.  An absent entry behaves as an invalid
row: ``shift_c`` on the way in, zero sums, rows (1, 0), and its frame -- like every fourth, pitch and guard byte -- untouched."""
import importlib

import pytest
import torch

import rgb32_cases as RC

pytestmark = pytest.mark.gpu
CASES = [(name, order) for name in RC.NAMES for order in RC.ORDERS]
IDS = [f"{name}-{order}" for name, order in CASES]
F = len(RC.SIZES)


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
    """A mixed case on the device: five flat buffers, the frame of each as a view [h,w,4], and the rest of the case.  ``absent``:
    the entries a table made by ``table()`` leaves out"""

    def __init__(self, c, dev, absent=()):
        self.c, self.order, self.absent = c, c["order"], set(absent)
        self.flats = [f.to(dev) for f in c["flats"]]
        self.frames = [s.view(f)[0] for s, f in zip(c["surfaces"], self.flats)]
        self.x, self.rows = c["x"].to(dev), c["rows"].to(dev)
        m = c["matte"]
        self.matte = None if m is None else m.to(dev)
        self.net, self.feather = c["net"], c["feather"]

    def table(self, ops):
        return ops.Rgb32Table([None if n in self.absent else f for n, f in enumerate(self.frames)])

    def matte_of(self, n):
        return None if self.matte is None else self.matte if self.matte.dim() == 2 else self.matte[n:n + 1]

    def untouched(self):
        return all(torch.equal(f.cpu(), b) for f, b in zip(self.flats, self.c["flats"]))


def test_the_layout_is_what_the_cases_say(pkg, dev):
    s = On(RC.mixed("generic", "rgba"), dev)
    assert [tuple(f.shape) for f in s.frames] == [(h, w, 4) for h, w in RC.SIZES]
    assert s.frames[1].data_ptr() % 16 == 4 and s.frames[1].stride(0) == 256 and all(f.stride(0) == 4 * bw + 16 for f, (_, bw, *_) in zip(s.frames, RC.FC.LAYOUT))
    t = s.table(pkg.ops)
    assert len(t) == F and t.sizes == RC.SIZES and t.dev.numel() == 24 * F


@pytest.mark.parametrize("name,order", CASES, ids=IDS)
def test_way_in_and_statistics_of_entry_n_are_the_strided_launch_on_it(pkg, dev, name, order):
    ops, s = pkg.ops, On(RC.mixed(name, order), dev)
    table = s.table(ops)
    got = ops.frames_from_rgb32_aligned(table, s.net, s.rows, channel_order=order)
    kw = dict(matte=s.matte, feather=s.feather, channel_order=order)
    sums, rows = ops.paste_colour_sums_rgb32(s.x, table, s.rows, **kw), ops.paste_colour_match_rgb32(s.x, table, s.rows, **kw)
    assert tuple(got.shape) == (F, 3, *s.net) and tuple(sums.shape) == (F, 13) and tuple(rows.shape) == (F, 3, 2)
    for n, f in enumerate(s.frames):
        one = dict(matte=s.matte_of(n), feather=s.feather, channel_order=order)
        want = ops.frames_from_rgb32_aligned(f, s.net, s.rows[n:n + 1], channel_order=order)
        assert torch.equal(got[n:n + 1].view(torch.int32), want.view(torch.int32)), n
        want = ops.paste_colour_sums_rgb32(s.x[n:n + 1], f.unsqueeze(0), s.rows[n:n + 1], **one)
        assert torch.equal(sums[n:n + 1].view(torch.int64), want.view(torch.int64)), n
        want = ops.paste_colour_match_rgb32(s.x[n:n + 1], f.unsqueeze(0), s.rows[n:n + 1], **one)
        assert torch.equal(rows[n:n + 1].view(torch.int32), want.view(torch.int32)), n
    assert bool(sums.any()) and s.untouched()


@pytest.mark.parametrize("name,order", CASES, ids=IDS)
def test_paste_into_entry_n_is_the_strided_paste_into_it(pkg, dev, name, order):
    """Plain, with the case's matte, with colour rows and with both: every byte of every buffer -- colour, fourth bytes, the
    surroundings of the view, pitch and guards -- is that of the strided launch at N = 1 in place on a copy"""
    ops, c = pkg.ops, RC.mixed(name, order)
    ref = On(c, dev)
    colour = ops.paste_colour_match_rgb32(ref.x, ref.table(ops), ref.rows, matte=ref.matte, feather=ref.feather, channel_order=order)
    differs = 0
    for how, matte, col in (("plain", False, None), ("matte", True, None), ("colour", False, colour), ("both", True, colour)):
        s, t = On(c, dev), On(c, dev)
        table = s.table(ops)
        kw = dict(feather=s.feather, channel_order=order)
        assert ops.frames_paste_rgb32_aligned(s.x, table, s.rows, matte=s.matte if matte else None, colour=col, **kw) is table
        for n, f in enumerate(t.frames):
            one = f.unsqueeze(0)
            ops.frames_paste_rgb32_aligned(t.x[n:n + 1], one, t.rows[n:n + 1], out=one, matte=t.matte_of(n) if matte else None,
                                           colour=None if col is None else col[n:n + 1], **kw)
            assert torch.equal(s.flats[n], t.flats[n]), (how, n)
            # and what no paste may change: every fourth byte, and every byte that is no pixel of the frame
            assert torch.equal(RC.fourth(s.frames[n], order).cpu(), RC.fourth(c["surfaces"][n].view(c["flats"][n])[0], order)), (how, n)
            assert c["surfaces"][n].outside_intact(s.flats[n], c["flats"][n]), (how, n)
            differs += not torch.equal(s.flats[n].cpu(), c["flats"][n])
    assert differs >= 4                                                     # the pastes wrote


@pytest.mark.parametrize("order", RC.ORDERS)
def test_an_absent_entry_behaves_as_an_invalid_row(pkg, dev, order):
    ops, c = pkg.ops, RC.mixed("feather and matte", order)
    full, s = On(c, dev), On(c, dev, absent=(0, 2))
    table = s.table(ops)
    assert table.sizes[0] == (0, 0) and table.sizes[2] == (0, 0)
    kw = dict(matte=s.matte, feather=s.feather, channel_order=order)
    got, want = ops.frames_from_rgb32_aligned(table, s.net, s.rows, channel_order=order), ops.frames_from_rgb32_aligned(full.table(ops), s.net, s.rows, channel_order=order)
    sums, want_sums = ops.paste_colour_sums_rgb32(s.x, table, s.rows, **kw), ops.paste_colour_sums_rgb32(full.x, full.table(ops), full.rows, **kw)
    rows = ops.paste_colour_match_rgb32(s.x, table, s.rows, **kw)
    for n in range(F):
        if n in s.absent:
            assert bool((got[n] == -1.0).all()) and not sums[n].any() and torch.equal(rows[n], torch.tensor([[1.0, 0.0]] * 3, device=dev)), n
        else:
            assert torch.equal(got[n], want[n]) and torch.equal(sums[n], want_sums[n]), n
    ops.frames_paste_rgb32_aligned(s.x, table, s.rows, **kw)
    ops.frames_paste_rgb32_aligned(full.x, full.table(ops), full.rows, **kw)
    for n in range(F):
        if n in s.absent:
            assert torch.equal(s.flats[n].cpu(), c["flats"][n]), n          # the frame of an absent entry: untouched
        else:
            assert torch.equal(s.flats[n], full.flats[n]), n
    assert not torch.equal(full.flats[0].cpu(), c["flats"][0])
    # a table with every entry absent is a table
    none = ops.Rgb32Table([None] * 3)
    assert bool((ops.frames_from_rgb32_aligned(none, s.net, s.rows[:3], channel_order=order) == -1.0).all())


def test_refusals_come_before_a_launch(pkg, dev):
    ops, L = pkg.ops, pkg._lib
    s = On(RC.mixed("generic", "bgra"), dev)
    table = s.table(ops)
    with pytest.raises(ValueError, match="5 generated frames, a table of 4 frames"):
        ops.frames_paste_rgb32_aligned(s.x, ops.Rgb32Table(s.frames[:4]), s.rows)
    with pytest.raises(L.SpkError, match="pasted in place"):
        ops.frames_paste_rgb32_aligned(s.x, table, s.rows, out=s.frames[0])
    with pytest.raises(L.SpkError, match="overlap"):                        # written frames that share bytes
        ops.frames_paste_rgb32_aligned(s.x, ops.Rgb32Table([s.frames[0]] * 2 + s.frames[2:]), s.rows)
    shared = ops.Rgb32Table([s.frames[0]] * 2 + s.frames[2:])               # ... which the way in, which only reads, takes
    assert torch.equal(ops.frames_from_rgb32_aligned(shared, s.net, s.rows)[0], ops.frames_from_rgb32_aligned(table, s.net, s.rows)[0])
    with pytest.raises(ValueError, match="aligned to 4 bytes"):
        ops.Rgb32Table([s.flats[0][RC.GUARD + 1:RC.GUARD + 1 + 4 * 6].view(2, 3, 4)])
    with pytest.raises(ValueError, match=r"\[H,W,4\]"):
        ops.Rgb32Table([s.frames[0][..., :3]])
    with pytest.raises(ValueError, match="Rgb32Table"):                     # the tables are not each other's
        ops.frames_paste_rgb32_aligned(s.x, ops.FrameTable([torch.zeros(4, 4, 3, dtype=torch.uint8, device=dev)] * F), s.rows)
    torch.cuda.synchronize()
    assert s.untouched()
