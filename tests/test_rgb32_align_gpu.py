"""GPU checks of the aligned RGB32 edge (csrc/frame_sim_rgb32.hip): ``ops.frames_from_rgb32_aligned``, ``ops.paste_colour_sums_rgb32``,
``ops.paste_colour_match_rgb32`` and ``ops.frames_paste_rgb32_aligned``.  The defining property is the criterion: on an RGB32 frame
the launchers give the fp32 bits, the fp64 sums, the rows and the colour bytes the rgb24 launchers give on a contiguous copy of the
colour bytes -- ``torch.equal``, no tolerance: identical byte values go through identical arithmetic in an identical order (the
rgb24 launchers are held to the fp64 model by tests/test_align_gpu.py and tests/test_blend_gpu.py) -- and EVERY FOURTH BYTE, every
pitch byte and every guard byte is what it was.  The cases are those of tests/blend_cases.py as tests/rgb32_cases.py lays them out
(40 x 56 frames at pitch 4 W + 16 between guard bytes, nets 16 x 16 and 12 x 20), each in the four channel orders, and a 33 x 47 view
at pixel offset (3, 5) of a 40 x 60 surface whose first pixel is 4-aligned and not 16-aligned."""
import importlib

import pytest
import torch

import rgb32_cases as RC

pytestmark = pytest.mark.gpu
CASES = [(name, order) for name in RC.NAMES for order in RC.ORDERS]
IDS = [f"{name}-{order}" for name, order in CASES]


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
    """A case on the device: the pitched RGB32 frames (``frames``, a view of ``flat``), the packed colour bytes they hold (``bg``),
    and the rest of the case"""

    def __init__(self, c, dev):
        self.c, self.surface, self.order = c, c["surface"], c["order"]
        self.rgb = RC.colour_of(self.order)[0]
        self.flat = c["flat"].to(dev)
        assert self.flat.data_ptr() % 16 == 0
        self.frames = self.surface.view(self.flat)
        self.bg = c["bg"].to(dev)
        self.x, self.rows = c["x"].to(dev), c["rows"].to(dev)
        self.matte = None if c.get("matte") is None else c["matte"].to(dev)
        self.net, self.feather = c["net"], c.get("feather", 0.0)

    def untouched(self):
        return torch.equal(self.flat.cpu(), self.c["flat"])


def test_the_layout_is_what_the_cases_say(dev):
    s = On(RC.case("generic", "argb"), dev)
    assert s.frames.stride() == (40 * 240, 240, 4, 1) and s.frames.data_ptr() % 4 == 0 and not s.frames.is_contiguous()
    assert torch.equal(RC.packed(s.frames, "argb"), s.bg) and int(RC.fourth(s.frames, "argb").max()) < 255
    r = On(RC.roi_case("bgra"), dev)
    assert tuple(r.frames.shape) == (1, 33, 47, 4) and r.frames.data_ptr() % 16 == 4 and r.frames.stride(1) == 256


@pytest.mark.parametrize("name,order", CASES, ids=IDS)
def test_way_in_is_the_rgb24_way_in_bit_for_bit(pkg, dev, name, order):
    ops, s = pkg.ops, On(RC.case(name, order), dev)
    got = ops.frames_from_rgb32_aligned(s.frames, s.net, s.rows, channel_order=order)
    want = ops.frames_from_u8_aligned(s.bg, s.net, s.rows, channel_order=s.rgb)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
    flipped = ops.frames_from_u8_aligned(s.bg, s.net, s.rows, channel_order="bgr" if s.rgb == "rgb" else "rgb")
    assert not torch.equal(got, flipped)                                    # the order is read, not guessed
    # a contiguous copy, one frame as [H,W,4], host rows, and a view that has to be copied (a pixel stride): the same bits
    assert torch.equal(ops.frames_from_rgb32_aligned(s.frames.contiguous(), s.net, s.rows, channel_order=order), got)
    assert torch.equal(ops.frames_from_rgb32_aligned(s.frames[1], s.net, s.rows[1:2], channel_order=order), got[1:2])
    if not s.c["by_rule"]:
        assert torch.equal(ops.frames_from_rgb32_aligned(s.frames, s.net, s.c["rows"], channel_order=order), got)
    wide = torch.zeros((*s.frames.shape[:2], 2 * RC.BC.W, 4), dtype=torch.uint8, device=dev)
    wide[:, :, ::2] = s.frames
    assert torch.equal(ops.frames_from_rgb32_aligned(wide[:, :, ::2], s.net, s.rows, channel_order=order), got)
    for n in s.c["by_rule"]:
        if not bool(torch.isfinite(s.rows[n]).all()):
            assert bool((got[n] == -1.0).all())
    assert s.untouched()


@pytest.mark.parametrize("name,order", CASES, ids=IDS)
def test_sums_and_rows_are_the_rgb24_ones_bit_for_bit(pkg, dev, name, order):
    ops, s = pkg.ops, On(RC.case(name, order), dev)
    kw = dict(matte=s.matte, feather=s.feather)
    sums = ops.paste_colour_sums_rgb32(s.x, s.frames, s.rows, channel_order=order, **kw)
    want = ops.paste_colour_sums(s.x, s.bg, s.rows, channel_order=s.rgb, **kw)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (s.x.size(0), 13)
    assert torch.equal(sums.view(torch.int64), want.view(torch.int64)) and bool(want.any())
    rows = ops.paste_colour_match_rgb32(s.x, s.frames, s.rows, channel_order=order, **kw)
    want_rows = ops.paste_colour_match(s.x, s.bg, s.rows, channel_order=s.rgb, **kw)
    assert torch.equal(rows.view(torch.int32), want_rows.view(torch.int32))
    for n in s.c["by_rule"]:
        assert not sums[n].any() and torch.equal(rows[n], torch.tensor([[1.0, 0.0]] * 3, device=dev))
    assert s.untouched()                                                    # the statistics only read


def check_paste(s, got, want, how):
    """``got``: RGB32 frames after a paste on the inputs of ``s``; ``want``: the rgb24 paste on the packed colour bytes"""
    assert torch.equal(RC.packed(got, s.order), want), how                  # the colour bytes
    assert torch.equal(RC.fourth(got, s.order).cpu(), RC.fourth(s.surface.view(s.c["flat"]), s.order)), how       # every fourth byte


@pytest.mark.parametrize("name,order", CASES, ids=IDS)
def test_paste_leaves_the_colour_bytes_of_the_rgb24_paste_and_every_other_byte(pkg, dev, name, order):
    """Plain, with the case's matte, with colour rows and with both: in place on the pitched frames, cloned, and into another
    pitched buffer"""
    ops, c = pkg.ops, RC.case(name, order)
    ref = On(c, dev)
    colour = ops.paste_colour_match(ref.x, ref.bg, ref.rows, channel_order=ref.rgb, matte=ref.matte, feather=ref.feather)
    differs = False
    for how, matte, col in (("plain", None, None), ("matte", ref.matte, None), ("colour", None, colour), ("both", ref.matte, colour)):
        kw = dict(feather=ref.feather, matte=matte, colour=col)
        want = ops.frames_paste_u8_aligned(ref.x, ref.bg, ref.rows, channel_order=ref.rgb, **kw)
        s = On(c, dev)
        assert ops.frames_paste_rgb32_aligned(s.x, s.frames, s.rows, out=s.frames, channel_order=order, **kw) is s.frames       # in place
        check_paste(s, s.frames, want, how)
        assert s.surface.rest_intact(s.flat, c["flat"]), how               # every guard and pitch byte
        for n in (~torch.isfinite(c["rows"]).all(1)).nonzero().flatten().tolist():       # a frame with a NaN row: every byte as it was
            assert torch.equal(s.frames[n].cpu(), s.surface.view(c["flat"])[n]), how
        differs |= not torch.equal(want, ref.bg)
        # cloned: out=None gives a contiguous clone with the same bytes and leaves the input alone
        t = On(c, dev)
        got = ops.frames_paste_rgb32_aligned(t.x, t.frames, t.rows, channel_order=order, **kw)
        assert got.is_contiguous() and torch.equal(got, s.frames) and t.untouched(), how
        # another out=, pitched and between guards of its own, first receives a copy
        other = torch.full((s.surface.size,), 0x3C, dtype=torch.uint8, device=dev)
        before = other.clone()
        out = s.surface.view(other)
        assert ops.frames_paste_rgb32_aligned(t.x, t.frames, t.rows, out=out, channel_order=order, **kw) is out
        assert torch.equal(out, s.frames) and s.surface.rest_intact(other, before) and t.untouched(), how
    assert differs


@pytest.mark.parametrize("order", RC.ORDERS)
def test_a_view_at_a_pixel_offset_of_a_wider_surface(pkg, dev, order):
    """33 x 47 at (3, 5) of 40 x 60: the first pixel 4-aligned and not 16-aligned; the surroundings of the view stay as they were"""
    ops, c = pkg.ops, RC.roi_case(order)
    s = On(c, dev)
    assert s.frames.data_ptr() % 16 == 4
    got = ops.frames_from_rgb32_aligned(s.frames, s.net, s.rows, channel_order=order)
    assert torch.equal(got, ops.frames_from_u8_aligned(s.bg, s.net, s.rows, channel_order=s.rgb))
    sums = ops.paste_colour_sums_rgb32(s.x, s.frames, s.rows, channel_order=order, feather=2.0)
    assert torch.equal(sums, ops.paste_colour_sums(s.x, s.bg, s.rows, channel_order=s.rgb, feather=2.0)) and bool(sums.any())
    want = ops.frames_paste_u8_aligned(s.x, s.bg, s.rows, channel_order=s.rgb, feather=2.0)
    assert ops.frames_paste_rgb32_aligned(s.x, s.frames, s.rows, out=s.frames, channel_order=order, feather=2.0) is s.frames
    check_paste(s, s.frames, want, order)
    assert not torch.equal(want, s.bg) and s.surface.outside_intact(s.flat, c["flat"])


def test_refusals_come_before_a_launch(pkg, dev):
    ops, L = pkg.ops, pkg._lib
    s = On(RC.case("generic", "bgra"), dev)
    odd = s.flat[RC.GUARD + 1:RC.GUARD + 1 + 4 * 40 * 56 * 4].view(4, 40, 56, 4)          # a misaligned base
    assert odd.data_ptr() % 4 == 1
    with pytest.raises(L.SpkError, match="aligned 32-bit words"):
        ops.frames_paste_rgb32_aligned(s.x, odd, s.rows, out=odd, channel_order="bgra")
    # read only, the same view is copied: the bits are those of its contiguous copy
    assert torch.equal(ops.frames_from_rgb32_aligned(odd, s.net, s.rows, channel_order="bgra"),
                       ops.frames_from_rgb32_aligned(odd.clone(), s.net, s.rows, channel_order="bgra"))
    with pytest.raises(L.SpkError, match="no CPU path"):
        ops.frames_from_rgb32_aligned(s.frames.cpu(), s.net, s.rows)
    with pytest.raises(L.SpkError, match="must not overlap"):              # frames of a written tensor that share bytes
        ops.frames_paste_rgb32_aligned(s.x, s.frames, s.rows, out=s.frames[:1].expand(4, -1, -1, -1), channel_order="bgra")
    with pytest.raises(L.SpkError, match="aligned 32-bit words"):           # a row pitch that is no multiple of 4
        pitch = torch.zeros(4, 40, 4 * 56 + 2, dtype=torch.uint8, device=dev)
        ops.frames_paste_rgb32_aligned(s.x, s.frames, s.rows, out=pitch[:, :, :4 * 56].unflatten(2, (56, 4)), channel_order="bgra")
    with pytest.raises(ValueError, match=r"frames must be \[4,H,W,4\]"):
        ops.frames_paste_rgb32_aligned(s.x, s.bg, s.rows)
    with pytest.raises(ValueError, match="channel_order"):
        ops.frames_paste_rgb32_aligned(s.x, s.frames, s.rows, channel_order="bgr")
    torch.cuda.synchronize()
    assert s.untouched()
