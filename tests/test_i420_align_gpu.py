"""GPU checks of the aligned I420 edge (csrc/frame_sim_i420.hip): ``ops.frames_from_i420_aligned``, ``ops.paste_colour_sums_i420``,
``ops.paste_colour_match_i420`` and ``ops.frames_paste_i420_aligned``.  The defining property is the criterion: on an I420 surface
the launchers give the fp32 bits, the fp64 sums, the rows and the Y, U and V bytes the NV12 launchers give on the NV12 surface with
the same Y bytes and ``UV[cy][cx] = (U[cy][cx], V[cy][cx])`` -- ``torch.equal``, no tolerance.  The way in is also held to the fp64
model tests/nv12_sim_ref.py, within the bound tests/test_nv12_align_gpu.py uses for the NV12 way in (``TOL_IN``, imported from
there).  The cases are those of tests/nv12_sim_cases.py as tests/i420_cases.py lays them out: Y at pitch 64, U at the odd pitch 29
from an odd address with an odd image stride, V at pitch 32, every plane an allocation of its own between guard bytes."""
import importlib

import numpy as np
import pytest
import torch

import i420_cases as IC
import nv12_sim_cases as NC
import nv12_sim_ref as M
from test_nv12_align_gpu import TOL_IN

pytestmark = pytest.mark.gpu
NAMES = sorted(NC.SPECS)
BGR = {"wide 709", "matte frames 709", "constant"}                         # the cases whose way in is asked in bgr first


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
    """A case on the device: the pitched I420 planes of tests/i420_cases.py (``planes``, views of ``flats``), the NV12 surface they
    de-interleave (``nv12``: contiguous planes), and the rest of the case"""

    def __init__(self, c, dev):
        self.c, self.layout = c, c["layout"]
        self.flats = [f.to(dev) for f in c["flats"]]
        self.planes = self.layout.planes(self.flats, 0)
        self.nv12 = (c["y"].to(dev), c["uv"].to(dev))
        self.x, self.rows = c["x"].to(dev), c["rows"].to(dev)
        self.matte = None if c["matte"] is None else c["matte"].to(dev)
        self.colour, self.net, self.feather = c["colour"], c["net"], c["feather"]

    def intact(self):
        return self.layout.rest_intact(self.flats, self.c["flats"])


def test_the_layout_is_what_the_cases_say(dev):
    """On the device: an odd U address, an odd U pitch and image stride, pitches that differ, the bytes of the NV12 case"""
    s = On(IC.case("generic 601"), dev)
    y, u, v = s.planes
    assert u.data_ptr() % 2 == 1 and u.stride(1) % 2 == 1 and u.stride(0) % 2 == 1 and u.stride(1) != v.stride(1) and y.stride(1) == 64
    assert torch.equal(y, s.nv12[0]) and torch.equal(IC.interleave(u, v), s.nv12[1]) and s.intact()


@pytest.mark.parametrize("name", NAMES)
def test_way_in_is_the_nv12_way_in_bit_for_bit(pkg, dev, name):
    ops, s = pkg.ops, On(IC.case(name), dev)
    c = s.c
    orders = ("bgr", "rgb") if name in BGR else ("rgb", "bgr")
    for order in orders:
        got = ops.frames_from_i420_aligned(s.planes, s.net, s.rows, channel_order=order, **s.colour)
        want = ops.frames_from_nv12_aligned(s.nv12, s.net, s.rows, channel_order=order, **s.colour)
        assert got.dtype == torch.float32 and torch.equal(got, want), order
        if order == orders[0]:                                             # and the fp64 model, within the NV12 test's bound
            to_rgb, _ = NC.coeffs(**s.colour)
            model, hit = M.warp_in(c["y"].numpy(), c["uv"].numpy(), np.asarray(c["rows"]), s.net[0], s.net[1], to_rgb, swap_rb=order == "bgr")
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - model).max())
            print(f"way in, {name}, {order}: largest |got - model| = {err:.3e} (bound {TOL_IN}); {int((~hit).sum())} of {hit.size} outputs by rule")
            assert err <= TOL_IN
            assert (got.cpu().numpy()[(~hit)[:, None].repeat(3, 1)] == -1.0).all()
    # host rows, contiguous planes, the packed tensor and one frame as 2-D planes: the same bits
    f = ops.frames_from_i420_aligned
    got = f(s.planes, s.net, s.rows, **s.colour)
    apart = (c["y"].to(dev), c["u"].to(dev), c["v"].to(dev))
    assert torch.equal(f(apart, s.net, s.rows, **s.colour), got)
    packed = torch.cat([c["y"].flatten(1), c["u"].flatten(1), c["v"].flatten(1)], 1).view(-1, 3 * IC.H // 2, IC.W).to(dev)
    assert torch.equal(f(packed, s.net, s.rows, **s.colour), got)
    if not c["by_rule"]:
        assert torch.equal(f(s.planes, s.net, c["rows"], **s.colour), got)
    assert torch.equal(f(tuple(p[1] for p in s.planes), s.net, s.rows[1:2], **s.colour), got[1:2])
    assert s.intact()


@pytest.mark.parametrize("name", NAMES)
def test_sums_and_rows_are_the_nv12_ones_bit_for_bit(pkg, dev, name):
    ops, s = pkg.ops, On(IC.case(name), dev)
    kw = dict(matte=s.matte, feather=s.feather, **s.colour)
    sums, want = ops.paste_colour_sums_i420(s.x, s.planes, s.rows, **kw), ops.paste_colour_sums_nv12(s.x, s.nv12, s.rows, **kw)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (s.x.size(0), 13)
    assert torch.equal(sums.view(torch.int64), want.view(torch.int64)) and bool(want.any())
    rows, want_rows = ops.paste_colour_match_i420(s.x, s.planes, s.rows, **kw), ops.paste_colour_match_nv12(s.x, s.nv12, s.rows, **kw)
    assert torch.equal(rows.view(torch.int32), want_rows.view(torch.int32))
    for n in s.c["by_rule"]:
        assert not sums[n].any() and torch.equal(rows[n], torch.tensor([[1.0, 0.0]] * 3, device=dev))
    assert s.intact() and all(torch.equal(a.cpu(), b) for a, b in zip(s.flats, s.c["flats"]))       # the statistics only read


@pytest.mark.parametrize("name", NAMES)
def test_paste_leaves_the_bytes_of_the_nv12_paste(pkg, dev, name):
    """Plain, with the case's matte, with colour rows and with both: in place on the pitched planes"""
    ops, c = pkg.ops, IC.case(name)
    ref = On(c, dev)
    stat = dict(matte=ref.matte, feather=ref.feather, **ref.colour)
    colour = ops.paste_colour_match_nv12(ref.x, ref.nv12, ref.rows, **stat)
    differs = False
    for how, matte, col in (("plain", None, None), ("matte", ref.matte, None), ("colour", None, colour), ("both", ref.matte, colour)):
        kw = dict(feather=ref.feather, matte=matte, colour=col, **ref.colour)
        want = ops.nv12_planes(ops.frames_paste_nv12_aligned(ref.x, ref.nv12, ref.rows, **kw))
        want_u, want_v = IC.split(want[1])
        s = On(c, dev)
        assert ops.frames_paste_i420_aligned(s.x, s.planes, s.rows, out=s.planes, **kw) is s.planes        # in place
        y, u, v = s.planes
        assert torch.equal(y, want[0]) and torch.equal(u, want_u) and torch.equal(v, want_v), how
        assert s.intact(), how                                             # every guard and pitch-padding byte
        for n in (~torch.isfinite(c["rows"]).all(1)).nonzero().flatten().tolist():       # a frame with a NaN row: every byte as it was
            assert torch.equal(y[n].cpu(), c["y"][n]) and torch.equal(u[n].cpu(), c["u"][n]) and torch.equal(v[n].cpu(), c["v"][n]), how
        differs |= not torch.equal(y.cpu(), c["y"]) and not torch.equal(u.cpu(), c["u"]) and not torch.equal(v.cpu(), c["v"])
        # cloned: out=None gives a packed clone with the same bytes and leaves the input alone; another out= receives a copy
        t = On(c, dev)
        got = ops.frames_paste_i420_aligned(t.x, t.planes, t.rows, **kw)
        assert tuple(got.shape) == (t.x.size(0), 3 * IC.H // 2, IC.W) and got.is_contiguous()
        gy, gu, gv = ops.i420_planes(got)
        assert torch.equal(gy, y) and torch.equal(gu, u) and torch.equal(gv, v), how
        assert all(torch.equal(a.cpu(), b) for a, b in zip(t.flats, c["flats"])), how
        if how == "both":
            other = tuple(torch.zeros(p.shape, dtype=torch.uint8, device=dev) for p in t.planes)
            assert ops.frames_paste_i420_aligned(t.x, t.planes, t.rows, out=other, **kw) is other
            assert torch.equal(other[0], y) and torch.equal(other[1], u) and torch.equal(other[2], v)
    assert differs                                                         # the paste wrote all three planes


def test_yv12_is_the_same_call_with_the_planes_swapped_in_memory(pkg, dev):
    """One allocation: Y, then V, then U (YV12): the planes may lie in any order"""
    ops, c = pkg.ops, IC.case("wide 709")
    N, q = c["y"].size(0), IC.H * IC.W // 4
    buf = torch.cat([c["y"].flatten(1), c["v"].flatten(1), c["u"].flatten(1)], 1).to(dev)
    y, v, u = buf[:, :4 * q].view(N, IC.H, IC.W), buf[:, 4 * q:5 * q].view(N, IC.H // 2, IC.W // 2), buf[:, 5 * q:].view(N, IC.H // 2, IC.W // 2)
    assert v.data_ptr() < u.data_ptr()
    rows, x, kw = c["rows"].to(dev), c["x"].to(dev), dict(feather=c["feather"], **c["colour"])
    nv12 = (c["y"].to(dev), c["uv"].to(dev))
    assert torch.equal(ops.frames_from_i420_aligned((y, u, v), c["net"], rows, **c["colour"]), ops.frames_from_nv12_aligned(nv12, c["net"], rows, **c["colour"]))
    want = ops.nv12_planes(ops.frames_paste_nv12_aligned(x, nv12, rows, **kw))
    ops.frames_paste_i420_aligned(x, (y, u, v), rows, out=(y, u, v), **kw)
    assert torch.equal(y, want[0]) and torch.equal(u, want[1][..., 0]) and torch.equal(v, want[1][..., 1])


def test_refusals_come_before_a_launch(pkg, dev):
    ops, L = pkg.ops, pkg._lib
    s = On(IC.case("generic 601"), dev)
    y, u, v = s.planes
    with pytest.raises(L.SpkError, match="no CPU path"):
        ops.frames_from_i420_aligned(tuple(p.cpu() for p in s.planes), s.net, s.rows)
    with pytest.raises(L.SpkError, match="pixel stride"):
        ops.frames_from_i420_aligned((y, torch.zeros(4, 20, 56, dtype=torch.uint8, device=dev)[:, :, ::2], v), s.net, s.rows)
    with pytest.raises(L.SpkError, match="must not overlap"):              # frames of a written surface that share bytes
        ops.frames_paste_i420_aligned(s.x, s.planes, s.rows, out=(y, u[:1].expand(4, -1, -1), v))
    with pytest.raises(ValueError, match="4 generated frames, 3 I420 frames"):
        ops.frames_paste_i420_aligned(s.x, tuple(p[:3] for p in s.planes), s.rows)
    with pytest.raises(L.SpkError, match="out must hold"):
        ops.frames_paste_i420_aligned(s.x, s.planes, s.rows, out=torch.zeros(4, 63, 56, dtype=torch.uint8, device=dev))       # 42 x 56
    torch.cuda.synchronize()
    assert s.intact() and all(torch.equal(a.cpu(), b) for a, b in zip(s.flats, s.c["flats"]))
