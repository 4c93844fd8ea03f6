"""The region epilogue of the Winograd forward kernel (csrc/conv3x3_wino_f32.hip) in each form the host chooses: the LEAN rows (whole
channel tiles, no out_pre, no accumulate: straight-line code), the GENERIC rows (a partial last tile, out_pre, accumulate), the sliced
launch's raw partial sums and the fused toRGB with and without the stored activation.  Every case runs the full epilogue -- out_scale,
bias, noise, LeakyReLU 0.2 with a gain, style -- against an fp64 convolution followed by the fp64 epilogue, bound 5e-6 rel-L2
(tests/test_wino_gpu.py's); the forms must agree with each other bit for bit: they differ in addressing and control flow only."""
import functools
import importlib
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOL = 5e-6
DEV = "cuda:0"
B, CIN, CMAX = 2, 16, 128
SLOPE, GAIN, OSC = 0.2, 2 ** 0.5, 0.7
SHAPES = [(8, 32), (16, 64), (16, 16)]          # one WIDE region per image; 2 x 2 WIDE regions; SQUARE
UPS = [False, True]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd").ops


def _operands(seed, b, cin, cout, H, W, up):
    g = torch.Generator().manual_seed(seed)
    t = {"x": torch.randn(b, cin, H // 2 if up else H, W // 2 if up else W, generator=g),
         "w": torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5),
         "bias": torch.randn(cout, generator=g), "nw": torch.randn(cout, generator=g),
         "noise": torch.randn(b, 1, H, W, generator=g), "style": torch.randn(b, 2 * cout, generator=g)}
    return g, {k: v.to(DEV) for k, v in t.items()}


def _first(t, C):
    """the first C filters and their epilogue operands"""
    full = t["w"].shape[0]
    return {"x": t["x"], "w": t["w"][:C].contiguous(), "bias": t["bias"][:C].contiguous(), "nw": t["nw"][:C].contiguous(), "noise": t["noise"],
            "style": torch.cat([t["style"][:, :C], t["style"][:, full:full + C]], dim=1).contiguous()}


def _ref(t, up):
    """fp64: (after the style, before the style)"""
    x = t["x"].double()
    if up:
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    C = t["w"].shape[0]
    y = F.conv2d(x, t["w"].double(), padding=1) * OSC + t["bias"].double().view(1, -1, 1, 1) + t["nw"].double().view(1, -1, 1, 1) * t["noise"].double()
    pre = F.leaky_relu(y, SLOPE) * GAIN
    s = t["style"].double()
    return pre * (s[:, :C].view(-1, C, 1, 1) + 1) + s[:, C:].view(-1, C, 1, 1), pre


def _run(ops, t, up, **kw):
    C = t["w"].shape[0]
    return ops.conv3x3_wino(t["x"], ops.pack_conv_weight_wino(t["w"]), C, bias=t["bias"], noise_w=t["nw"], noise=t["noise"], style=t["style"],
                            lrelu_slope=SLOPE, act_gain=GAIN, out_scale=OSC, upsample=up, **kw)


@functools.lru_cache(maxsize=None)
def _case(H, W, up):
    """operands, the fp64 references and the LEAN launches (Cout 128, and 64 = its first channel tile) of one shape: computed once"""
    ops_ = importlib.import_module("speak-hack_amd").ops
    _, t = _operands(1000 * H + W + int(up), B, CIN, CMAX, H, W, up)
    ref, ref_pre = _ref(t, up)
    return {"t": t, "ref": ref, "ref_pre": ref_pre, "lean128": _run(ops_, t, up), "lean64": _run(ops_, _first(t, 64), up)}


def _bits(a):
    return a.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("up", UPS, ids=["plain", "x2"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_lean_rows_equal_fp64(ops, H, W, up):
    c = _case(H, W, up)
    e128, e64 = rel_l2(c["lean128"], c["ref"]), rel_l2(c["lean64"], c["ref"][:, :64])
    print(f"lean {H}x{W} up={up}: rel-L2 Cout 128 {e128:.2e}, Cout 64 {e64:.2e}")
    assert e128 < TOL and e64 < TOL, (e128, e64)
    assert _same_bits(c["lean64"], c["lean128"][:, :64])         # a channel's result does not depend on the launch's tile count


@pytest.mark.parametrize("up", UPS, ids=["plain", "x2"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_partial_tile_equals_lean_bit_for_bit(ops, H, W, up):
    c = _case(H, W, up)
    y96 = _run(ops, _first(c["t"], 96), up)
    e = rel_l2(y96, c["ref"][:, :96])
    print(f"Cout 96 {H}x{W} up={up}: rel-L2 {e:.2e}")
    assert e < TOL, e
    assert _same_bits(y96, c["lean128"][:, :96])


@pytest.mark.parametrize("up", UPS, ids=["plain", "x2"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_out_pre_rows_equal_lean_bit_for_bit(ops, H, W, up):
    c = _case(H, W, up)
    pre = torch.empty(B, CMAX, H, W, device=DEV)
    y = _run(ops, c["t"], up, out_pre=pre)
    e = rel_l2(pre, c["ref_pre"])
    print(f"out_pre {H}x{W} up={up}: rel-L2 {e:.2e}")
    assert _same_bits(y, c["lean128"])
    assert e < TOL, e


@pytest.mark.parametrize("up", UPS, ids=["plain", "x2"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_accumulate_rows(ops, H, W, up):
    c = _case(H, W, up)
    y0 = _run(ops, c["t"], up, out=torch.zeros(B, CMAX, H, W, device=DEV), accumulate=True)
    assert torch.equal(y0, c["lean128"])
    base = torch.randn(B, CMAX, H, W, generator=torch.Generator().manual_seed(H + W)).to(DEV)
    y = _run(ops, c["t"], up, out=base.clone(), accumulate=True)
    e = rel_l2(y, base.double() + c["ref"])
    print(f"accumulate {H}x{W} up={up}: rel-L2 {e:.2e}")
    assert e < TOL, e


@pytest.mark.parametrize("up", UPS, ids=["plain", "x2"])
def test_sliced_launch_full_epilogue(ops, up):
    """ksplit 2: the kernel writes raw partial sums (lean rows, no epilogue flag) and the finisher applies the epilogue"""
    b, cin, cout, H, W = 1, 64, 64, 16, 64
    _, t = _operands(5, b, cin, cout, H, W, up)
    assert ops.wino_ksplit(b, cin, cout, H, W, 2) == 2
    y = _run(ops, t, up, ksplit=2)
    e = rel_l2(y, _ref(t, up)[0])
    print(f"ksplit 2 up={up}: rel-L2 {e:.2e}")
    assert e < TOL, e


@pytest.mark.parametrize("up", UPS, ids=["plain", "x2"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_fused_torgb_with_and_without_the_activation(ops, H, W, up):
    c = _case(H, W, up)
    t = _first(c["t"], 64)
    g = torch.Generator().manual_seed(H * W)
    rw, rb = (torch.randn(3, 64, 1, 1, generator=g) / 8).to(DEV), torch.randn(3, generator=g).to(DEV)
    none, rgb_only = _run(ops, t, up, rgb=(rw, rb), store_out=False)
    y, rgb = _run(ops, t, up, rgb=(rw, rb))
    assert none is None
    ref_rgb = F.conv2d(c["ref"][:, :64], rw.double(), rb.double())
    e = rel_l2(rgb, ref_rgb)
    print(f"toRGB {H}x{W} up={up}: rel-L2 {e:.2e}")
    assert _same_bits(rgb_only, rgb)
    assert _same_bits(y, c["lean64"])
    assert e < TOL, e


def _walk_batch():
    """B for Cin 16 -> Cout 256 at 128^2 (64 regions per image, 4 channel tiles) such that every persistent workgroup -- the launch
    starts (CUs / 4) rounded down to a multiple of 8 per channel tile -- walks at least three regions: 3 on 256 CUs."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    gx = max(8, n_cu // 4 // 8 * 8)
    return max(1, -(-3 * gx // 64))


@pytest.mark.parametrize("up", UPS, ids=["plain", "x2"])
def test_walk_of_three_regions_with_the_full_epilogue(ops, up):
    """A region's stores are still in flight when the next region's K loop starts: every pixel of every region is checked."""
    b = _walk_batch()
    _, t = _operands(321 + int(up), b, 16, 256, 128, 128, up)
    y = _run(ops, t, up)
    ref, _ = _ref(t, up)
    e = rel_l2(y, ref)
    err = (y.double() - ref).abs().amax(dim=(0, 1))
    print(f"walk B={b} up={up}: rel-L2 {e:.2e}, worst pixel {float(err.max()):.2e} of {float(ref.abs().max()):.2e}")
    assert e < TOL, e
    assert float(err.max()) < 1e-4 * float(ref.abs().max()), float(err.max())
