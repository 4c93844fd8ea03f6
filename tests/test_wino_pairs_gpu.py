"""The input transform of the Winograd forward kernel (csrc/conv3x3_wino_f32.hip) with a PAIR of tiles per lane.  In the bilinear x2
form a half-wave transforms one of the wave's two planes and a lane two tiles, one above the other; the row pass runs once over the
two raw rows they share.  (The plain and modulated forms were built with horizontal pairs too, measured, and keep a lane per tile --
DESIGN.md 4.12; their cases stay: the shapes are those at which either mapping can go wrong.)  What can go wrong is geometry -- which
raw window a lane reads, which V slots it writes, which member of a pair carries an image edge's coefficient, which plane a
half-wave takes -- so the shapes are the smallest that hold every seam: one WIDE region (8 x 32: all four image edges in one region),
2 x 2 WIDE regions (16 x 64: pair seams and region seams), one SQUARE region (16 x 16); Cin 16 (one pair of chunks: the first chunk's
planes go through the transform in front of the K loop) and Cin 32 (the K loop's transform); B = 2 (a region's last chunk transforms
the NEXT image's first planes).

Reference: the fp64 convolution of the same operands (x2: of the fp64 bilinear interpolation, align_corners=False).  Bounds: rel-L2 <
5e-6 per case, and per pixel |err| < 1e-4 max|ref| -- both from tests/test_wino_gpu.py / test_wino_x2_gpu.py.  One-hot inputs: a
single 1.0 makes the output a copy of the filter around it; every output pixel within 1e-6 times the largest weight magnitude -- a V
value written into a neighbour's slot moves a whole filter tap, which random data would only show as a blur."""
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
B, COUT = 2, 64
SHAPES = [(8, 32), (16, 64), (16, 16)]          # OUTPUT sizes: one WIDE region per image; 2 x 2 WIDE regions; one SQUARE region
CINS = [16, 32]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd").ops


def _up64(x):
    return F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False)


@functools.lru_cache(maxsize=None)
def _case(H, W, cin, up):
    """operands and the fp64 convolution of one shape: computed once, never written to"""
    g = torch.Generator().manual_seed(7919 * H + 31 * W + cin + int(up))
    x = torch.randn(B, cin, H // 2 if up else H, W // 2 if up else W, generator=g).to(DEV)
    w = (torch.randn(COUT, cin, 3, 3, generator=g) / (3 * cin ** 0.5)).to(DEV)
    ref = F.conv2d(_up64(x) if up else x.double(), w.double(), padding=1)
    return x, w, ref


def _check(y, ref, what):
    e = rel_l2(y, ref)
    err = (y.double() - ref).abs()
    top = float(ref.abs().max())
    print(f"{what}: rel-L2 {e:.2e}, worst pixel {float(err.max()):.2e} of {top:.2e}")
    assert e < TOL, e
    assert float(err.max()) < 1e-4 * top, float(err.max())
    return err


@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_plain_pairs_equal_fp64(ops, H, W, cin):
    x, w, ref = _case(H, W, cin, False)
    y = ops.conv3x3_wino(x, ops.pack_conv_weight_wino(w), COUT)
    _check(y, ref, f"plain {H}x{W} Cin {cin}")


@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_x2_pairs_equal_fp64(ops, H, W, cin):
    """the top / bottom edge coefficients belong to different members of a pair: the image's four corners are looked at on their own"""
    x, w, ref = _case(H, W, cin, True)
    assert ops.wino_fuse_x2(B, cin, COUT, H, W)
    y = ops.conv3x3_wino(x, ops.pack_conv_weight_wino(w), COUT, upsample=True)
    assert y.shape == (B, COUT, H, W)
    err = _check(y, ref, f"x2 {H}x{W} Cin {cin}")
    corners = err[:, :, [0, 0, -1, -1], [0, -1, 0, -1]]
    print(f"  corners: worst {float(corners.max()):.2e}")
    assert float(corners.max()) < 1e-4 * float(ref.abs().max()), float(corners.max())


@pytest.mark.parametrize("H,W", SHAPES)
def test_modulated_pairs_equal_fp64(ops, H, W):
    """a distinct modulation per channel and image (a plane's scale belongs to its channel alone), with the demodulation"""
    x, w, _ = _case(H, W, 16, False)
    g = torch.Generator().manual_seed(H + W)
    s = (torch.rand(B, 16, generator=g) + 0.5).to(DEV)
    d = (torch.rand(B, COUT, generator=g) + 0.5).to(DEV)
    assert s.flatten().unique().numel() == s.numel()
    y = ops.conv3x3_wino(x, ops.pack_conv_weight_wino(w), COUT, batch_scale=s, demod=d)
    ref = F.conv2d(x.double() * s.double().view(B, 16, 1, 1), w.double(), padding=1) * d.double().view(B, COUT, 1, 1)
    _check(y, ref, f"modulated {H}x{W}")


def _epilogue64(c, bias, nw, noise, style, osc, slope):
    y = c * osc + bias.double().view(1, -1, 1, 1) + nw.double().view(1, -1, 1, 1) * noise.double()
    y = F.leaky_relu(y, slope)
    s = style.double()
    return y * (s[:, :COUT].view(-1, COUT, 1, 1) + 1) + s[:, COUT:].view(-1, COUT, 1, 1)


@pytest.mark.parametrize("up", [False, True], ids=["plain", "x2"])
def test_fused_torgb_launch(ops, up):
    H, W = 16, 64
    x, w, ref = _case(H, W, 32, up)
    g = torch.Generator().manual_seed(11 + int(up))
    bias, nw = torch.randn(COUT, generator=g).to(DEV), torch.randn(COUT, generator=g).to(DEV)
    noise, style = torch.randn(B, 1, H, W, generator=g).to(DEV), torch.randn(B, 2 * COUT, generator=g).to(DEV)
    rw, rb = (torch.randn(3, COUT, 1, 1, generator=g) / 8).to(DEV), torch.randn(3, generator=g).to(DEV)
    none, img = ops.conv3x3_wino(x, ops.pack_conv_weight_wino(w), COUT, bias=bias, noise_w=nw, noise=noise, style=style, lrelu_slope=0.2,
                                 out_scale=0.7, upsample=up, rgb=(rw, rb), store_out=False)
    assert none is None
    ref_img = F.conv2d(_epilogue64(ref, bias, nw, noise, style, 0.7, 0.2), rw.double(), rb.double())
    _check(img, ref_img, f"toRGB up={up}")


@pytest.mark.parametrize("up", [False, True], ids=["plain", "x2"])
def test_sliced_launch_through_the_finisher(ops, up):
    """ksplit 2.  A slice keeps at least four chunks (spk_conv2d_wino_ksplit), so two slices need Cin 64: the smallest sliced launch"""
    H, W, cin = 16, 64, 64
    x, w, ref = _case(H, W, cin, up)
    g = torch.Generator().manual_seed(13 + int(up))
    assert ops.wino_ksplit(B, cin, COUT, H, W, 2) == 2
    bias, nw = torch.randn(COUT, generator=g).to(DEV), torch.randn(COUT, generator=g).to(DEV)
    noise, style = torch.randn(B, 1, H, W, generator=g).to(DEV), torch.randn(B, 2 * COUT, generator=g).to(DEV)
    y = ops.conv3x3_wino(x, ops.pack_conv_weight_wino(w), COUT, bias=bias, noise_w=nw, noise=noise, style=style, lrelu_slope=0.2,
                         out_scale=0.7, upsample=up, ksplit=2)
    _check(y, _epilogue64(ref, bias, nw, noise, style, 0.7, 0.2), f"ksplit 2 up={up}")


# One-hot positions in the INPUT of a 16 x 64 output (2 x 2 WIDE regions of 8 x 32 pixels = 4 x 16 tiles).
# plain: a horizontal pair of tiles covers columns 4 m .. 4 m + 3 -- pair seam between columns 3 | 4; region seams between rows 7 | 8, columns 31 | 32.
# x2 (input 8 x 32, a tile = one input pixel): a lane's pair covers input rows 2 k, 2 k + 1 -- pair seam between rows 1 | 2; region seams between
# input rows 3 | 4, columns 15 | 16.
ONE_HOT = {False: [(2, 3), (5, 4), (7, 31), (8, 32), (0, 0), (15, 63)],
           True: [(1, 5), (2, 6), (3, 15), (4, 16), (0, 0), (7, 31)]}
CHANNELS = [0, 3, 4, 7]          # of a chunk: waves 0 and 3, both half-waves


@pytest.mark.parametrize("up", [False, True], ids=["plain", "x2"])
def test_one_hot_inputs(ops, up):
    """One image per (chunk, channel of the chunk, position), all in one launch: Cin 16 -- the hot channel in the first chunk (whose planes
    the transform in front of the K loop or a predecessor's last chunk stages) and in the second (the K loop's own)."""
    H, W, cin = 16, 64, 16
    Hi, Wi = (H // 2, W // 2) if up else (H, W)
    hot = [(ck * 8 + c, py, px) for ck in (0, 1) for c in CHANNELS for (py, px) in ONE_HOT[up]]
    x = torch.zeros(len(hot), cin, Hi, Wi)
    for n, (c, py, px) in enumerate(hot):
        x[n, c, py, px] = 1.0
    x = x.to(DEV)
    w = (torch.randn(COUT, cin, 3, 3, generator=torch.Generator().manual_seed(97 + int(up))) / (3 * cin ** 0.5)).to(DEV)
    y = ops.conv3x3_wino(x, ops.pack_conv_weight_wino(w), COUT, upsample=up)
    ref = F.conv2d(_up64(x) if up else x.double(), w.double(), padding=1)
    err = (y.double() - ref).abs().amax(dim=(1, 2, 3))
    bound = 1e-6 * float(w.abs().max())
    worst = int(err.argmax())
    print(f"one-hot up={up}: worst |err| {float(err.max()):.2e} (image {worst}: channel, y, x = {hot[worst]}), bound {bound:.2e}")
    assert float(err.max()) < bound, (float(err.max()), hot[worst])
