"""The Winograd conv of a bilinear x2 layer with the interpolation inside the input transform (SPK_CONV_WINOGRAD |
SPK_CONV_UPSAMPLE2X, csrc/conv3x3_wino_f32.hip): the launch reads the low-resolution tensor, B^T (bilinear) B is one 4x3 matrix
per dimension, the conv's zero padding of the x2 image a coefficient of the edge tiles.  Reference: the fp64 convolution of the fp64
interpolation, plus the epilogue in fp64 (``_ref`` of tests/test_wino_gpu.py).  Bounds, both from that file: rel-L2 < 5e-6, and per
pixel |err| < 1e-4 max|ref| -- a wrong edge coefficient moves one row or column of pixels, which the aggregate would not show."""
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


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd").ops


def _ref(x, w, **kw):
    y = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False), w.double(), padding=1)
    if kw.get("out_scale") is not None:
        y = y * kw["out_scale"]
    if kw.get("bias") is not None:
        y = y + kw["bias"].double().view(1, -1, 1, 1)
    if kw.get("noise") is not None:
        y = y + kw["noise_w"].double().view(1, -1, 1, 1) * kw["noise"].double()
    if kw.get("slope") is not None:
        y = F.leaky_relu(y, kw["slope"])
    pre = y
    if kw.get("style") is not None:
        C = w.shape[0]
        s = kw["style"].double()
        y = y * (s[:, :C].view(-1, C, 1, 1) + 1) + s[:, C:].view(-1, C, 1, 1)
    return y, pre


def _operands(B, Cin, Cout, Hs, Ws, dev):
    g = torch.Generator().manual_seed(B * 1000 + Cin + Cout + Hs + 7 * Ws)
    x = torch.randn(B, Cin, Hs, Ws, generator=g).to(dev)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)).to(dev)
    return g, x, w


def _check(y, ref):
    assert rel_l2(y, ref) < TOL, rel_l2(y, ref)
    err = (y.double() - ref).abs().amax(dim=(0, 1))
    assert float(err.max()) < 1e-4 * float(ref.abs().max()), float(err.max())


# The persistent grid is min(CUs / channel tiles rounded down to 8, items rounded up to 8) workgroups per channel tile, each XCD (workgroup
# index % 8) walking a contiguous eighth of the item list.  One item per workgroup (256 CUs): one WIDE region touching all four image
# edges / 3 x 3 WIDE regions, the centre one without an edge / two images, ragged Cout / one SQUARE region / 2 x 3 SQUARE regions /
# the sliced contraction (the 1/16 goes through the finisher) / 128 items, one channel tile.
# SEVERAL items per workgroup -- the current / next coefficient sets, their select in a region's last chunk and the clamped offsets'
# hand-over: 4 channel tiles -> 64 workgroups per tile; 8 images = 128 items, 2 per workgroup within one image (an XCD's 16 items are one
# image's); 6 images = 96 items, 12 per XCD: half the workgroups walk 2 items, and those of the odd XCDs step from one image into the
# next (items 12 -> 20, 44 -> 52, ...); 512 items of a 64 x 256 output against 256 workgroups of one channel tile.
@pytest.mark.parametrize("B,Cin,Cout,Hs,Ws,ksplit", [(1, 16, 64, 4, 16, 0), (1, 16, 64, 12, 48, 0), (2, 32, 48, 8, 32, 0), (1, 16, 64, 8, 8, 0),
                                                     (1, 32, 64, 16, 24, 0), (1, 64, 64, 8, 8, 2), (8, 16, 64, 16, 64, 0),
                                                     (8, 16, 256, 16, 64, 0), (6, 16, 256, 16, 64, 0), (8, 16, 64, 32, 128, 0)])
def test_wino_x2_plain_equals_fp64(ops, B, Cin, Cout, Hs, Ws, ksplit):
    dev = torch.device("cuda:0")
    _, x, w = _operands(B, Cin, Cout, Hs, Ws, dev)
    assert ops.wino_fuse_x2(B, Cin, Cout, 2 * Hs, 2 * Ws)
    if ksplit:
        assert ops.wino_ksplit(B, Cin, Cout, 2 * Hs, 2 * Ws, want=ksplit) == ksplit
    wp = ops.pack_conv_weight_wino(w)
    y = ops.conv3x3_wino(x, wp, Cout, upsample=True, ksplit=ksplit)
    assert y.shape == (B, Cout, 2 * Hs, 2 * Ws)
    ref, _ = _ref(x, w)
    _check(y, ref)
    assert rel_l2(y, ops.conv3x3_wino(ops.upsample2x_bilinear(x), wp, Cout, ksplit=ksplit)) < TOL


def test_wino_x2_full_epilogue(ops):
    dev = torch.device("cuda:0")
    B, Cin, Cout, Hs, Ws = 2, 64, 64, 8, 32
    g, x, w = _operands(B, Cin, Cout, Hs, Ws, dev)
    H, W = 2 * Hs, 2 * Ws
    bias, nw = torch.randn(Cout, generator=g).to(dev), torch.randn(Cout, generator=g).to(dev)
    noise = torch.randn(B, 1, H, W, generator=g).to(dev)
    style = torch.randn(B, 2 * Cout, generator=g).to(dev)
    pre = torch.empty(B, Cout, H, W, device=dev)
    wp = ops.pack_conv_weight_wino(w)
    kw = dict(bias=bias, noise_w=nw, noise=noise, style=style, lrelu_slope=0.2, out_scale=0.7)
    y = ops.conv3x3_wino(x, wp, Cout, upsample=True, out_pre=pre, **kw)
    ref, ref_pre = _ref(x, w, bias=bias, noise_w=nw, noise=noise, style=style, slope=0.2, out_scale=0.7)
    _check(y, ref)
    _check(pre, ref_pre)
    assert rel_l2(y, ops.conv3x3_wino(ops.upsample2x_bilinear(x), wp, Cout, **kw)) < TOL


def test_wino_x2_fused_torgb(ops):
    dev = torch.device("cuda:0")
    B, Cin, Cout, Hs, Ws = 2, 64, 64, 8, 32
    g, x, w = _operands(B, Cin, Cout, Hs, Ws, dev)
    H, W = 2 * Hs, 2 * Ws
    bias, nw = torch.randn(Cout, generator=g).to(dev), torch.randn(Cout, generator=g).to(dev)
    noise = torch.randn(B, 1, H, W, generator=g).to(dev)
    style = torch.randn(B, 2 * Cout, generator=g).to(dev)
    rw, rb = (torch.randn(3, Cout, 1, 1, generator=g) / Cout ** 0.5).to(dev), torch.randn(3, generator=g).to(dev)
    wp = ops.pack_conv_weight_wino(w)
    kw = dict(bias=bias, noise_w=nw, noise=noise, style=style, lrelu_slope=0.2, out_scale=0.7)
    none, img = ops.conv3x3_wino(x, wp, Cout, upsample=True, rgb=(rw, rb), store_out=False, **kw)
    assert none is None and img.shape == (B, 3, H, W)
    ref, _ = _ref(x, w, bias=bias, noise_w=nw, noise=noise, style=style, slope=0.2, out_scale=0.7)
    ref_img = F.conv2d(ref, rw.double(), rb.double())
    _check(img, ref_img)
    y, img2 = ops.conv3x3_wino(x, wp, Cout, upsample=True, rgb=(rw, rb), **kw)
    _check(y, ref)
    assert torch.equal(img2, img)
    _, img_m = ops.conv3x3_wino(ops.upsample2x_bilinear(x), wp, Cout, rgb=(rw, rb), store_out=False, **kw)
    assert rel_l2(img, img_m) < TOL


def test_wino_x2_rejects_what_it_does_not_serve(ops):
    L = importlib.import_module("speak-hack_amd")._lib
    dev = torch.device("cuda:0")
    x, w = torch.randn(2, 32, 8, 32, device=dev), torch.randn(64, 32, 3, 3, device=dev)
    wp = ops.pack_conv_weight_wino(w)
    msg = "SPK_CONV_UPSAMPLE2X is the bilinear x2 of a plain launch"
    with pytest.raises(L.SpkError, match=msg):          # a modulated conv keeps its pass
        ops.conv3x3_wino(x, wp, 64, upsample=True, batch_scale=torch.ones(2, 32, device=dev))
    with pytest.raises(L.SpkError, match=msg):          # a grouped launch
        ops.conv3x3_wino(x, torch.cat([ops.pack_conv_weight_wino(w[:, :16].contiguous())] * 2), 64, upsample=True, groups=2)
    # an odd output height cannot be twice an input height: the descriptor says H = 17 over Hin = 8
    assert not L.lib().spk_conv2d_wino_up_supported(2, 32, 64, 17, 64)
    # the 2 GB limit of the 32-bit gather offsets is the INPUT tensor's: an x2 image of 4 GB over an input of 1 GB is served
    assert L.lib().spk_conv2d_wino_up_supported(64, 64, 64, 512, 512) and not L.lib().spk_conv2d_wino_supported(64, 64, 64, 512, 512)
    assert not L.lib().spk_conv2d_wino_up_supported(64, 256, 64, 512, 512)
    d, _ = ops.conv_desc(x, wp, 64, flags=L.CONV_WINOGRAD, upsample=True, out=torch.empty(2, 64, 17, 64, device=dev))
    d.H = 17
    with pytest.raises(L.SpkError, match="needs an output of twice the input size"):
        ops._launch_conv2d(d)
    # the upfirdn2d form is not the bilinear one
    d, _ = ops.conv_desc(x, wp, 64, flags=L.CONV_WINOGRAD, upsample=True, up_fir=True, out=torch.empty(2, 64, 16, 64, device=dev))
    with pytest.raises(L.SpkError, match=msg):
        ops._launch_conv2d(d)
