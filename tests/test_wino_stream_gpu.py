"""The Winograd forward kernel's chunk stream (csrc/conv3x3_wino_f32.hip: operand staging interleaved with the MFMAs of the K loop,
one stream across a workgroup's regions) at every length and boundary it has: one, two and three chunk pairs; workgroups that walk
three and more regions, some one more than others; the x2 form of the same; a sliced contraction; square regions; the fused toRGB;
the modulated and the grouped form.  Against an fp64 convolution, bound 5e-6 rel-L2 (tests/test_wino_gpu.py's)."""
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


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd").ops


def _operands(seed, B, Cin, Cout, H, W, up=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H // 2 if up else H, W // 2 if up else W, generator=g).to(DEV)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)).to(DEV)
    return g, x, w


def _conv64(x, w, up=False):
    xd = x.double()
    if up:
        xd = F.interpolate(xd, scale_factor=2, mode="bilinear", align_corners=False)
    return F.conv2d(xd, w.double(), padding=1)


def _check(ops, B, Cin, Cout, H, W, up, seed):
    _, x, w = _operands(seed, B, Cin, Cout, H, W, up)
    assert ops.wino_supported(B, Cin, Cout, H, W)
    y = ops.conv3x3_wino(x, ops.pack_conv_weight_wino(w), Cout, upsample=up)
    ref = _conv64(x, w, up)
    e = rel_l2(y, ref)
    print(f"B={B} {Cin}->{Cout} {H}x{W} up={up}: rel-L2 {e:.2e}")
    assert e < TOL, e
    # every pixel, not only the aggregate: a stale or missing raw plane shows at single region borders
    err = (y.double() - ref).abs().amax(dim=(0, 1))
    assert float(err.max()) < 1e-4 * float(ref.abs().max()), float(err.max())


@pytest.mark.parametrize("up", [False, True], ids=["plain", "x2"])
@pytest.mark.parametrize("Cout", [64, 96])
@pytest.mark.parametrize("H,W", [(8, 32), (16, 64)])
@pytest.mark.parametrize("Cin", [16, 32, 48])
def test_one_two_and_three_chunk_pairs(ops, Cin, H, W, Cout, up):
    _check(ops, 2, Cin, Cout, H, W, up, seed=Cin + H + Cout)


def _walk_batch():
    """B for Cin 16 -> Cout 256 at 128^2 (64 regions per image, 4 channel tiles) such that every persistent workgroup -- the launch
    starts (CUs / 4) rounded down to a multiple of 8 per channel tile -- walks at least three regions: 3 on 256 CUs."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    gx = max(8, n_cu // 4 // 8 * 8)
    return max(1, -(-3 * gx // 64))


@pytest.mark.parametrize("up", [False, True], ids=["plain", "x2"])
@pytest.mark.parametrize("extra,H", [(0, 128), (1, 128), (0, 136)], ids=["even", "one-more-image", "ragged"])
def test_workgroups_walk_three_and_more_regions(ops, extra, H, up):
    """128^2: every workgroup the same number of regions (B images: B each on 256 CUs), then one image more; 136 x 128 (68 regions per
    image): the XCD shares and the workgroups' walks inside them differ by one."""
    _check(ops, _walk_batch() + extra, 16, 256, H, 128, up, seed=77 + extra + H)


@pytest.mark.parametrize("up", [False, True], ids=["plain", "x2"])
def test_sliced_contraction(ops, up):
    B, Cin, Cout, H, W = 1, 64, 64, 16, 64
    _, x, w = _operands(5, B, Cin, Cout, H, W, up)
    assert ops.wino_ksplit(B, Cin, Cout, H, W, 2) == 2
    y = ops.conv3x3_wino(x, ops.pack_conv_weight_wino(w), Cout, ksplit=2, upsample=up)
    e = rel_l2(y, _conv64(x, w, up))
    print(f"ksplit 2 up={up}: rel-L2 {e:.2e}")
    assert e < TOL, e


@pytest.mark.parametrize("up", [False, True], ids=["plain", "x2"])
def test_square_regions(ops, up):
    _check(ops, 2, 32, 64, 16, 16, up, seed=9)


@pytest.mark.parametrize("up", [False, True], ids=["plain", "x2"])
def test_fused_torgb(ops, up):
    B, Cin, Cout, H, W = 2, 16, 64, 16, 64
    g, x, w = _operands(11, B, Cin, Cout, H, W, up)
    rw, rb = (torch.randn(3, Cout, generator=g) / Cout ** 0.5).to(DEV), torch.randn(3, generator=g).to(DEV)
    y, rgb = ops.conv3x3_wino(x, ops.pack_conv_weight_wino(w), Cout, rgb=(rw, rb), upsample=up)
    ref = _conv64(x, w, up)
    ref_rgb = F.conv2d(ref, rw.double().view(3, Cout, 1, 1), rb.double())
    print(f"toRGB up={up}: rel-L2 {rel_l2(y, ref):.2e} / {rel_l2(rgb, ref_rgb):.2e}")
    assert rel_l2(y, ref) < TOL and rel_l2(rgb, ref_rgb) < TOL, (rel_l2(y, ref), rel_l2(rgb, ref_rgb))


def test_modulated_one_region_per_image(ops):
    B, Cin, Cout, H, W = 2, 32, 64, 8, 32
    g, x, w = _operands(13, B, Cin, Cout, H, W)
    s = (torch.rand(B, Cin, generator=g) + 0.5).to(DEV)
    d = (torch.rand(B, Cout, generator=g) + 0.5).to(DEV)
    y = ops.conv3x3_wino(x, ops.pack_conv_weight_wino(w), Cout, batch_scale=s, demod=d)
    ref = F.conv2d(x.double() * s.double().view(B, Cin, 1, 1), w.double(), padding=1) * d.double().view(B, Cout, 1, 1)
    e = rel_l2(y, ref)
    print(f"modulated: rel-L2 {e:.2e}")
    assert e < TOL, e


def test_two_groups(ops):
    B, G, Cin, Cout, H, W = 2, 2, 32, 64, 16, 64
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, G * Cin, H, W, generator=g).to(DEV)
    ws = [(torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)).to(DEV) for _ in range(G)]
    n = ops.L.lib().spk_conv2d_packed_bytes_wino(Cin, Cout) // 4
    wp = torch.empty(G * n, device=DEV)
    ops.pack_conv_weights_wino_into(ws, [wp[i * n:(i + 1) * n] for i in range(G)])
    y = ops.conv3x3_wino(x, wp, Cout, groups=G)
    ref = torch.cat([F.conv2d(x[:, q * Cin:(q + 1) * Cin].double(), ws[q].double(), padding=1) for q in range(G)], 1)
    e = rel_l2(y, ref)
    print(f"G=2: rel-L2 {e:.2e}")
    assert e < TOL, e
