"""csrc/conv3x3_bf16x3.hip (SPK_CONV_BF16X3) branch by branch, against the split-precision emulation of
tests/bf16x3_emulation.py: the emulation splits every operand into the kernel's own bf16 hi / lo halves and sums the three
products in fp64, so kernel and reference share every operand bit and differ by the fp32 accumulation alone.

The bound is measured on the reference, never on the kernel: per case max(4 x the error of the fp32 emulation on the CPU,
sqrt(27 Cin) 2^-24) -- 0.9e-6 to 2.5e-6 for the cases here -- plus, on the x2 path, 4 x the distance between the emulations on
the fp32-ordered and on the once-rounded x2 image (a fused multiply-add in the interpolation may move a value by an ulp and, rarely,
a lo half by a step; with it 1.4e-6 to 4.1e-6).  That is below the 4.4e-6 the 16-bit truncation alone costs against an fp64
conv of the unsplit operands, and a tenth of the 3e-5 of tests/test_bf16x3_gpu.py: a lo half that is wrong on the halo ring of
one image, or in the second k-group of the ragged last chunk, is 1.6e-4 to 8.7e-4 (tests/test_bf16x3_emulation_cpu.py).
A single wrong pixel: max|y - emu| <= 8 x bound x rms(emu).

Which tile geometry, gather rounds, chunk-pipeline depth and epilogue form each case reaches is asserted on the CPU
(test_bf16x3_emulation_cpu.py::test_case_tables_cover_every_branch).

Measured on an MI355X (rel-L2 against the emulation; the bound of the same cases):
    plain              1.4e-8 .. 1.5e-7   (0.9e-6 .. 2.5e-6)      max |diff| / limit <= 0.12
    x2, both forms     7.1e-8 .. 3.5e-7   (1.4e-6 .. 4.1e-6)      max |diff| / limit <= 0.21
    modulated          9.5e-8 .. 2.2e-7   (1.4e-6 .. 3.0e-6)      max |diff| / limit <= 0.26
    y_pre              2.7e-7 .. 3.2e-7   (3.0e-6 .. 3.6e-6)
    misaligned y/noise 1.3e-7, 2.9e-7     (1.8e-6, 3.6e-6): the dword epilogue gave the staged one's figures to three digits
    data gradient      1.9e-7 .. 2.4e-7   (1.9e-6 .. 2.5e-6);  4.3e-6 .. 4.5e-6 against fp64 autograd (the truncation; bound 3e-5)
The kernel sits an order of magnitude inside the bound, and the bound two orders below the smallest wrong-half error above."""
import importlib

import pytest
import torch

import bf16x3_emulation as E
from conftest import rel_l2
from oracle.weights_recipe import recipe_tensor

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _on(dev, t, *names):
    return {n: t[n].to(dev) for n in names if n in t}


def _check(what, y, emu, bound):
    """rel-L2 and the single-pixel form, both against the emulation; the figures are printed before they are asserted."""
    y = y.detach().cpu().double()
    assert y.shape == emu.shape
    err, worst, lim = rel_l2(y, emu), float((y - emu).abs().max()), E.MAX_FACTOR * bound * E.rms(emu)
    print(f"{what}: rel-L2 {err:.2e} (bound {bound:.2e}), max |diff| {worst:.2e} (limit {lim:.2e})")
    assert err <= bound, (err, bound)
    assert worst <= lim, (worst, lim)


def _plain(pkg, dev, case, modulated=False, **kw):
    ops, ref = pkg.ops, E.plain_reference(case, modulated)
    t = ref["inputs"]
    d = _on(dev, t, "x", "w", "bias", "s", "demod")
    mod = dict(batch_scale=d["s"], demod=d["demod"], act_gain=E.ACT_GAIN) if modulated else {}
    assert ops.bf16x3_supported(*case)
    y = ops.conv3x3_bf16x3(d["x"], ops.pack_conv_weight_bf16x3(d["w"]), case[2], bias=d["bias"], lrelu_slope=E.SLOPE,
                           out_scale=E.OUT_SCALE, **mod, **kw)
    return y, ref


def _x2(pkg, dev, case, fir, modulated=False, **kw):
    ops, ref = pkg.ops, E.x2_reference(case, fir, modulated)
    t = ref["inputs"]
    d = _on(dev, t, "x", "w", "bias", "noise_w", "noise", "style", "s", "demod")
    mod = dict(batch_scale=d["s"], demod=d["demod"], act_gain=E.ACT_GAIN, out_scale=E.OUT_SCALE) if modulated else {}
    B, Cin, Cout, Hs, Ws = case
    assert ops.bf16x3_supported(B, Cin, Cout, 2 * Hs, 2 * Ws)
    y = ops.conv3x3_bf16x3(d["x"], ops.pack_conv_weight_bf16x3(d["w"]), Cout, bias=d["bias"], noise_w=d["noise_w"], noise=d["noise"],
                           style=d["style"], upsample=True, up_fir=fir, lrelu_slope=E.SLOPE, **mod, **kw)
    return y, ref


@pytest.mark.parametrize("case", E.PLAIN_CASES)
def test_plain_branches(pkg, dev, case):
    """Images per tile (1, several, cut by the 768-item limit, a ragged last group), 2 and 3 gather rounds, 1 / 2 / 3 / 4 chunks, a
    last chunk of 3 / 8 / 12 / 16 channels, staged and dword epilogue with partial tiles, TW 1 / 2 / 4; bias, LeakyReLU, out_scale."""
    y, ref = _plain(pkg, dev, case)
    _check(f"plain {case}", y, ref["y"], ref["bound"])


@pytest.mark.parametrize("fir", [False, True], ids=["bilinear", "fir1331"])
@pytest.mark.parametrize("case", E.X2_CASES)
def test_x2_branches(pkg, dev, case, fir):
    """The x2 staging (source tile in LDS, interpolation into the split image): several images per tile, the second source
    round, 2 and 3 plane rounds, 1 / 2 / 3 / 4 / 5 chunks, a last chunk of 5 / 8 / 13 / 16 channels; bias, noise, LeakyReLU, style."""
    y, ref = _x2(pkg, dev, case, fir)
    _check(f"x2 {case} fir={fir}", y, ref["y"], ref["bound"])


@pytest.mark.parametrize("case", E.PLAIN_MODULATED)
def test_plain_modulated(pkg, dev, case):
    """SPK_CONV_IN_BATCH_SCALE (it_sc: the scale of the item's own image, also in a ragged image group), out_scale_bc, act_gain."""
    y, ref = _plain(pkg, dev, case, modulated=True)
    _check(f"modulated {case}", y, ref["y"], ref["bound"])


@pytest.mark.parametrize("case,fir", E.X2_MODULATED)
def test_x2_modulated(pkg, dev, case, fir):
    """The modulation applied to the source tile (si_sc, before the interpolation), with and without SPK_CONV_UP_FIR1331."""
    y, ref = _x2(pkg, dev, case, fir, modulated=True)
    _check(f"modulated x2 {case} fir={fir}", y, ref["y"], ref["bound"])


@pytest.mark.parametrize("case,staged", [((3, 48, 64, 4, 4), True), ((2, 29, 64, 3, 5), False)])
def test_y_pre(pkg, dev, case, staged):
    """``out_pre``: the value before the style stage, from the staged and from the dword epilogue; y does not change by asking."""
    assert E.geometry(case[0], 2 * case[3], 2 * case[4], x2=True)["staged"] == staged
    y0, ref = _x2(pkg, dev, case, False)
    pre = torch.full_like(y0, float("nan"))
    y1, _ = _x2(pkg, dev, case, False, out_pre=pre)
    assert torch.equal(y0, y1)
    _check(f"y_pre {case}", pre, ref["pre"], ref["bound"])
    _check(f"y with y_pre {case}", y1, ref["y"], ref["bound"])
    assert rel_l2(ref["pre"], ref["y"]) > 0.1                     # (the two are different things)


def _offset_view(like, dev):
    """A contiguous tensor of ``like``'s shape that starts 4 bytes into a larger buffer: not 16-byte aligned."""
    buf = torch.full((like.numel() + 4,), float("nan"), device=dev)
    v = buf[1:1 + like.numel()].view(like.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return buf, v


def test_forced_dword_epilogue_by_a_misaligned_out(pkg, dev):
    """W % 4 == 0 and TW >= 4, but y is not 16-byte aligned: the dword epilogue, held to the emulation (not to the staged result)."""
    case = (3, 32, 64, 8, 8)
    ref = E.plain_reference(case)
    buf, out = _offset_view(ref["y"], dev)
    y, _ = _plain(pkg, dev, case, out=out)
    assert y.data_ptr() == out.data_ptr()
    _check(f"misaligned out {case}", y, ref["y"], ref["bound"])
    assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[1 + out.numel():]).all())        # nothing outside the view was written


def test_forced_dword_epilogue_by_a_misaligned_noise(pkg, dev):
    case = (3, 48, 64, 4, 4)
    ref = E.x2_reference(case, False)
    ops, t = pkg.ops, ref["inputs"]
    d = _on(dev, t, "x", "w", "bias", "noise_w", "style")
    _, nz = _offset_view(t["noise"], dev)
    nz.copy_(t["noise"])
    y = ops.conv3x3_bf16x3(d["x"], ops.pack_conv_weight_bf16x3(d["w"]), case[2], bias=d["bias"], noise_w=d["noise_w"], noise=nz,
                           style=d["style"], upsample=True, lrelu_slope=E.SLOPE)
    _check(f"misaligned noise {case}", y, ref["y"], ref["bound"])


@pytest.mark.parametrize("case", E.DGRAD_CASES)
def test_data_gradient_operator(pkg, dev, case):
    """The ``transpose_flip`` image run on the output-side gradient with Cin / Cout exchanged: against the emulation on the
    transposed, flipped operator, and against fp64 autograd at the 3e-5 of tests/test_bf16x3_gpu.py."""
    ops, ref = pkg.ops, E.dgrad_reference(case)
    B, Cin, Cout, H, W = case
    gy, w = ref["inputs"]["gy"].to(dev), ref["inputs"]["w"].to(dev)
    image = ops.pack_conv_weight_bf16x3(w, transpose_flip=True)
    assert image.numel() == pkg._lib.lib().spk_conv2d_packed_bytes_bf16x3(Cout, Cin)
    gx = ops.conv3x3_bf16x3(gy, image, Cin)
    _check(f"data gradient {case}", gx, ref["y"], ref["bound"])
    err = rel_l2(gx, ref["autograd"])
    print(f"data gradient {case}: rel-L2 {err:.2e} against fp64 autograd")
    assert err < 3e-5, err


@pytest.mark.parametrize("Cout", [5, 64, 130])
@pytest.mark.parametrize("Cin", [7, 16, 40])
def test_pack_bit_for_bit(pkg, dev, Cin, Cout):
    """The packed image [co tile][chunk][hi/lo][tap][h][64 co][8 ci], zero padded, byte for byte -- both operators, and ``out=``."""
    ops = pkg.ops
    w = recipe_tensor(f"bfb.pack.{Cin}.{Cout}", (Cout, Cin, 3, 3), 1.0)
    for tf in (False, True):
        want = E.pack_image(w, tf)
        got = ops.pack_conv_weight_bf16x3(w.to(dev), transpose_flip=tf)
        assert got.dtype == torch.uint8 and got.numel() == want.numel()
        assert torch.equal(got.cpu(), want), f"transpose_flip={tf}: {int((got.cpu() != want).sum())} bytes differ"
        out = torch.full((want.numel(),), 0xA5, dtype=torch.uint8, device=dev)           # the zero padding is WRITTEN
        assert ops.pack_conv_weight_bf16x3(w.to(dev), out=out, transpose_flip=tf) is out
        assert torch.equal(out.cpu(), want)


def test_pack_refuses_a_wrong_sized_out(pkg, dev):
    ops = pkg.ops
    w = torch.zeros(5, 40, 3, 3, device=dev)                # one Cout tile x three chunks; its data-gradient operator: x one chunk
    n = E.pack_image(w.cpu()).numel()
    assert n == 3 * E.pack_image(w.cpu(), True).numel()
    for bad in (n - 1, n + 16):
        with pytest.raises(pkg._lib.SpkError, match="out must hold"):
            ops.pack_conv_weight_bf16x3(w, out=torch.empty(bad, dtype=torch.uint8, device=dev))
    with pytest.raises(pkg._lib.SpkError, match="out must hold"):
        ops.pack_conv_weight_bf16x3(w, out=torch.empty(n, dtype=torch.uint8, device=dev), transpose_flip=True)   # (the other operator's size)
    with pytest.raises(pkg._lib.SpkError, match="3x3"):
        ops.pack_conv_weight_bf16x3(torch.zeros(5, 7, 1, 1, device=dev))


def test_refusals(pkg, dev):
    """What the kernel does not compute it refuses, on valid tensors and before anything is launched: the output stays as it was."""
    ops, L = pkg.ops, pkg._lib
    B, Cin, Cout, H, W = 2, 16, 8, 8, 8
    x = torch.randn(B, Cin, H, W, device=dev)
    image = ops.pack_conv_weight_bf16x3(torch.randn(Cout, Cin, 3, 3, device=dev))
    out = torch.full((B, Cout, H, W), 7.0, device=dev)
    vec = lambda n: torch.ones(n, device=dev)

    def refused(desc, match="bf16x3"):
        with pytest.raises(L.SpkError, match=match):
            ops._launch_conv2d(desc)

    def desc(x_=x, out_=out, **kw):
        return ops.conv_desc(x_, image, Cout, flags=L.CONV_BF16X3, out=out_, **kw)[0]

    refused(desc(accumulate=True))
    refused(desc(stats=torch.zeros(2 * Cout, dtype=torch.float64, device=dev)))
    refused(desc(in_affine=(vec(Cin), vec(Cin))))
    refused(desc(x_=torch.randn(B, 2 * Cin, H, W, device=dev), out_=torch.full((B, 2 * Cout, H, W), 7.0, device=dev), groups=2))
    wide = torch.full((B, Cout, 2 * H, 2 * W + 2), 7.0, device=dev)      # (every output is as large as its descriptor says)
    refused(desc(out_=wide, upsample=True, hw=(2 * H, 2 * W + 2)), match="2x the input")
    refused(desc(out_=wide, hw=(H, W + 1)), match="equal the input size")
    # demodulation without the modulation (include/spk.h: out_scale_bc without SPK_CONV_IN_BATCH_SCALE is rejected)
    d = desc(batch_scale=torch.ones(B, Cin, device=dev), demod=torch.ones(B, Cout, device=dev))
    d.flags &= ~L.CONV_IN_BATCH_SCALE
    d.in_scale = None
    refused(d, match="out_scale_bc")
    refused(desc(out_scale_dev=vec(1)), match="out_scale_dev")          # (a device scalar this kernel would not read)
    # flags without their tensors
    d = desc(noise_w=vec(Cout), noise=torch.zeros(B, 1, H, W, device=dev))
    d.noise = None
    refused(d, match="SPK_EPI_NOISE without noise")
    d = desc(noise_w=vec(Cout), noise=torch.zeros(B, 1, H, W, device=dev))
    d.noise_w = None
    refused(d, match="SPK_EPI_NOISE without noise")
    d = desc(bias=vec(Cout))
    d.bias = None
    refused(d, match="SPK_EPI_BIAS without bias")
    d = desc(batch_scale=torch.ones(B, Cin, device=dev))
    d.in_scale = None
    refused(d, match="IN_BATCH_SCALE without in_scale")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((wide == 7.0).all())
    # and the same descriptor without the offending part runs
    ops._launch_conv2d(desc())
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
