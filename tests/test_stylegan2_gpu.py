"""GPU parity of the build-defined StyleGAN2 variant (parity unpinned by the reference,
which has no StyleGAN2 code): modulated conv with the modulation folded into the input staging and the
demodulation into the epilogue, upfirdn2d, modulated toRGB, and the whole variant decoder, against the CPU
restatement of the published formulas (oracle/modconv_ref.py).  Tolerance 2e-5 per op, 2e-4 end to end; backward
against autograd of those formulas in fp64 (mask-flip-robust criterion)."""
import importlib

import pytest
import torch
import torch.nn.functional as F

from conftest import grad_close, rel_l2
from oracle import modconv_ref as M
from oracle.weights_recipe import recipe_input, recipe_tensor

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sg2():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd.stylegan2")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("speak-hack_amd.ops")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("up,down,pad,k1d,shape", [
    (2, 1, (2, 1), (1, 3, 3, 1), (2, 5, 8, 8)),       # Upsample
    (1, 2, (1, 1), (1, 3, 3, 1), (1, 3, 12, 10)),     # Downsample
    (1, 1, (1, 1), (1, 2, 1), (2, 4, 7, 9)),          # Blur, 3-tap
    (1, 1, (2, 1), (1, 3, 3, 1), (1, 2, 6, 6)),       # Blur after a transposed conv
    (2, 2, (3, 2), (1, 3, 3, 1), (1, 2, 9, 5)),       # both, odd sizes
    (1, 1, (-1, 0), (1, 3, 3, 1), (1, 1, 8, 8)),      # negative padding = crop
])
def test_upfirdn2d(ops, dev, up, down, pad, k1d, shape):
    """StyleGAN2's own uses at small sizes, held to an aggregate norm: every output here is at most 16 columns wide and every filter
    symmetric with fx == fy.  The per-branch tests -- all twelve separable instantiations at three widths, asymmetric filters, the
    generic kernel, exact impulses, element-wise bounds -- are tests/test_small_fwd_kernels_gpu.py's (cases: small_fwd_cases.py)."""
    x = recipe_input(f"ufd.{up}.{down}.{pad}.{shape}", shape)
    k = M.make_kernel(k1d) * (up ** 2)
    ref = M.upfirdn2d(x, k, up, down, pad)
    y = ops.upfirdn2d(x.to(dev), k, up, down, pad)
    assert y.shape == ref.shape
    assert rel_l2(y, ref) < 2e-6


@pytest.mark.parametrize("B,Cin,Cout,H", [(2, 16, 24, 8), (3, 64, 64, 16), (1, 512, 512, 4), (8, 128, 64, 32), (2, 20, 40, 11)])
@pytest.mark.parametrize("demodulate", [True, False])
def test_modulated_conv3x3(sg2, dev, B, Cin, Cout, H, demodulate):
    m = sg2.ModulatedConv2d(Cin, Cout, 3, 32, demodulate=demodulate)
    with torch.no_grad():
        m.weight.copy_(recipe_tensor(f"mc.{Cin}.{Cout}.weight", m.weight.shape, 1.0))
        m.modulation.weight.copy_(recipe_tensor(f"mc.{Cin}.mod.weight", m.modulation.weight.shape, 1.0))
        m.modulation.bias.copy_(1.0 + recipe_tensor(f"mc.{Cin}.mod.bias", m.modulation.bias.shape, 0.2))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = recipe_input(f"mc.x.{B}.{Cin}.{H}", (B, Cin, H, H))
    st = recipe_input(f"mc.st.{B}", (B, 32))
    ref = M.modulated_conv2d(x, sd["weight"], M.equal_linear(st, sd["modulation.weight"], sd["modulation.bias"]), demodulate)
    with torch.no_grad():
        y = m.to(dev)(x.to(dev), st.to(dev))
    assert rel_l2(y, ref) < 2e-5


@pytest.mark.parametrize("B", [1, 3, 8, 11])
def test_demod_grouped_launch(ops, dev, B):
    """All layers' demodulation vectors in one launch: rsqrt(scale^2 sum_{ci,k} (w s)^2 + eps) per (batch, cout),
    ragged channel counts (Cout not a multiple of 4, Cin not of 64), 3x3 and 1x1 taps, batch beyond one register pass."""
    shapes = [(24, 16, 3), (512, 512, 3), (5, 70, 1), (64, 128, 3), (33, 9, 3)]
    items = []
    for i, (Cout, Cin, k) in enumerate(shapes):
        w = recipe_tensor(f"dg.{i}.w", (Cout, Cin, k, k), 1.0)
        s = 1.0 + recipe_tensor(f"dg.{i}.s.{B}", (B, Cin), 0.5)
        items.append((w, s, 1 / (Cin * k * k) ** 0.5))
    got = ops.modconv_demod_grouped([(w.to(dev), s.to(dev), sc) for w, s, sc in items])
    for (w, s, sc), d in zip(items, got):
        ww = (sc * w.double()[None] * s.double()[:, None, :, None, None])
        ref = torch.rsqrt(ww.pow(2).sum((2, 3, 4)) + 1e-8)
        assert d.shape == ref.shape and rel_l2(d, ref) < 2e-6
        assert rel_l2(ops.modconv_demod(w.to(dev), s.to(dev), sc), ref) < 2e-6


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 16, 24, 8, 8), (1, 6, 10, 5, 7), (3, 64, 32, 16, 16), (9, 12, 8, 3, 4), (8, 128, 64, 32, 32)])
def test_modulated_conv_fused_upfirdn(sg2, dev, B, Cin, Cout, H, W):
    """upfirdn2d(up=2, [1,3,3,1]) folded into the modulated conv's input staging (SPK_CONV_UP_FIR1331) vs
    the oracle's materialised Upsample -> modulated conv; ragged channels, odd / non-square sizes."""
    m = sg2.ModulatedConv2d(Cin, Cout, 3, 32)
    with torch.no_grad():
        m.weight.copy_(recipe_tensor(f"mcu.{Cin}.{Cout}.weight", m.weight.shape, 1.0))
        m.modulation.weight.copy_(recipe_tensor(f"mcu.{Cin}.mod.weight", m.modulation.weight.shape, 1.0))
        m.modulation.bias.copy_(1.0 + recipe_tensor(f"mcu.{Cin}.mod.bias", m.modulation.bias.shape, 0.2))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = recipe_input(f"mcu.x.{B}.{Cin}.{H}.{W}", (B, Cin, H, W))
    st = recipe_input(f"mcu.st.{B}", (B, 32))
    s = M.equal_linear(st, sd["modulation.weight"], sd["modulation.bias"])
    ref = M.modulated_conv2d(M.upsample2x(x), sd["weight"], s, True)
    with torch.no_grad():
        y = m.to(dev)(x.to(dev), st.to(dev), upsample=True)
    assert y.shape == ref.shape == (B, Cout, 2 * H, 2 * W)
    assert rel_l2(y, ref) < 2e-5


def test_styled_conv_and_to_rgb(sg2, dev):
    B, Cin, Cout, H = 2, 32, 24, 8
    for upsample in (False, True):
        m = sg2.StyledConv(Cin, Cout, 3, 32, upsample=upsample)
        with torch.no_grad():
            m.noise.weight.fill_(0.37)
            m.activate.bias.copy_(recipe_tensor("sc.act.bias", (Cout,), 0.3))
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        x, st = recipe_input("sc.x", (B, Cin, H, H)), recipe_input("sc.st", (B, 32))
        Ho = 2 * H if upsample else H
        nz = recipe_input(f"sc.nz.{Ho}", (B, 1, Ho, Ho))
        ref = M.styled_conv(x, st, sd, "", nz, upsample)
        with torch.no_grad():
            y = m.to(dev)(x.to(dev), st.to(dev), nz.to(dev))
        assert rel_l2(y, ref) < 2e-5, upsample
    rgb = sg2.ToRGB(Cin, 32)
    with torch.no_grad():
        rgb.bias.copy_(recipe_tensor("rgb.bias", (1, 3, 1, 1), 0.3))
    sd = {k: v.detach().clone() for k, v in rgb.state_dict().items()}
    x, st, skip = recipe_input("rgb.x", (B, Cin, 16, 16)), recipe_input("rgb.st", (B, 32)), recipe_input("rgb.skip", (B, 3, 8, 8))
    ref = M.to_rgb(x, st, sd, "", skip)
    with torch.no_grad():
        y = rgb.to(dev)(x.to(dev), st.to(dev), skip.to(dev))
    assert rel_l2(y, ref) < 2e-5


@pytest.mark.parametrize("B,res", [(2, 256), (1, 64)])
def test_variant_generator_vs_oracle(sg2, dev, B, res):
    torch.manual_seed(5)
    g = sg2.StyleGAN2Generator(6144, resolution=res).eval()
    with torch.no_grad():
        for n, p in g.named_parameters():
            if n.endswith("noise.weight"):
                p.fill_(0.1)
            elif n.endswith("activate.bias") or (n.endswith("bias") and "to_rgb" in n and "modulation" not in n):
                p.normal_(0, 0.1)
    sd = {k: v.detach().clone() for k, v in g.state_dict().items()}
    feats = recipe_input(f"sg2.f.{B}", (B, 6144))
    noises = [recipe_input(f"sg2.n{i}.{B}.{res}", s) for i, s in enumerate(M.noise_shapes(B, res))]
    with torch.no_grad():
        ref = M.generator(feats, sd, noises, resolution=res)
        y = g.to(dev)(feats.to(dev), [n.to(dev) for n in noises])
        y2 = g(feats.to(dev))                       # device-drawn noise path
    assert y.shape == (B, 3, res, res) and torch.isfinite(y2).all()
    assert rel_l2(y, ref) < 2e-4


@pytest.mark.parametrize("upsample", [False, True])
@pytest.mark.parametrize("B,Cin,Cout,H", [(2, 20, 24, 8), (3, 70, 130, 12), (8, 128, 64, 16), (1, 64, 64, 32), (2, 16, 16, 4), (2, 8, 8, 5)])
def test_styled_conv_backward(sg2, dev, upsample, B, Cin, Cout, H):
    """Backward of the modulated conv (data, weight, modulation incl. the demodulation path, noise weight, bias) vs
    autograd of the published formulas evaluated in fp64.  Round 3: the fused form (SPK_CONV_IN_BATCH_SCALE weight gradient,
    spk_modconv_dx_finish, spk_modconv_demod_bwd) on ragged channel blocks, several pixel tiles per workgroup, the batch
    changing between a workgroup's tiles, and the small / odd planes that take the rescale-first fallback (4^2, 5^2)."""
    m = sg2.StyledConv(Cin, Cout, 3, 32, upsample=upsample)
    with torch.no_grad():
        m.noise.weight.fill_(0.37)
        m.activate.bias.copy_(recipe_tensor(f"scb.act.bias.{Cout}", (Cout,), 0.3))
    Ho = 2 * H if upsample else H
    x, st, nz = recipe_input(f"scb.x.{B}.{Cin}.{H}", (B, Cin, H, H)), recipe_input(f"scb.st.{B}", (B, 32)), recipe_input(f"scb.nz.{B}.{Ho}", (B, 1, Ho, Ho))
    gy = recipe_input(f"scb.gy.{B}.{Cout}.{Ho}", (B, Cout, Ho, Ho))
    res = {}
    for name, dt_, device in (("ref32", torch.float32, "cpu"), ("ref64", torch.float64, "cpu"), ("hip", torch.float32, dev)):
        xi = x.detach().clone().to(device, dt_).requires_grad_(True)
        si = st.detach().clone().to(device, dt_).requires_grad_(True)
        if name == "hip":
            mm = m.to(dev)
            y = mm(xi, si, nz.to(dev))
            params = dict(mm.named_parameters())
        else:
            params = {k: v.detach().clone().to(dt_).requires_grad_(True) for k, v in m.state_dict().items()}
            y = M.styled_conv(xi, si, params, "", nz.to(dt_), upsample)
        (y * gy.to(device, dt_)).sum().backward()
        g = {k: p.grad for k, p in params.items() if p.grad is not None}
        g["x"], g["style"] = xi.grad, si.grad
        res[name] = (y, g)
        if name == "hip":
            for p in mm.parameters():
                p.grad = None
    assert rel_l2(res["hip"][0], res["ref64"][0]) < 2e-5
    assert set(res["hip"][1]) == set(res["ref64"][1]) and "conv.modulation.weight" in res["hip"][1] and "noise.weight" in res["hip"][1]
    for k in res["ref64"][1]:
        ok, info = grad_close(res["hip"][1][k], res["ref32"][1][k], res["ref64"][1][k], pixels=B * Ho * Ho)
        assert ok, (k, info)


def test_variant_generator_backward(sg2, dev):
    """Whole variant decoder, fwd + bwd of a quadratic loss, every parameter and the input latent."""
    B, res = 2, 32
    torch.manual_seed(6)
    g = sg2.StyleGAN2Generator(6144, resolution=res).train()
    with torch.no_grad():
        for n, p in g.named_parameters():
            if n.endswith("noise.weight"):
                p.fill_(0.1)
            elif n.endswith("activate.bias") or (n.endswith("bias") and "to_rgb" in n and "modulation" not in n):
                p.normal_(0, 0.1)
    feats = recipe_input(f"sg2b.f.{B}", (B, 6144))
    noises = [recipe_input(f"sg2b.n{i}.{B}.{res}", s) for i, s in enumerate(M.noise_shapes(B, res))]
    target = recipe_input("sg2b.t", (B, 3, res, res))
    out = {}
    for name, dt_, device in (("ref32", torch.float32, "cpu"), ("ref64", torch.float64, "cpu"), ("hip", torch.float32, dev)):
        f = feats.detach().clone().to(device, dt_).requires_grad_(True)
        if name == "hip":
            gg = g.to(dev)
            y = gg(f, [n.to(dev) for n in noises])
            params = dict(gg.named_parameters())
        else:
            params = {k: v.detach().clone().to(dt_).requires_grad_(True) for k, v in g.state_dict().items() if v.dtype.is_floating_point}
            y = M.generator(f, params, [n.to(dt_) for n in noises], resolution=res)
        ((y - target.to(device, dt_)) ** 2).mean().backward()
        gr = {k: p.grad for k, p in params.items() if p.grad is not None}
        gr["features"] = f.grad
        out[name] = (y, gr)
    assert rel_l2(out["hip"][0], out["ref64"][0]) < 2e-4
    missing = set(out["ref64"][1]) - set(out["hip"][1])
    assert not missing, sorted(missing)[:5]
    for k in out["ref64"][1]:
        ok, info = grad_close(out["hip"][1][k], out["ref32"][1][k], out["ref64"][1][k], pixels=B * res * res)
        assert ok, (k, info)


def test_weight_gradients_on_the_second_stream_equal_in_order_launches(sg2, ops, dev, monkeypatch):
    """A training pass of the variant routes the styled convs' weights through ``autograd.WeightGateFn`` and queues each weight
    gradient AND the demodulation adjoint's share of it on ``ops.side_stream`` (the modulation's share stays on the current
    stream): bitwise the in-order schedule, where one ``spk_modconv_demod_bwd`` call writes both shares."""
    B, res = 4, 128
    torch.manual_seed(3)
    g = sg2.StyleGAN2Generator(6144, resolution=res).train().to(dev)
    with torch.no_grad():
        for n, p in g.named_parameters():
            if n.endswith("noise.weight"):
                p.fill_(0.1)
    feats = recipe_input(f"sg2s.f.{B}", (B, 6144)).to(dev)
    noises = [recipe_input(f"sg2s.n{i}.{B}.{res}", s).to(dev) for i, s in enumerate(M.noise_shapes(B, res))]

    def grads():
        g.zero_grad(set_to_none=True)
        (g(feats, noises) ** 2).mean().backward()
        return {k: p.grad.clone() for k, p in g.named_parameters() if p.grad is not None}

    assert ops.side_stream(dev) is not None
    aside = [grads() for _ in range(3)]
    monkeypatch.setattr(ops, "side_stream", lambda device: None)
    inline = grads()
    for got in aside:
        bad = [k for k in inline if not torch.equal(got[k], inline[k])]
        assert not bad, bad[:4]


def test_variant_launch_plan_equals_launch_by_launch(sg2, dev):
    """The variant's inference forward as one launch list (plan.StyleGAN2Plan) against its launch-by-launch path, which
    runs the skip upsample as the stand-alone upfirdn2d + a torch add when handed a non-matching skip -- here both paths
    use the fused toRGB, so they agree to the bit; the fused toRGB itself is held to the oracle in test_styled_conv_and_to_rgb."""
    torch.manual_seed(9)
    g = sg2.StyleGAN2Generator(6144, resolution=64).eval().to(dev)
    with torch.no_grad():
        for n, p in g.named_parameters():
            if n.endswith("noise.weight"):
                p.fill_(0.2)
    B = 3
    feats = recipe_input("sg2.plan.f", (B, 6144)).to(dev)
    noises = [recipe_input(f"sg2.plan.n{i}", s).to(dev) for i, s in enumerate(M.noise_shapes(B, 64))]
    with torch.no_grad():
        y = g(feats, noises)
        assert "_plans" in g.__dict__
        sg2.StyleGAN2Generator.use_plan = False
        try:
            y_ref = g(feats, noises)
        finally:
            sg2.StyleGAN2Generator.use_plan = True
        assert rel_l2(y, y_ref) < 1e-5          # (the plan reads cached per-(co,ci) weight norms for the demodulation: one rounding apart)
        g.convs[1].conv.weight.mul_(1.3)
        g.convs[2].noise.weight.fill_(0.5)
        y2 = g(feats, noises)
        sg2.StyleGAN2Generator.use_plan = False
        try:
            y2_ref = g(feats, noises)
        finally:
            sg2.StyleGAN2Generator.use_plan = True
        assert rel_l2(y2, y2_ref) < 1e-5 and not torch.equal(y2, y)


@pytest.mark.parametrize("B,C,H,W", [(2, 32, 16, 16), (1, 70, 6, 10), (3, 512, 8, 8), (8, 64, 64, 64)])
def test_to_rgb_with_fused_skip_upsample(ops, dev, B, C, H, W):
    """Modulated 1x1 + bias + upfirdn2d(skip, up=2, [1,3,3,1]) + add in one launch against the oracle's materialised Upsample and
    sum.  The four cases take, in order: conv1x1_small_kernel<true> (C = 32 < 64), conv1x1_small_kernel<false> (W % 4 == 2), and the
    channel-split kernel twice -- (8, 64, 64, 64) too: its (HW/4 + 255) / 256 * B = 32 is below the gate's 512.  <true> with a skip
    at C >= 64 and the other branches are tests/test_small_fwd_kernels_gpu.py's, by name (spk_conv1x1_small_form)."""
    x = recipe_input(f"rgbs.x.{B}.{C}.{H}.{W}", (B, C, H, W))
    wt = recipe_input(f"rgbs.w.{C}", (3, C, 1, 1))
    mod = 1.0 + 0.3 * recipe_input(f"rgbs.m.{B}.{C}", (B, C))
    bias = recipe_input("rgbs.b", (3,))
    skip = recipe_input(f"rgbs.s.{B}.{H}.{W}", (B, 3, H // 2, W // 2))
    sc = C ** -0.5
    ref = torch.einsum("oc,bc,bchw->bohw", wt.view(3, C).double(), mod.double(), x.double()) * sc + bias.double().view(1, 3, 1, 1) \
        + M.upsample2x(skip.double())
    y = ops.conv1x1_small_mod(x.to(dev), wt.to(dev), mod.to(dev), bias.to(dev), in_scale=sc, skip=skip.to(dev))
    assert rel_l2(y, ref) < 2e-6
