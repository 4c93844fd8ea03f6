"""Direct fp64 tests of the grouped spectral normalisation (csrc/spectral_norm.hip, called through ``ops`` rather than the
nn.Module path) and of the stand-alone StyleGAN1 / ProGAN ops of csrc/legacy_ops.hip, at the shapes that reach each branch:
row chunks and 256-column blocks with tails, flat sizes off a multiple of 4 / 1024, 16 layers per call, tensors at a 4-byte
offset (the float4 paths must fall back to the same values), planes of more than 256 pixels, both pixelnorm kernels on both
sides of their switch.  Criterion: ``assert_rounding`` of test_sg2_backward_kernels_gpu.py."""
import importlib
import math

import pytest
import torch

from oracle.weights_recipe import recipe_input, recipe_tensor
from test_sg2_backward_kernels_gpu import assert_rounding, place, rtol_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd.ops")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("speak-hack_amd._lib")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ---- spectral normalisation -------------------------------------------------------------------------------------------------
# (R, C) of the [R, C] matrix: R % 32 != 0 (a short last row chunk), C across 256-column blocks, n = R*C % 4 != 0
SN_SHAPES = [(5, 27), (37, 300), (64, 512), (48, 75), (33, 257), (512, 4608), (16, 3), (7, 1030)]


def _sn_layer(key, R, C, settled=False):
    """W [R, C] and unit u, v; ``settled``: u, v after a few float64 power iterations, as a trained layer holds them (without
    that, sigma = u^T W v of two random vectors is mostly cancellation)."""
    w = recipe_tensor(key + ".w", (R, C), 1.0 / math.sqrt(C))
    u = recipe_input(key + ".u", (R,)).double()
    v = recipe_input(key + ".v", (C,)).double()
    u, v = u / u.norm(), v / v.norm()
    for _ in range(5 if settled else 0):
        v = w.double().t() @ u
        v = v / v.norm()
        u = w.double() @ v
        u = u / u.norm()
    return w, u.float(), v.float()


def _sn_ref(w, u, v, power_iteration, eps=1e-12):
    """float64 (w_hat, u', v', sigma) and the abs-contraction scales of u', v', sigma."""
    W, u, v = w.double(), u.double(), v.double()
    if power_iteration:
        t = W.t() @ u
        v_abs = (W.abs().t() @ u.abs()) / t.norm().clamp_min(eps)
        v = t / t.norm().clamp_min(eps)
        s = W @ v
        u_abs = (W.abs() @ v.abs()) / s.norm().clamp_min(eps)
        u = s / s.norm().clamp_min(eps)
    else:
        s = W @ v
        u_abs = v_abs = None
    sigma = u @ s
    sigma_abs = u.abs() @ (W.abs() @ v.abs())
    return W / sigma, u, v, sigma, u_abs, v_abs, sigma_abs


def _check_sn_fwd(hat, sigma, u_got, v_got, w, u0, v0, power_iteration):
    rh, ru, rv, rs, u_abs, v_abs, s_abs = _sn_ref(w, u0, v0, power_iteration)
    rt = 1e-5                                       # fixed: sigma carries two chained reductions into every element of w_hat
    assert_rounding(sigma, rs.reshape(1), s_abs.reshape(1), rt, 1e-5, what="sigma")
    assert_rounding(hat, rh, 2 * w.double().abs() / rs.abs(), rt, 1e-5, what="w_hat")    # (sigma's own error, then the division)
    if power_iteration:
        assert_rounding(u_got, ru, u_abs + ru.abs(), rt, 1e-5, what="u")
        assert_rounding(v_got, rv, v_abs + rv.abs(), rt, 1e-5, what="v")
    else:
        assert torch.equal(u_got.cpu(), u0) and torch.equal(v_got.cpu(), v0)


@pytest.mark.parametrize("power_iteration", [True, False])
@pytest.mark.parametrize("misaligned", [False, True])
def test_spectral_norm_grouped(ops, dev, power_iteration, misaligned):
    """All of SN_SHAPES in one call; ``misaligned``: W, u and v 4 bytes off a 16-byte boundary (the W_hat scale must take its
    scalar loop and give the same values)."""
    layers = [_sn_layer(f"snk.{R}.{C}", R, C, settled=not power_iteration) for R, C in SN_SHAPES]
    ws = [place(w, dev, misaligned) for w, _, _ in layers]
    us = [place(u, dev, misaligned) for _, u, _ in layers]
    vs = [place(v, dev, misaligned) for _, _, v in layers]
    hats, sigma = ops.spectral_norm_grouped(ws, us, vs, power_iteration)
    for i, (w, u0, v0) in enumerate(layers):
        _check_sn_fwd(hats[i], sigma[i:i + 1], us[i], vs[i], w, u0, v0, power_iteration)


def test_spectral_norm_grouped_sixteen_layers_and_determinism(ops, L, dev):
    """16 layers in one call; the same layer gives bitwise equal u, v, sigma and W_hat alone, in the 16-layer list, and at
    another position of a different list (dp.py's replicas stay identical on this); more than SN_MAX_GROUPS layers are refused."""
    shapes = [(8 + 5 * i, 9 * (i + 1)) for i in range(16)]
    layers = [_sn_layer(f"snk16.{i}", R, C) for i, (R, C) in enumerate(shapes)]
    ws = [w.to(dev) for w, _, _ in layers]

    def run(idx):
        us, vs = [layers[i][1].to(dev) for i in idx], [layers[i][2].to(dev) for i in idx]
        hats, sigma = ops.spectral_norm_grouped([ws[i] for i in idx], us, vs, True)
        return {i: (hats[k].cpu(), sigma[k].cpu(), us[k].cpu(), vs[k].cpu()) for k, i in enumerate(idx)}

    full = run(list(range(16)))
    for i, (w, u0, v0) in enumerate(layers):
        h, s, u, v = full[i]
        _check_sn_fwd(h, s.reshape(1), u, v, w, u0, v0, True)
    for idx in ([7], [3, 7, 11], [15, 2, 7]):
        for i, got in run(idx).items():
            assert all(torch.equal(a, b) for a, b in zip(got, full[i])), f"layer {i} differs in group list {idx}"
    n = L.SN_MAX_GROUPS + 1
    with pytest.raises(L.SpkError):
        ops.spectral_norm_grouped([ws[0]] * n, [layers[0][1].to(dev)] * n, [layers[0][2].to(dev)] * n, True)


def _sn_bwd_ref(g, w, u, v, sigma):
    """float64 dW and its element-wise error bound: a few roundings of G, the n-term dot <G, W> on the rank-1 part."""
    G, W, u, v, s = g.double(), w.double(), u.double(), v.double(), float(sigma)
    dot, dot_abs = (G * W).sum(), (G * W).abs().sum()
    ref = (G - (dot / s) * torch.outer(u, v)) / s
    bound = (rtol_for(4) * G.abs() + rtol_for(G.numel()) * (dot_abs / abs(s)) * torch.outer(u.abs(), v.abs())) / abs(s)
    return ref, bound


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
def test_spectral_norm_grouped_bwd(ops, dev, misaligned, accumulate):
    """dW = (G - <G,W>/sigma u v^T) / sigma for SN_SHAPES in one call, one layer without a gradient.  ``misaligned``: G, u, v and
    the ``into`` tensors 4 bytes off (as the autograd Function's split views of one flat v are); ``accumulate``: ``into`` holds
    recipe values, checked against old + ref."""
    layers = [_sn_layer(f"snb.{R}.{C}", R, C) for R, C in SN_SHAPES]
    ws = [w.to(dev) for w, _, _ in layers]
    us = [place(u, dev, misaligned) for _, u, _ in layers]
    vs = [place(v, dev, misaligned) for _, _, v in layers]
    gs_host = [recipe_input(f"snb.{R}.{C}.g", (R, C)) for R, C in SN_SHAPES]
    gs = [place(g, dev, misaligned) for g in gs_host]
    gs[3] = None
    sigma_h = torch.stack([torch.tensor(float(w.double().norm() / 3.0)) for w, _, _ in layers]).float()
    olds = [recipe_input(f"snb.{R}.{C}.old", (R, C)) for R, C in SN_SHAPES]
    into = [place(o, dev, misaligned) for o in olds] if accumulate else None
    res = ops.spectral_norm_grouped_bwd(gs, ws, us, vs, sigma_h.to(dev), into=into)
    for i, (w, u, v) in enumerate(layers):
        if gs[i] is None:
            assert res[i] is None
            if accumulate:
                assert torch.equal(into[i].cpu(), olds[i])
            continue
        ref, bound = _sn_bwd_ref(gs_host[i], w, u, v, sigma_h[i])
        got = into[i] if accumulate else res[i]
        if accumulate:
            assert res[i] is None
            ref, bound = ref + olds[i].double(), bound + rtol_for(4) * (olds[i].double().abs() + ref.abs())
        assert_rounding(got, ref, bound, 1.0, 1e-5, what=f"dW {tuple(w.shape)}")


def test_spectral_norm_grouped_bwd_is_bitwise_reproducible(ops, dev):
    layers = [_sn_layer(f"snr.{R}.{C}", R, C) for R, C in SN_SHAPES]
    args = ([recipe_input(f"snr.{R}.{C}.g", (R, C)).to(dev) for R, C in SN_SHAPES], [w.to(dev) for w, _, _ in layers],
            [u.to(dev) for _, u, _ in layers], [v.to(dev) for _, _, v in layers], torch.full((len(layers),), 1.5, device=dev))
    a = [t.cpu() for t in ops.spectral_norm_grouped_bwd(*args)]
    b = [t.cpu() for t in ops.spectral_norm_grouped_bwd(*args)]
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- pixelnorm --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [
    (2, 6, 9, 7),          # narrow: the old golden shape
    (2, 16, 20, 20),       # narrow: 400-pixel planes, two grid-stride trips at most
    (1, 255, 64, 64),      # narrow: B*HW = 4096 but C = 255
    (1, 256, 64, 64),      # wide: B*HW = 4096 and C = 256, the switch's edge
    (4, 300, 3, 3),        # wide: C > 256 with a tail lane
    (3, 6144),             # wide: the mapping network's latent
    (2, 256, 65, 64),      # narrow: B*HW = 8320 > 4096
])
@pytest.mark.parametrize("sqrt_form", [False, True])
def test_pixelnorm_fwd_bwd(ops, dev, shape, sqrt_form):
    key = f"lgk.pn.{shape}"
    x = recipe_input(key + ".x", shape)
    dy = recipe_input(key + ".dy", shape)
    C = shape[1]
    y = ops.pixelnorm(x.to(dev), sqrt_form=sqrt_form)
    dx = ops.pixelnorm_bwd(x.to(dev), dy.to(dev))
    x64, dy64 = x.double(), dy.double()
    r = torch.rsqrt(x64.pow(2).mean(1, keepdim=True) + 1e-8)
    assert_rounding(y, x64 * r, x64.abs() * r, rtol_for(C), 1e-5, what="y")
    t = (x64 * dy64).mean(1, keepdim=True)
    t_abs = (x64 * dy64).abs().mean(1, keepdim=True)
    assert_rounding(dx, r * dy64 - x64 * r.pow(3) * t, r * dy64.abs() + x64.abs() * r.pow(3) * t_abs, rtol_for(C), 1e-5, what="dx")


# ---- instance_norm_affine ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W", [(2, 3, 9, 7), (2, 5, 20, 20), (1, 3, 64, 64)])        # 63 px; 400 px; 4096 px planes
@pytest.mark.parametrize("affine", ["none", "scale", "bias", "both"])
def test_instance_norm_affine_fwd_bwd(ops, dev, B, C, H, W, affine):
    """scale / bias are per-(b,c) column blocks of one style buffer (row stride 2C + 4, ``sb_stride``)."""
    key = f"lgk.in.{B}.{C}.{H}"
    x = 0.5 + recipe_input(key + ".x", (B, C, H, W))
    dy = recipe_input(key + ".dy", (B, C, H, W))
    sty = recipe_input(key + ".style", (B, 2 * C + 4))
    sty_d = sty.to(dev)
    scale = sty_d[:, 1:1 + C] if affine in ("scale", "both") else None
    bias = sty_d[:, 1 + C:1 + 2 * C] if affine in ("bias", "both") else None
    y = ops.instance_norm_affine(x.to(dev), scale, bias)
    dx, dscale, dbias = ops.instance_norm_affine_bwd(x.to(dev), dy.to(dev), scale)
    HW = H * W
    x64, dy64 = x.double(), dy.double()
    g = sty.double()[:, 1:1 + C, None, None] if scale is not None else torch.ones((B, C, 1, 1), dtype=torch.float64)
    o = sty.double()[:, 1 + C:1 + 2 * C, None, None] if bias is not None else torch.zeros((B, C, 1, 1), dtype=torch.float64)
    mean = x64.mean((2, 3), keepdim=True)
    inv = torch.rsqrt(x64.var((2, 3), unbiased=False, keepdim=True) + 1e-5)
    xh = (x64 - mean) * inv
    xh_abs = (x64.abs() + x64.abs().mean((2, 3), keepdim=True)) * inv               # the centring is a sum of |x| and |mean|
    rt = rtol_for(HW)
    assert_rounding(y, xh * g + o, xh_abs * g.abs() + o.abs(), rt, 1e-5, what="y")
    m1, m2 = dy64.mean((2, 3), keepdim=True), (dy64 * xh).mean((2, 3), keepdim=True)
    m1_abs, m2_abs = dy64.abs().mean((2, 3), keepdim=True), (dy64.abs() * xh_abs).mean((2, 3), keepdim=True)
    assert_rounding(dbias, dy64.sum((2, 3)), dy64.abs().sum((2, 3)), rt, 1e-5, what="dbias")
    assert_rounding(dscale, (dy64 * xh).sum((2, 3)), (dy64.abs() * xh_abs).sum((2, 3)), rt, 1e-5, what="dscale")
    assert_rounding(dx, g * inv * (dy64 - m1 - xh * m2), g.abs() * inv * (dy64.abs() + m1_abs + xh_abs * m2_abs), rt, 1e-5, what="dx")
    _, dscale2, dbias2 = ops.instance_norm_affine_bwd(x.to(dev), dy.to(dev), scale, need_dx=False)
    assert torch.equal(dscale2, dscale) and torch.equal(dbias2, dbias)


# ---- blur2d / upscale2d / fade-in -------------------------------------------------------------------------------------------
FIR = [[1.0, 2.0, 1.0], [2.0, 4.0, 2.0], [1.0, 2.0, 1.0]]


def _blur_ref(x64, f64, stride):
    C = x64.shape[1]
    k = f64.shape[0]
    return torch.nn.functional.conv2d(x64, f64.expand(C, 1, k, k).contiguous(), stride=stride, padding=(k - 1) // 2, groups=C)


@pytest.mark.parametrize("B,C,H,W,stride", [
    (2, 3, 9, 7, 1), (2, 3, 9, 7, 2),       # odd sizes, both strides (the old golden plane)
    (1, 4, 33, 31, 2),                       # > 256 px, odd, stride 2
    (2, 2, 20, 18, 1),                       # > 256 px, stride 1
])
def test_blur2d_fwd_bwd(ops, dev, B, C, H, W, stride):
    key = f"lgk.blur.{B}.{C}.{H}.{W}.{stride}"
    f64 = torch.tensor(FIR, dtype=torch.float64) / 16
    x = recipe_input(key + ".x", (B, C, H, W))
    y = ops.blur2d(x.to(dev), f64.float(), stride)
    f32 = f64.float().double()
    assert_rounding(y, _blur_ref(x.double(), f32, stride), _blur_ref(x.double().abs(), f32, stride), rtol_for(9), what="y")
    dy = recipe_input(key + ".dy", tuple(y.shape))
    dx = ops.blur2d_bwd(dy.to(dev), f64.float(), stride, (H, W))

    def adj(g):
        xx = torch.zeros((B, C, H, W), dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad((_blur_ref(xx, f32, stride) * g).sum(), xx)[0]
    assert_rounding(dx, adj(dy.double()), adj(dy.double().abs()), rtol_for(9), what="dx")


@pytest.mark.parametrize("B,C,H,W,factor,gain", [(2, 3, 9, 7, 2, 1.0), (1, 4, 17, 20, 2, 0.5), (2, 2, 5, 6, 4, 2.0)])
def test_upscale2d_nearest_fwd_bwd(ops, dev, B, C, H, W, factor, gain):
    key = f"lgk.up.{B}.{C}.{H}.{W}.{factor}"
    x = recipe_input(key + ".x", (B, C, H, W))
    y = ops.upscale2d_nearest(x.to(dev), factor, gain)
    ref = x.double().repeat_interleave(factor, 2).repeat_interleave(factor, 3) * gain
    assert_rounding(y, ref, ref.abs(), rtol_for(1), what="y")
    dy = recipe_input(key + ".dy", (B, C, H * factor, W * factor))
    dx = ops.upscale2d_nearest_bwd(dy.to(dev), factor, gain)
    blocks = dy.double().view(B, C, H, factor, W, factor)
    assert_rounding(dx, blocks.sum((3, 5)) * gain, blocks.abs().sum((3, 5)) * abs(gain), rtol_for(factor * factor), what="dx")


@pytest.mark.parametrize("shape,alpha", [((2, 3, 9, 7), 0.3), ((3, 16, 20, 20), 0.75), ((5, 1001), 0.0)])
def test_fade_in_tanh(ops, dev, shape, alpha):
    a, b = recipe_input(f"lgk.fade.{shape}.a", shape), recipe_input(f"lgk.fade.{shape}.b", shape)
    y = ops.fade_in_tanh(a.to(dev), b.to(dev), alpha)
    z = alpha * a.double() + (1 - alpha) * b.double()
    z_abs = (alpha * a.double()).abs() + ((1 - alpha) * b.double()).abs()
    ref = torch.tanh(z)
    # tanh's slope carries the argument's rounding; the result itself may be off by a few ulp of tanhf
    assert_rounding(y, ref, z_abs * (1 - ref.pow(2)) + 4 * ref.abs(), rtol_for(2), what="y")
