"""TEST INFRASTRUCTURE ONLY -- the case table of ``speak-hack_amd/autograd.py`` and a plain-torch composition of every
``torch.autograd.Function`` in it (tests/test_autograd_cases_cpu.py, tests/test_autograd_functions_gpu.py,
tests/test_autograd_sharing_gpu.py).  Importable without a GPU: the HIP side of a case (``Case.hip``) imports nothing until it
is called.

A case names the Function, its shapes and options; ``Case.ref(t)`` is the same operation written with ``F.conv2d`` /
``F.leaky_relu`` / ``F.interpolate`` / ``F.conv_transpose2d`` / ``oracle.modconv_ref`` / ``progan_critic_ref`` in the dtype of
its inputs, and returns ``(y, [every LeakyReLU pre-activation])``.  ``Case.subsets()`` are the sets of differentiable inputs
that require grad: every non-empty subset up to four inputs; singletons, leave-one-out sets and the full set above.

Inputs make mask flips impossible.  Plain convs draw x and w as multiples of 1/4 and the bias as an odd multiple of 1/32, so
every pre-activation is an odd multiple of 1/32 (and the fp32 forward is exact); a factor on the whole weight (1 / sigma,
``w_scale``) multiplies the bias too, which keeps that structure at any size.  Where another non-dyadic factor enters
(demodulation, random noise) ``SEEDS`` keeps, per case, the first seed for which ``min|z| >= MARGIN * rms(z)`` holds in fp64 (tests/test_autograd_cases_cpu.py asserts it for every case): fp32 summation error
is ~1e-6 of that scale, so no element can change side, nothing is masked out and the bound is rounding-level."""
from __future__ import annotations

import functools
import itertools
import math
import types
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle import modconv_ref as MR
from progan_critic_ref import minibatch_std as minibatch_std_ref

TOL_OP = 2e-5            # the project's single-op bound (tests/test_decoder_gpu.py, tests/test_encoder_backward_gpu.py)
MARGIN = 1e-4            # min|z| >= MARGIN * rms(z) over every LeakyReLU pre-activation of a case
SQRT2 = math.sqrt(2.0)

# Functions whose first-order backward is itself differentiable (the module docstring of autograd.py); ConvDgradFn and
# FCDgradFn are the recorded backwards of ConvBiasLReLUFn / FCFn and are run by THEIR second-order cases
TWICE = ("ConvBiasLReLUFn", "_LReluMaskFn", "FCFn", "GlobalAvgPoolFn", "AvgPool2xBlendFn", "AvgPool2xBlendBwdFn", "MinibatchStdFn")
TWICE_VIA = {"ConvDgradFn": "ConvBiasLReLUFn", "FCDgradFn": "FCFn"}


@dataclass(frozen=True)
class Case:
    name: str
    fn: str                    # the Function class under test
    make: object               # generator -> {name: fp64 CPU tensor}
    diff: tuple                # the inputs that can require grad
    ref: object                # {name: tensor, any dtype} -> (y, [pre-activations])
    hip: object                # (autograd module, ops module, {name: HIP fp32 tensor}) -> y
    route: object = None       # ops module -> bool: the branch this case asks for is the one taken (no device needed)
    side: bool = False         # a gated or spectrally normalised weight: weight gradients go to the second stream
    also: tuple = ()           # further Function classes the case runs
    wrt: str = "x"             # the input of the create_graph pass

    def subsets(self):
        d = self.diff
        if len(d) <= 4:
            return [c for r in range(1, len(d) + 1) for c in itertools.combinations(d, r)]
        return [(n,) for n in d] + [tuple(m for m in d if m != n) for n in d] + [d]

    @property
    def second(self):
        return "twice" if self.fn in TWICE else ("via" if self.fn in TWICE_VIA else "raise")


CASES = []


def _add(*a, **k):
    CASES.append(Case(*a, **k))


# ---- input draws -------------------------------------------------------------------------------------------------------------------
def q4(g, *shape):
    """multiples of 1/4 in [-2, 2]"""
    return torch.randint(-8, 9, shape, generator=g).double() / 4


def odd32(g, *shape):
    """odd multiples of 1/32 in (-1, 1)"""
    return (2 * torch.randint(-16, 16, shape, generator=g) + 1).double() / 32


def rnd(g, *shape):
    return torch.randn(shape, generator=g, dtype=torch.float64)


def unit(g, n):
    v = rnd(g, n)
    return v / v.norm()


def power_uv(w, g, iters=6):
    """u, v of a few fp64 power iterations on the [R, C] matrix of ``w``: sigma is then close to the largest singular value"""
    m = w.flatten(1)
    u = unit(g, m.shape[0])
    for _ in range(iters):
        v = F.normalize(m.t() @ u, dim=0)
        u = F.normalize(m @ v, dim=0)
    return u, v


# ---- shared pieces of the references -------------------------------------------------------------------------------------------------
def sn_ref(w, u, v):
    """W / sigma, sigma = u^T W v with constant u, v (torch.nn.utils.spectral_norm's hook, eval mode)"""
    return w / torch.dot(u, w.flatten(1) @ v)


def weight_ref(t, form, w_scale=1.0):
    w = sn_ref(t["weight"], t["u"], t["v"]) if form == "sn" else t["weight"]
    return w * w_scale if w_scale != 1.0 else w


def lrelu_ref(z, slope, zs):
    if slope is None or slope == 1.0:
        return z
    zs.append(z)
    return F.leaky_relu(z, slope)


def style_ref(x, style):
    if style is None:
        return x
    C = x.shape[1]
    return x * (style[:, :C, None, None] + 1) + style[:, C:, None, None]


def chan(v):
    return v.view(1, -1, 1, 1)


def up_fir_ref(x):
    """upfirdn2d(up=2, [1,3,3,1] * 4, pad (2,1)): the StyleGAN2 x2 upsample"""
    return MR.upfirdn2d(x, MR.make_kernel() * 4, up=2, down=1, pad=(2, 1))


def weight_hip(A, t, form):
    """The weight the shipped modules hand the Function: the Parameter, or W / sigma from ``spectral_norm_all`` (carries ``_spk_sn``)."""
    if form != "sn":
        return t["weight"]
    m = types.SimpleNamespace(weight_orig=t["weight"], weight_u=t["u"], weight_v=t["v"])
    return A.spectral_norm_all([m], False)[0]


def gated_hip(A, w, gated):
    """Behind a WeightGateFn when the weight requires grad (the generators gate only then), else the bare weight."""
    return A.gate_weights([w])[0] if gated and w.requires_grad else w


# ---- ConvBiasLReLUFn / ConvDgradFn as discriminator.py and progan.py call them ------------------------------------------------------------
def _conv_make(B, Cin, Cout, H, W, k, form, bias, w_scale=1.0):
    """x, w multiples of 1/4; the bias an odd multiple of 1/32 TIMES the non-dyadic factor on the weight (``w_scale``, 1 / sigma), so
    that z = factor * (a multiple of 1/16 + an odd multiple of 1/32): |z| >= factor / 32 by construction, at any size."""
    def make(g):
        t = {"x": q4(g, B, Cin, H, W) if bias else rnd(g, B, Cin, H, W), "weight": q4(g, Cout, Cin, k, k)}
        factor = w_scale
        if form == "sn":
            t["u"], t["v"] = (a.float().double() for a in power_uv(t["weight"], g))
            factor = 1 / float(torch.dot(t["u"], t["weight"].flatten(1) @ t["v"]))
        if bias:
            t["bias"] = odd32(g, Cout) * factor
        return t
    return make


def _conv_case(tag, B, Cin, Cout, H, W, k, stride, route, form, slope=0.2, bias=True):
    w_scale = math.sqrt(2.0 / (Cin * k * k)) if form == "ws" else 1.0

    def ref(t):
        zs = []
        z = F.conv2d(t["x"], weight_ref(t, form, w_scale), t.get("bias"), stride=stride, padding=(k - 1) // 2)
        return lrelu_ref(z, slope, zs), zs

    def hip(A, ops, t):
        return A.conv_bias_lrelu(t["x"], weight_hip(A, t, form), t.get("bias"), k, stride, slope, w_scale)

    _add(f"conv-{tag}-{form}", "ConvBiasLReLUFn", _conv_make(B, Cin, Cout, H, W, k, form, bias, w_scale), ("x", "weight") + (("bias",) if bias else ()),
         ref, hip, route=route, side=form == "sn", also=("ConvDgradFn", "_LReluMaskFn") + (("SpectralNormAllFn",) if form == "sn" else ()))


def _x_of(B, C, H, W):
    return torch.empty(B, C, H, W)


for _form in ("plain", "sn", "ws"):
    _conv_case("k3s1-direct", 2, 12, 8, 8, 8, 3, 1, lambda ops: ops.conv3x3_route(2, 12, 8, 8, 8)[0] == "direct"
               and ops.conv3x3_route(2, 8, 12, 8, 8)[0] == "direct", _form)
    # (the smallest shape the chooser sends to Winograd: 192 workgroups of one 32 x 8 region x 64 output channels x >= 64 input channels)
    _conv_case("k3s1-wino", 3, 256, 256, 32, 32, 3, 1, lambda ops: ops.conv3x3_route(3, 256, 256, 32, 32)[0] == "wino", _form)
    _conv_case("k3s2", 3, 16, 24, 8, 8, 3, 2, lambda ops: ops.dgrad_plan(3, 2, 3, 24, 16, (8, 8), (4, 4))[1] == 2, _form)
    _conv_case("k1s1", 2, 12, 20, 8, 8, 1, 1, lambda ops: not ops.conv1x1_expand_ok(_x_of(2, 12, 8, 8), 12, 1, 1)
               and ops.dgrad_plan(1, 1, 2, 20, 12, (8, 8), (8, 8))[1] == 1, _form)
    _conv_case("fromrgb", 2, 3, 16, 8, 8, 1, 1, lambda ops: ops.conv1x1_expand_ok(_x_of(2, 3, 8, 8), 3, 1, 1), _form)
_conv_case("k3s1-direct-noslope", 2, 12, 8, 8, 8, 3, 1, None, "ws", slope=None)
_conv_case("k3s1-direct-nobias", 2, 12, 8, 8, 8, 3, 1, None, "plain", bias=False)
_conv_case("fromrgb-odd-plane", 2, 3, 16, 5, 5, 1, 1, lambda ops: not ops.conv1x1_expand_ok(_x_of(2, 3, 5, 5), 3, 1, 1), "ws")


def _dgrad_case(tag, B, Cin, Cout, H, W, k, stride, form):
    Ho, Wo = (H + 2 * ((k - 1) // 2) - k) // stride + 1, (W + 2 * ((k - 1) // 2) - k) // stride + 1
    w_scale = math.sqrt(2.0 / (Cin * k * k)) if form == "ws" else 1.0

    def make(g):
        t = {"x": q4(g, B, Cout, Ho, Wo), "weight": q4(g, Cout, Cin, k, k)}
        if form == "sn":
            t["u"], t["v"] = power_uv(t["weight"], g)
        return t

    def ref(t):
        p = (k - 1) // 2
        op = (H + 2 * p - k) % stride
        return F.conv_transpose2d(t["x"], weight_ref(t, form, w_scale), stride=stride, padding=p, output_padding=op), []

    def hip(A, ops, t):
        return A.ConvDgradFn.apply(t["x"], weight_hip(A, t, form), k, stride, (H, W), w_scale)

    _add(f"dgrad-{tag}-{form}", "ConvDgradFn", make, ("x", "weight"), ref, hip, side=form == "sn")


_dgrad_case("k3s1", 2, 12, 8, 8, 8, 3, 1, "plain")
_dgrad_case("k3s1-wino", 3, 256, 256, 32, 32, 3, 1, "sn")
_dgrad_case("k3s2", 3, 16, 24, 8, 8, 3, 2, "ws")
_dgrad_case("k1s1", 2, 8, 12, 8, 8, 1, 1, "plain")
_dgrad_case("fromrgb", 2, 3, 16, 8, 8, 1, 1, "ws")


def _lrelu_mask_case():
    def make(g):
        return {"x": rnd(g, 3, 10, 5, 7), "y": odd32(g, 3, 10, 5, 7)}

    def ref(t):
        return t["x"] * torch.where(t["y"] > 0, 1.0, 0.2).to(t["x"].dtype), [t["y"]]

    _add("lrelu-mask", "_LReluMaskFn", make, ("x",), ref, lambda A, ops, t: A._LReluMaskFn.apply(t["x"], t["y"], 0.2))


_lrelu_mask_case()


# ---- FCFn / FCDgradFn / StyleFCGroupFn ------------------------------------------------------------------------------------------------
def _fc_case(tag, B, I, O, wmul, bmul, slope, bias=True, form="plain"):
    def make(g):
        t = {"x": q4(g, B, I) if bias else rnd(g, B, I), "weight": q4(g, O, I)}
        if bias:
            t["bias"] = odd32(g, O)
        if form == "sn":
            t["u"], t["v"] = power_uv(t["weight"], g)
        return t

    def ref(t):
        zs = []
        z = wmul * F.linear(t["x"], weight_ref(t, form))
        if bias:
            z = z + bmul * t["bias"]
        return lrelu_ref(z, slope, zs), zs

    def hip(A, ops, t):
        return A.fc(t["x"], weight_hip(A, t, form), t.get("bias"), wmul, bmul, slope)

    _add(f"fc-{tag}", "FCFn", make, ("x", "weight") + (("bias",) if bias else ()), ref, hip, also=("FCDgradFn",))


_fc_case("lrelu", 3, 40, 33, 1.0, 1.0, 0.2)                                   # dense0 of the discriminator
_fc_case("lrelu-sn", 3, 40, 33, 1.0, 1.0, 0.2, form="sn")                      # ... on W / sigma (2-D: no _spk_sn)
_fc_case("linear", 2, 33, 1, 1.0, 1.0, 1.0)                                   # dense1
_fc_case("mults", 3, 24, 20, 0.125 * SQRT2, 0.01 * SQRT2, 0.2)                # EqualLinear with the folded gain
_fc_case("relu", 2, 24, 20, math.sqrt(2.0 / 24), 1.0, 0.0)                                   # progan's WSLinear(relu)
_fc_case("nobias", 2, 24, 20, 0.5, 1.0, 0.2, bias=False)
_fc_case("critic-valid4x4", 2, 16 * 12, 10, math.sqrt(2.0 / (12 * 16)), 1.0, 0.2)   # the critic's 4x4 valid conv (_valid4x4_fc)


def _fc_dgrad_case():
    B, I, O, wmul, slope = 3, 24, 20, 0.25, 0.2

    def make(g):
        return {"x": rnd(g, B, O), "out": odd32(g, B, O), "weight": q4(g, O, I)}

    def ref(t):
        m = torch.where(t["out"] > 0, 1.0, slope).to(t["x"].dtype)
        return wmul * (t["x"] * m) @ t["weight"], [t["out"]]

    _add("fc-dgrad", "FCDgradFn", make, ("x", "weight"), ref, lambda A, ops, t: A.FCDgradFn.apply(t["x"], t["out"], t["weight"], wmul, slope))


_fc_dgrad_case()


def _style_group_case(tag, rows, used, slope, biases):
    B, I, n = 2, 24, 3
    Os = (16, 20, 8)
    confs = tuple((0.25, 0.5, slope, b) for b in biases)

    def make(g):
        t = {"x": q4(g, B, rows, I)}
        for j in range(n):
            t[f"weight{j}"] = q4(g, Os[j], I)
            if biases[j]:
                t[f"bias{j}"] = odd32(g, Os[j]) * 2
        return t

    def ref(t):
        zs, outs = [], []
        for j in used:
            z = 0.25 * F.linear(t["x"][:, j], t[f"weight{j}"])
            if biases[j]:
                z = z + 0.5 * t[f"bias{j}"]
            outs.append(lrelu_ref(z, slope, zs).flatten())
        return torch.cat(outs), zs

    def hip(A, ops, t):
        params = [t.get(f"{k}{j}") for j in range(n) for k in ("weight", "bias")]
        outs = A.StyleFCGroupFn.apply(t["x"], confs, torch.is_grad_enabled(), *params)
        return torch.cat([outs[j].flatten() for j in used])

    diff = ("x",) + tuple(f"{k}{j}" for j in used for k in ("weight", "bias") if k == "weight" or biases[j])
    _add(f"stylefc-{tag}", "StyleFCGroupFn", make, diff, ref, hip)


_style_group_case("all", 3, (0, 1, 2), 0.2, (True, True, True))
_style_group_case("more-rows", 5, (0, 1, 2), 0.2, (True, True, True))           # a latent with more rows than layers
_style_group_case("one-unused", 3, (0, 2), 0.2, (True, True, True))             # douts[1] is None
_style_group_case("linear-nobias1", 3, (0, 1, 2), 1.0, (True, False, True))     # stylegan2's modulations: slope 1


# ---- FusedConvFn ------------------------------------------------------------------------------------------------------------------------
def _fused_case(tag, B, Cin, Cout, Hs, upsample, route, gated=False, bias=True, noise=True, style=True, slope=0.2, w_scale=1.0, coarse=False):
    H = 2 * Hs if upsample else Hs

    def make(g):
        if coarse:      # a plane count at which no seed keeps a random margin: x on the 1/2 grid and w in {-1, 0, 1} put conv(up(x)) on
            # the 1/32 grid (bilinear weights are k/16), noise_w * noise as well; the bias is an odd multiple of 1/64
            t = {"x": torch.randint(-2, 3, (B, Cin, Hs, Hs), generator=g).double() / 2, "weight": torch.randint(-1, 2, (Cout, Cin, 3, 3), generator=g).double(),
                 "bias": odd32(g, Cout) / 2, "noise_w": q4(g, Cout), "noise": torch.randint(-16, 17, (B, 1, H, H), generator=g).double() / 8}
            assert bias and noise
            if style:
                t["style"] = q4(g, B, 2 * Cout) / 4
            return t
        t = {"x": q4(g, B, Cin, Hs, Hs) if bias else rnd(g, B, Cin, Hs, Hs), "weight": q4(g, Cout, Cin, 3, 3)}
        if bias:
            t["bias"] = odd32(g, Cout)
        if noise:
            t["noise_w"], t["noise"] = q4(g, Cout) / 4, rnd(g, B, 1, H, H)
        if style:
            t["style"] = q4(g, B, 2 * Cout) / 4
        return t

    def ref(t):
        zs = []
        x = F.interpolate(t["x"], scale_factor=2, mode="bilinear", align_corners=False) if upsample else t["x"]
        z = F.conv2d(x, t["weight"] * w_scale, t.get("bias"), padding=1)
        if noise:
            z = z + chan(t["noise_w"]) * t["noise"]
        return style_ref(lrelu_ref(z, slope, zs), t.get("style")), zs

    def hip(A, ops, t):
        return A.fused_conv(t["x"], gated_hip(A, t["weight"], gated), t.get("bias"), t.get("noise_w"), t.get("noise"), t.get("style"),
                            upsample, slope, ops.PackedConvWeight(), w_scale)

    diff = ("x", "weight") + (("bias",) if bias else ()) + (("noise_w",) if noise else ()) + (("style",) if style else ())
    _add(f"fused-{tag}", "FusedConvFn", make, diff, ref, hip, route=route, side=gated, also=("WeightGateFn",) if gated else ())


def _fused_route(kind, B, Cin, Cout, H):
    return lambda ops: ops.conv3x3_route(B, Cin, Cout, H, H)[0] == kind


_fused_case("up-wino-gated", 4, 256, 256, 16, True, lambda ops: ops.conv3x3_route(4, 256, 256, 32, 32)[0] == "wino"
            and ops.use_wgrad_wino(4, 256, 256, 32, 32), gated=True, coarse=True)                              # keeps the x2 image
_fused_case("up-direct", 2, 12, 8, 4, True, _fused_route("direct", 2, 12, 8, 8))
_fused_case("up-direct-odd", 2, 12, 8, 5, True, _fused_route("direct", 2, 12, 8, 10))
_fused_case("wino", 3, 256, 256, 32, False, lambda ops: ops.conv3x3_route(3, 256, 256, 32, 32)[0] == "wino"
            and not ops.use_wgrad_wino(3, 256, 256, 32, 32), coarse=True)
_fused_case("direct-gated", 3, 12, 8, 8, False, _fused_route("direct", 3, 12, 8, 8), gated=True)
_fused_case("nobias", 2, 12, 8, 8, False, None, bias=False)
_fused_case("nonoise", 2, 12, 8, 8, False, None, noise=False)
_fused_case("nostyle-ws", 2, 12, 8, 8, False, None, style=False, w_scale=math.sqrt(2.0 / (12 * 9)))      # progan's WSConv2d
_fused_case("up-nostyle-ws-noslope", 2, 12, 8, 4, True, None, style=False, slope=None, w_scale=math.sqrt(2.0 / (12 * 9)))
_fused_case("bare", 2, 12, 8, 8, False, None, bias=False, noise=False, style=False)


# ---- ModConvFn / ModToRGBFn / UpFirDnFn ---------------------------------------------------------------------------------------------------
def _mod_case(tag, B, Cin, Cout, Hs, upsample, route, gated=False, demodulate=True, bias=True, noise=True, slope=0.2):
    H = 2 * Hs if upsample else Hs
    scale = 1 / math.sqrt(Cin * 9)

    def make(g):
        t = {"x": q4(g, B, Cin, Hs, Hs), "weight": q4(g, Cout, Cin, 3, 3), "s": 1 + q4(g, B, Cin) / 8}
        if bias:
            t["bias"] = odd32(g, Cout)
        if noise:
            t["noise_w"], t["noise"] = q4(g, Cout) / 4, rnd(g, B, 1, H, H)
        return t

    def ref(t):
        zs = []
        z = MR.modulated_conv2d(up_fir_ref(t["x"]) if upsample else t["x"], t["weight"], t["s"], demodulate)
        if noise:
            z = z + chan(t["noise_w"]) * t["noise"]
        if bias:
            z = z + chan(t["bias"])
        return (SQRT2 * lrelu_ref(z, slope, zs) if slope is not None else z), zs      # (the gain is the activation's: none without one)

    def hip(A, ops, t):
        fir = MR.make_kernel() * 4.0
        return A.mod_conv(t["x"], gated_hip(A, t["weight"], gated), t["s"], t.get("bias"), t.get("noise_w"), t.get("noise"), scale,
                          upsample, slope, SQRT2, fir, ops.PackedConvWeight(), demodulate)

    diff = ("x", "weight", "s") + (("bias",) if bias else ()) + (("noise_w",) if noise else ())
    _add(f"modconv-{tag}", "ModConvFn", make, diff, ref, hip, route=route, side=gated, also=("WeightGateFn",) if gated else ())


def _mod_route(want, B, Cin, Cout, H, upsample):
    return lambda ops: bool(ops.wgrad_mod_supported(B, Cin, Cout, H, H, upsample)) == want


_mod_case("fused-wgrad", 2, 16, 24, 16, False, _mod_route(True, 2, 16, 24, 16, False))
_mod_case("fused-wgrad-up-gated", 2, 16, 24, 8, True, _mod_route(True, 2, 16, 24, 16, True), gated=True)
_mod_case("tiny-4x4", 2, 16, 12, 4, False, _mod_route(False, 2, 16, 12, 4, False))
_mod_case("tiny-4x4-gated", 2, 16, 12, 4, False, _mod_route(False, 2, 16, 12, 4, False), gated=True)
_mod_case("odd-5x5-up", 2, 16, 12, 5, True, None)
_mod_case("nodemod", 2, 16, 24, 16, False, None, demodulate=False)
_mod_case("nodemod-tiny", 2, 16, 12, 4, False, None, demodulate=False)
_mod_case("nobias", 2, 16, 24, 16, False, None, bias=False)
_mod_case("nonoise-noslope", 2, 16, 24, 16, False, None, noise=False, slope=None)


def _torgb_mod_case(tag, B, C, H, skip, bias=True):
    scale = 1 / math.sqrt(C)

    def make(g):
        t = {"x": q4(g, B, C, H, H), "weight": q4(g, 3, C, 1, 1), "s": 1 + q4(g, B, C) / 8}
        if bias:
            t["bias"] = odd32(g, 3)
        if skip:
            t["skip"] = q4(g, B, 3, H // 2, H // 2)
        return t

    def ref(t):
        y = MR.modulated_conv2d(t["x"], t["weight"], t["s"], False)
        if bias:
            y = y + chan(t["bias"])
        return (y + up_fir_ref(t["skip"]) if skip else y), []

    def hip(A, ops, t):
        return A.mod_to_rgb(t["x"], t["weight"], t["s"], t.get("bias"), scale, t.get("skip"), MR.make_kernel() * 4.0)

    diff = ("x", "weight", "s") + (("bias",) if bias else ()) + (("skip",) if skip else ())
    _add(f"modtorgb-{tag}", "ModToRGBFn", make, diff, ref, hip)


_torgb_mod_case("skip", 2, 24, 8, True)
_torgb_mod_case("noskip", 3, 24, 6, False)
_torgb_mod_case("skip-nobias", 2, 12, 16, True, bias=False)


def _upfirdn_case(tag, B, C, H, up, down, pad):
    def ref(t):
        return MR.upfirdn2d(t["x"], MR.make_kernel() * (up ** 2), up=up, down=down, pad=pad), []

    _add(f"upfirdn-{tag}", "UpFirDnFn", lambda g: {"x": rnd(g, B, C, H, H)}, ("x",), ref,
         lambda A, ops, t: A.upfirdn(t["x"], MR.make_kernel() * (up ** 2), up, down, pad))


_upfirdn_case("up2-pad21", 2, 3, 8, 2, 1, (2, 1))          # stylegan2.Upsample: the one (up, down, pad) the module uses
_upfirdn_case("up2-pad21-odd", 3, 5, 7, 2, 1, (2, 1))


# ---- the decoder's small ops ------------------------------------------------------------------------------------------------------------
def _torgb_case(tag, B, C, H, W, bias):
    def make(g):
        t = {"x": q4(g, B, C, H, W), "weight": q4(g, 3, C, 1, 1)}
        if bias:
            t["bias"] = odd32(g, 3)
        return t

    _add(f"torgb-{tag}", "ToRGBFn", make, ("x", "weight") + (("bias",) if bias else ()),
         lambda t: (F.conv2d(t["x"], t["weight"], t.get("bias")), []), lambda A, ops, t: A.to_rgb(t["x"], t["weight"], t.get("bias")))


_torgb_case("bias", 2, 24, 8, 8, True)
_torgb_case("nobias-odd", 3, 10, 5, 7, False)


def _bns_case(tag, B, C, H, broadcast, bias, noise, style):
    def make(g):
        t = {"x": rnd(g, 1 if broadcast else B, C, H, H)}
        if bias:
            t["bias"] = rnd(g, C)
        if noise:
            t["noise_w"], t["noise"] = rnd(g, C), rnd(g, B, 1, H, H)
        if style:
            t["style"] = rnd(g, B, 2 * C) / 2
        return t

    def ref(t):
        y = t["x"].expand(B, -1, -1, -1)
        if bias:
            y = y + chan(t["bias"])
        if noise:
            y = y + chan(t["noise_w"]) * t["noise"]
        return style_ref(y, t.get("style")), []

    def hip(A, ops, t):
        return A.bias_noise_style(t["x"], t.get("bias"), t.get("noise_w"), t.get("noise"), t.get("style"), B)

    diff = ("x",) + (("bias",) if bias else ()) + (("noise_w",) if noise else ()) + (("style",) if style else ())
    _add(f"bns-{tag}", "BiasNoiseStyleFn", make, diff, ref, hip)


_bns_case("const-broadcast", 3, 10, 4, True, True, True, True)       # the decoder prologue: [1,C,4,4] over B > 1
_bns_case("all", 2, 10, 6, False, True, True, True)
_bns_case("noise-only", 2, 10, 6, False, False, True, False)         # ApplyNoise
_bns_case("style-only", 2, 10, 6, False, False, False, True)         # ApplyStyle
_bns_case("bias-only-broadcast", 2, 10, 4, True, True, False, False)


def _simple(name, fn, shape, ref, hip, **kw):
    _add(name, fn, lambda g: {"x": rnd(g, *shape)}, ("x",), lambda t: (ref(t["x"]), []), lambda A, ops, t: hip(A, t["x"]), **kw)


def _inorm_ref(x, eps):
    return (x - x.mean((2, 3), keepdim=True)) / torch.sqrt(x.var((2, 3), unbiased=False, keepdim=True) + eps)


def _inorm_case(tag, affine):
    B, C, H, W, eps = 2, 10, 6, 7, 1e-5

    def make(g):
        t = {"x": rnd(g, B, C, H, W)}
        if affine:
            t["scale"], t["bias"] = rnd(g, B, C), rnd(g, B, C)
        return t

    def ref(t):
        y = _inorm_ref(t["x"], eps)
        return (y * t["scale"][:, :, None, None] + t["bias"][:, :, None, None] if affine else y), []

    _add(f"inorm-{tag}", "InstanceNormAffineFn", make, ("x", "scale", "bias") if affine else ("x",), ref,
         lambda A, ops, t: A.instance_norm_affine(t["x"], t.get("scale"), t.get("bias"), eps))


_inorm_case("adain", True)
_inorm_case("plain", False)
_simple("upsample2x", "Upsample2xFn", (2, 5, 6, 7), lambda x: F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False),
        lambda A, x: A.upsample2x(x))
for _sq in (False, True):
    _simple(f"pixelnorm-{'sqrt' if _sq else 'rsqrt'}", "PixelNormFn", (3, 20, 4, 5), lambda x: x * torch.rsqrt((x * x).mean(1, keepdim=True) + 1e-8),
            lambda A, x, _sq=_sq: A.pixelnorm(x, 1e-8, _sq))
_simple("pixelnorm-2d", "PixelNormFn", (3, 40), lambda x: x * torch.rsqrt((x * x).mean(1, keepdim=True) + 1e-8), lambda A, x: A.pixelnorm(x, 1e-8, False))


def _blur_filter():
    f = torch.tensor([1.0, 2.0, 1.0])
    f = f[:, None] * f[None, :]
    return f / f.sum()


for _st, _hw in ((1, 7), (2, 8), (2, 7)):
    _simple(f"blur-s{_st}-{_hw}", "Blur2dFn", (2, 6, _hw, _hw),
            lambda x, _st=_st: F.conv2d(x, _blur_filter().to(x.dtype)[None, None].expand(x.shape[1], 1, 3, 3), stride=_st, padding=1, groups=x.shape[1]),
            lambda A, x, _st=_st: A.blur2d(x, _blur_filter(), _st))
_simple("upscale2d", "Upscale2dFn", (2, 5, 3, 5), lambda x: 1.5 * x.repeat_interleave(2, 2).repeat_interleave(2, 3), lambda A, x: A.upscale2d(x, 2, 1.5))


def _fused_upscale_case(tag, B, Cin, Cout, H, bias):
    def make(g):
        t = {"x": q4(g, B, Cin, H, H), "weight": q4(g, Cin, Cout, 4, 4)}
        if bias:
            t["bias"] = odd32(g, Cout)
        return t

    _add(f"fusedup-{tag}", "FusedUpscaleFn", make, ("x", "weight") + (("bias",) if bias else ()),
         lambda t: (F.conv_transpose2d(t["x"], t["weight"], t.get("bias"), stride=2, padding=1), []),
         lambda A, ops, t: A.fused_upscale(t["x"], t["weight"], t.get("bias"), ops.PackedConvWeight()))


_fused_upscale_case("bias", 2, 16, 24, 8, True)
_fused_upscale_case("nobias", 2, 16, 8, 5, False)


# ---- the discriminators' pooling ops --------------------------------------------------------------------------------------------------------
_simple("gap", "GlobalAvgPoolFn", (3, 10, 5, 7), lambda x: F.adaptive_avg_pool2d(x, 1), lambda A, x: A.global_avgpool(x))
_simple("mbstd", "MinibatchStdFn", (3, 10, 4, 4), minibatch_std_ref, lambda A, x: A.minibatch_std(x))


def _pool_case(tag, z, a, b):
    def make(g):
        t = {"x": rnd(g, 2, 6, 8, 6)}
        if z:
            t["z"] = rnd(g, 2, 6, 4, 3)
        return t

    def ref(t):
        y = a * F.avg_pool2d(t["x"], 2, 2)
        return (y + b * t["z"] if z else y), []

    _add(f"pool-{tag}", "AvgPool2xBlendFn", make, ("x", "z") if z else ("x",), ref,
         lambda A, ops, t: A.avgpool2x_blend(t["x"], t.get("z"), a, b), also=("AvgPool2xBlendBwdFn",))


_pool_case("plain", False, 1.0, 0.0)
_pool_case("blend", True, 0.3, 0.7)


def _pool_bwd_case(tag, a, b):
    def ref(t):
        dx = (a / 4) * t["x"].repeat_interleave(2, 2).repeat_interleave(2, 3)
        return (dx if b is None else torch.cat([dx.flatten(), (b * t["x"]).flatten()])), []

    def hip(A, ops, t):
        out = A.AvgPool2xBlendBwdFn.apply(t["x"], a, b)
        return out if b is None else torch.cat([out[0].flatten(), out[1].flatten()])

    _add(f"poolbwd-{tag}", "AvgPool2xBlendBwdFn", lambda g: {"x": rnd(g, 2, 6, 4, 3)}, ("x",), ref, hip, also=("AvgPool2xBlendFn",))


_pool_bwd_case("plain", 1.0, None)
_pool_bwd_case("blend", 0.3, 0.7)


# ---- SpectralNormAllFn / WeightGateFn on their own ------------------------------------------------------------------------------------------------
def _sn_case(tag, training):
    shapes = ((12, 8, 3, 3), (10, 24))

    def make(g):
        t = {}
        for i, s in enumerate(shapes):
            t[f"weight{i}"] = q4(g, *s)
            t[f"u{i}"], t[f"v{i}"] = power_uv(t[f"weight{i}"], g, iters=2)
        return t

    def ref(t):
        outs = []
        for i in range(len(shapes)):
            w, u, v = t[f"weight{i}"], t[f"u{i}"], t[f"v{i}"]
            if training:              # one power iteration first, on the detached matrix (the hook runs it under no_grad)
                m = w.detach().flatten(1)
                v = F.normalize(m.t() @ u, dim=0, eps=1e-12)
                u = F.normalize(m @ v, dim=0, eps=1e-12)
            outs.append(sn_ref(w, u, v).flatten())
        return torch.cat(outs), []

    def hip(A, ops, t):
        mods = [types.SimpleNamespace(weight_orig=t[f"weight{i}"], weight_u=t[f"u{i}"].clone(), weight_v=t[f"v{i}"].clone())
                for i in range(len(shapes))]
        return torch.cat([h.flatten() for h in A.spectral_norm_all(mods, training)])

    _add(f"sn-{tag}", "SpectralNormAllFn", make, tuple(f"weight{i}" for i in range(len(shapes))), ref, hip, wrt="weight0")


_sn_case("eval", False)
_sn_case("train", True)


def _gate_case():
    def make(g):
        return {"weight0": rnd(g, 8, 6, 3, 3), "weight1": rnd(g, 4, 8, 3, 3)}

    _add("gate", "WeightGateFn", make, ("weight0", "weight1"), lambda t: (torch.cat([t["weight0"].flatten(), t["weight1"].flatten()]), []),
         lambda A, ops, t: torch.cat([w.flatten() for w in A.gate_weights([t["weight0"], t["weight1"]])]), wrt="weight0", side=True)


_gate_case()

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the first seed (> 0) for which the margin assertion holds, for the cases where seed 0 does not (found on the CPU:
# ``python tests/autograd_cases.py`` prints this table)
SEEDS = {
    "fused-up-direct-odd": 1,
    "modconv-fused-wgrad-up-gated": 1,
    "modconv-nodemod": 1,
    "modconv-nobias": 1,
}


def is_param(name):
    """The inputs that are ``nn.Parameter``s in the shipped modules (``_first_or_add`` and the spectral-norm notes key on that)."""
    return name.startswith(("weight", "bias", "noise_w"))


def draw(case, seed):
    g = torch.Generator().manual_seed(seed)
    t = {k: v.float().double() for k, v in case.make(g).items()}            # every value is an fp32 number
    y, _ = case.ref(t)
    t["c"] = rnd(g, *y.shape).float().double()
    return t


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return draw(BY_NAME[name], SEEDS.get(name, 0))


def inputs(name):
    """{input name: fp64 CPU tensor} of a case, plus the fixed random ``c`` of ``loss = (y * c).sum()``: fresh copies."""
    return {k: v.clone() for k, v in _inputs(name).items()}


def margin(case, t):
    """min over the case's pre-activations of min|z| / rms(z) in fp64 (inf without a LeakyReLU)."""
    _, zs = case.ref(t)
    return min((float(z.abs().min() / z.pow(2).mean().sqrt()) for z in zs), default=math.inf)


def leaves(t, diff, dtype=None, device=None, req=None, c_grad=False):
    """The case's tensors as autograd leaves: ``req`` (default: all of ``diff``) require grad, the Parameters of the shipped
    modules are Parameters."""
    req = diff if req is None else req
    out = {}
    for k, v in t.items():
        v = v.to(dtype=dtype, device=device).clone()
        need = k in req or (k == "c" and c_grad)
        out[k] = torch.nn.Parameter(v, requires_grad=need) if (is_param(k) and k in diff) else v.requires_grad_(need)
    return out


def first_order(run, t, names):
    """(y, {name: d (y * c).sum() / d name}) of ``run(t) -> y``."""
    y = run(t)
    gs = torch.autograd.grad((y * t["c"]).sum(), [t[n] for n in names], allow_unused=True)
    return y.detach(), dict(zip(names, gs))


def second_order(run, t, wrt, names):
    """g = grad((y * c).sum(), wrt, create_graph=True); P = (g * g).sum(); -> (g, {name: dP / d name}) (None: unused)."""
    y = run(t)
    (g,) = torch.autograd.grad((y * t["c"]).sum(), t[wrt], create_graph=True)
    gs = torch.autograd.grad((g * g).sum(), [t[n] for n in names], allow_unused=True)
    return g.detach(), dict(zip(names, gs))


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """The composition in ``dtype`` on the CPU: {"y", "grads", and for the twice-differentiable Functions "g", "grads2"}.  Computed
    once per case and dtype; callers must not modify it."""
    case = BY_NAME[name]
    run = lambda t: case.ref(t)[0]
    y, grads = first_order(run, leaves(inputs(name), case.diff, dtype), case.diff)
    out = {"y": y, "grads": grads}
    if case.second == "twice":
        names = case.diff + ("c",)
        out["g"], out["grads2"] = second_order(run, leaves(inputs(name), case.diff, dtype, c_grad=True), case.wrt, names)
    return out


def bound(e32):
    """TOL_OP, or 4x the fp32 composition's own error where that is worse than a quarter of TOL_OP."""
    return 4 * e32 if e32 > TOL_OP / 4 else TOL_OP


if __name__ == "__main__":       # the seed table: first seed per case whose margin holds
    for case in CASES:
        for seed in range(200):
            if margin(case, draw(case, seed)) >= MARGIN:
                break
        else:
            raise SystemExit(f"{case.name}: no seed below 200 keeps the margin")
        if seed:
            print(f'    "{case.name}": {seed},')
