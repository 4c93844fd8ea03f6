"""Case table and fp64 reference of the weight gradient (csrc/wgrad_mfma_f32.hip, the Winograd route for its routing only) -- test
infrastructure, CPU only; the role tests/direct_conv_cases.py has for the forward conv.

A case names a launch (shape, mode, groups, fold, requested splits, scale / accumulate, which tensors sit 4 bytes off a 16-byte
boundary) and DECLARES the form it reaches; ``spk_conv2d_wgrad_launch_form`` -- the launch path's own statements -- decides whether
it does (tests/test_wgrad_forms_cpu.py without a GPU, tests/test_wgrad_branches_gpu.py again with the real pointers).

``reference(case)`` is the operator in fp64 on the CPU and, the same chain, in fp32: the input stage (affine + ReLU with a ZERO
halo | batch scale | bilinear x2 | upfirdn2d(up=2, [1,3,3,1]) of x * s with g * d'), torch.autograd through F.conv2d per group,
then fold, scale and accumulate.  The bound is measured on the reference, never on the kernel:
max(4 x rel-L2(fp32 chain, fp64 chain), sqrt(B H W) 2^-24) -- the rule of tests/direct_conv_cases.py with this operator's reduction
length; a single element: |dw - ref| <= MAX_FACTOR x bound x rms(ref).

Scope: the shipped dispatch: the switches the library reads once per process (ENV_SWITCHES) are assumed unset, and
``require_default_dispatch`` fails if one is set."""
import functools
import math
import os

import torch
import torch.nn.functional as F

from oracle.weights_recipe import recipe_input, recipe_tensor

TOL_OP = 2e-5                   # the aggregate rel-L2 of tests/test_backward_gpu.py: no case's bound may exceed it
MAX_FACTOR = 8.0                # as tests/bf16x3_emulation.py
GUARD = 64                      # NaN floats on either side of dw and behind the workspace
ENV_SWITCHES = ("SPK_WGRAD_WIDE", "SPK_WGRAD_S2", "SPK_WGRAD_PIPE", "SPK_WGRAD_FIXED", "SPK_WGRAD1X1_DMA", "SPK_WGRAD_STEM", "SPK_WGRAD_WINO_WGS")
KERNELS = ("tap", "tap_fixed", "pipe", "wide16", "wide8", "s2_16", "s2_8", "up", "gemm1x1", "gemm1x1_dma", "stem", "wino")     # SPK_WGRAD_*
MODES = ("plain", "affine", "bscale")
REDUCERS = ("dword", "vec", "deep")


def require_default_dispatch():
    """The case table is written for the shipped dispatch: fail (never skip) if a switch the library reads is set."""
    for name in ENV_SWITCHES:
        assert name not in os.environ, f"{name} is set: the weight-gradient case table assumes the shipped dispatch (unset it)"


def case(name, k, stride, B, Cin, Cout, Hs, Ws, mode="plain", up=None, G=1, shared=False, fold=1, splits=0, scale=1.0, accumulate=False,
         misalign=(), wino=False, **declares):
    """``Cin`` / ``Cout`` per group; ``Hs x Ws``: the size of x (the LOW-resolution tensor when ``up`` = "bilinear" | "fir").
    ``misalign``: of g / x / dw, the tensors that start 4 bytes off.  ``declares``: fields of spk_wgrad_form the case says it
    reaches, ``kernel`` / ``reducer`` by name."""
    assert mode in MODES and up in (None, "bilinear", "fir") and set(misalign) <= {"g", "x", "dw"} and "kernel" in declares
    return dict(name=name, k=k, stride=stride, B=B, Cin=Cin, Cout=Cout, Hs=Hs, Ws=Ws, mode=mode, up=up, G=G, shared=shared, fold=fold,
                splits=splits, scale=scale, accumulate=accumulate, misalign=frozenset(misalign), wino=wino, declares=declares)


def out_hw(c):
    if c["up"]:
        return 2 * c["Hs"], 2 * c["Ws"]
    k, s, p = c["k"], c["stride"], (c["k"] - 1) // 2
    return (c["Hs"] + 2 * p - k) // s + 1, (c["Ws"] + 2 * p - k) // s + 1


def x_channels(c):
    return c["Cin"] if (c["shared"] or c["G"] == 1) else c["G"] * c["Cin"]


def dw_shape(c):
    return (c["G"] // c["fold"] * c["Cout"], c["Cin"], c["k"], c["k"])


# ---- operands ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = BY_NAME[name]
    B, H, W = c["B"], *out_hw(c)
    Cx, Cy, tag = x_channels(c), c["G"] * c["Cout"], f"wgc.{name}"
    t = dict(x=recipe_input(f"{tag}.x", (B, Cx, c["Hs"], c["Ws"])), g=recipe_input(f"{tag}.g", (B, Cy, H, W)))
    if c["mode"] == "affine":              # shifts of both signs: a halo of relu(shift) instead of 0 must show
        t["a"] = 1.0 + 0.3 * recipe_input(f"{tag}.a", (Cx,))
        t["b"] = 0.5 * recipe_input(f"{tag}.b", (Cx,))
        t["b"][0], t["b"][1] = t["b"][0].abs(), -t["b"][1].abs()
    if c["mode"] == "bscale":
        t["s"] = 1.0 + 0.3 * recipe_input(f"{tag}.s", (B, Cx), "uniform")
        t["d"] = 0.5 + recipe_input(f"{tag}.d", (B, Cy), "uniform").abs()
    if c["accumulate"]:
        t["base"] = recipe_tensor(f"{tag}.base", dw_shape(c), 1.0)
    return t


def inputs(c):
    return _inputs(c["name"])


# ---- the operator chain ----------------------------------------------------------------------------------------------------------
def upfirdn_x2(x):
    """upfirdn2d(up=2, [1,3,3,1] (x) [1,3,3,1] * 4 / 64, pad (2,1)): zero-stuffed, zero border."""
    B, Cc, H, W = x.shape
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=x.dtype)
    k = (k1[:, None] * k1[None, :]) / 64.0 * 4.0
    up = torch.zeros(B, Cc, 2 * H, 2 * W, dtype=x.dtype)
    up[:, :, ::2, ::2] = x
    return F.conv2d(F.pad(up, (2, 1, 2, 1)), k.flip(0, 1).view(1, 1, 4, 4).repeat(Cc, 1, 1, 1), groups=Cc)


def _wgrad(xin, g, c, padding=None):
    """[G Cout, Cin, k, k]: autograd through F.conv2d, group by group."""
    Cin, Cout, k = c["Cin"], c["Cout"], c["k"]
    out = []
    for q in range(c["G"]):
        xq = xin if (c["shared"] or c["G"] == 1) else xin[:, q * Cin:(q + 1) * Cin]
        w = torch.zeros(Cout, Cin, k, k, dtype=xin.dtype, requires_grad=True)
        y = F.conv2d(xq, w, stride=c["stride"], padding=(k - 1) // 2 if padding is None else padding)
        y.backward(g[:, q * Cout:(q + 1) * Cout].contiguous())
        out.append(w.grad)
    return torch.cat(out, 0)


def fold_groups(dw, c, wrong_pairing=False):
    """Groups q and q + G/fold share their weights: their gradients add."""
    G, fold, Cout = c["G"], c["fold"], c["Cout"]
    if fold == 1:
        return dw
    v = dw.view(G, Cout, *dw.shape[1:])
    if wrong_pairing:          # q with q + 1
        return v.view(G // fold, fold, Cout, *dw.shape[1:]).sum(1).reshape(G // fold * Cout, *dw.shape[1:])
    return v.view(fold, G // fold, Cout, *dw.shape[1:]).sum(0).reshape(G // fold * Cout, *dw.shape[1:])


def chain(c, dtype, fault=None, form=None):
    """dw of the whole operator in ``dtype``.  ``fault`` seeds one of the faults of the sensitivity checks (``form``: the launch
    form, for the faults that speak of tiles and splits)."""
    t = inputs(c)
    x, g = t["x"].to(dtype), t["g"].to(dtype)
    H, W = out_hw(c)
    k, pad = c["k"], (c["k"] - 1) // 2
    padding = None
    if c["mode"] == "affine":
        a, b = t["a"].to(dtype).view(1, -1, 1, 1), t["b"].to(dtype).view(1, -1, 1, 1)
        x = torch.relu(x * a + b)
        if fault == "halo_relu_shift":     # the halo filled with relu(0 * a + b) instead of 0
            halo = torch.relu(b).expand(x.shape[0], -1, x.shape[2] + 2 * pad, x.shape[3] + 2 * pad).clone()
            halo[:, :, pad:pad + x.shape[2], pad:pad + x.shape[3]] = x
            x, padding = halo, 0
    if c["mode"] == "bscale":
        x = x * t["s"].to(dtype).view(x.shape[0], -1, 1, 1)
        if fault != "no_g_scale":
            g = g * t["d"].to(dtype).view(g.shape[0], -1, 1, 1)
    if c["up"] == "bilinear":
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        if fault == "bilinear_border":     # the top border clamped one source row wrong: row 0 interpolated like row 1
            x = x.clone()
            x[:, :, 0] = x[:, :, 1]
    elif c["up"] == "fir":
        x = upfirdn_x2(x)
    if fault == "last_tile_lost":          # the pixels of the last tile (the last split's last visit) never added
        g = g.clone()
        if form["TW"]:
            g[-1, :, (H - 1) // form["TH"] * form["TH"]:, (W - 1) // form["TW"] * form["TW"]:] = 0
        else:                              # GEMM form: the last split's 32-pixel k-tiles of the flattened (b, pixel) axis
            lost = (form["n_tiles"] - (form["splits"] - 1) * form["tiles_per_split"]) * 32
            flat = g.permute(1, 0, 2, 3).reshape(g.shape[1], -1)
            flat[:, -lost:] = 0
            g = flat.view(g.shape[1], g.shape[0], H, W).permute(1, 0, 2, 3).contiguous()
    dw = _wgrad(x, g, c, padding)
    if fault == "border_row":              # tap row ky = 0 without the last output row (it reads input row H - 2: in range)
        last = torch.zeros_like(g)
        last[:, :, H - 1] = g[:, :, H - 1]
        dw = dw.clone()
        dw[:, :, 0] -= _wgrad(x, last, c, padding)[:, :, 0]
    if fault == "taps_transposed":
        dw = dw.transpose(2, 3).contiguous()
    if fault == "ragged_rows":             # the rows of the last, partly filled, 64-channel block of every group
        dw = dw.clone()
        dw.view(c["G"], c["Cout"], *dw.shape[1:])[:, c["Cout"] // 64 * 64:] = 0
    dw = fold_groups(dw, c, wrong_pairing=fault == "fold_neighbour")
    sc = float(torch.tensor(c["scale"], dtype=torch.float32))
    dw = dw * sc
    if c["accumulate"]:
        dw = dw + t["base"].to(dtype)
    return dw


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = BY_NAME[name]
    dw, dw32 = chain(c, torch.float64), chain(c, torch.float32)
    H, W = out_hw(c)
    bound = max(4 * rel_l2(dw32, dw), math.sqrt(c["B"] * H * W) * 2.0 ** -24)
    return dict(dw=dw, dw32=dw32, bound=bound)


def reference(c):
    """fp64 result ``dw``, the fp32 chain ``dw32`` and the case's ``bound``.  Shared: do not write."""
    return _reference(c["name"])


def figures(c, dw):
    """-> {what: (figure, limit)}: every figure must stay at or below its limit."""
    ref = reference(c)
    got, want = dw.detach().cpu().double(), ref["dw"]
    assert got.shape == want.shape, (got.shape, want.shape)
    return {"dw rel-L2": (rel_l2(got, want), ref["bound"]),
            "dw max|diff|": (float((got - want).abs().max()), MAX_FACTOR * ref["bound"] * rms(want))}


# ---- the descriptor, for the query without a device --------------------------------------------------------------------------------
def flags_of(c, L):
    return ((L.CONV_IN_AFFINE_RELU if c["mode"] == "affine" else 0) | (L.CONV_IN_BATCH_SCALE if c["mode"] == "bscale" else 0) |
            (L.CONV_UPSAMPLE2X if c["up"] else 0) | (L.CONV_UP_FIR1331 if c["up"] == "fir" else 0) | (L.CONV_WINOGRAD if c["wino"] else 0))


def workspace_bytes(c, L):
    """What the caller is told to allocate (spk_conv2d_wgrad_workspace_bytes, its Winograd twin for the routing case)."""
    H, W = out_hw(c)
    if c["wino"]:
        return L.lib().spk_conv2d_wgrad_wino_workspace_bytes(c["splits"], c["B"], c["Cin"], c["G"] * c["Cout"], H, W)
    return L.lib().spk_conv2d_wgrad_workspace_bytes(c["k"], c["k"], c["stride"], c["splits"], c["B"], c["Cin"], c["G"] * c["Cout"], H, W)


def dummy_desc(c, L):
    """The case's ``spk_wgrad_desc`` with made-up pointers of the case's alignment (the query reads no memory)."""
    H, W = out_hw(c)
    nxt = iter(range(0x100000, 0x10000000, 0x1000))
    ptr = lambda on=True, off=False: (next(nxt) + (4 if off else 0)) if on else None
    return L.WgradDesc(g=ptr(True, "g" in c["misalign"]), x=ptr(True, "x" in c["misalign"]), in_scale=ptr(c["mode"] != "plain"),
                       in_shift=ptr(c["mode"] == "affine"), dw=ptr(True, "dw" in c["misalign"]), B=c["B"], Cin=c["Cin"], Cout=c["Cout"], H=H, W=W,
                       Hin=c["Hs"], Win=c["Ws"], kh=c["k"], kw=c["k"], stride=c["stride"], flags=flags_of(c, L), scale=c["scale"],
                       accumulate=int(c["accumulate"]), splits=c["splits"], workspace=ptr(), workspace_bytes=1 << 40, groups=c["G"],
                       group_in_stride=0 if (c["shared"] or c["G"] == 1) else c["Cin"], fold=c["fold"], g_scale=ptr(c["mode"] == "bscale"))


def query(c, L, desc=None):
    form = L.WgradForm()
    L.check(L.lib().spk_conv2d_wgrad_launch_form(desc if desc is not None else dummy_desc(c, L), form), "spk_conv2d_wgrad_launch_form")
    f = {n: getattr(form, n) for n, _ in L.WgradForm._fields_}
    f["kernel"], f["mode"], f["reducer"] = KERNELS[f["kernel"]], MODES[f["mode"]], REDUCERS[f["reducer"]]
    return f


def coverage_key(c, form):
    """(kernel[.kxk sS for the tap kernel], mode, reducer) of a case, from the form the library answered."""
    kern = form["kernel"] + (f".{c['k']}x{c['k']}s{c['stride']}" if form["kernel"] in ("tap", "gemm1x1") else "")
    mode = {"bilinear": "bilinear", "fir": "fir+bscale"}.get(c["up"], form["mode"])
    return (kern, mode, form["reducer"])


# ---- the table ---------------------------------------------------------------------------------------------------------------------
# Blocks: tap / pipe / wide 64co x 64ci (tap at stride 2: 64 x 32, 7x7: 64 x 4 packed); s2 128co x 32ci; GEMM (64 MT) x (64 NT).
A, S = "affine", "bscale"
CASES = [
    # -- tap kernel, 3x3 s1, runtime geometry: planes under 8 x 4 (the wide form needs W >= 8, the fixed / pipe forms a 16 x 4 tile)
    case("tap.s1.2x2", 3, 1, 5, 5, 3, 2, 2, kernel="tap", TW=2, TH=2, TB=8, reducer="dword"),                   # B % TB != 0
    case("tap.s1.5x3", 3, 1, 3, 68, 72, 5, 3, scale=0.5, accumulate=True, kernel="tap", TW=4, TH=8, TB=2, reducer="vec"),     # ragged vs 64
    case("tap.s1.affine.4x4", 3, 1, 5, 20, 24, 4, 4, A, kernel="tap", TW=4, TH=4, TB=2),
    # -- tap kernel, fixed 16 x 4 geometry (affine input the wide form declines)
    case("fixed.w13", 3, 1, 2, 20, 24, 9, 13, A, kernel="tap_fixed", TW=16, TH=4, TB=1),
    case("fixed.misg", 3, 1, 2, 70, 72, 8, 16, A, misalign=("g",), scale=0.5, accumulate=True, kernel="tap_fixed"),
    case("fixed.misx", 3, 1, 1, 8, 16, 8, 16, A, misalign=("x",), kernel="tap_fixed"),
    # -- the pipelined form (plain input the wide form declines)
    case("pipe.w13.split1", 3, 1, 3, 20, 40, 9, 13, splits=1, kernel="pipe", splits_=1, n_tiles=9, tiles_per_split=9),
    case("pipe.misg", 3, 1, 2, 8, 16, 8, 16, misalign=("g",), kernel="pipe"),
    case("pipe.misx.ragged", 3, 1, 2, 70, 72, 6, 20, misalign=("x",), scale=0.5, accumulate=True, kernel="pipe"),
    # -- the wide form, 16 x 4 tiles (W >= 16) and 8 x 8 tiles, each plain / affine / batch scale
    case("wide16.plain.partial", 3, 1, 2, 24, 40, 6, 20, kernel="wide16", TW=16, TH=4),
    case("wide16.affine.g2.fold", 3, 1, 2, 8, 64, 8, 16, A, G=2, fold=2, kernel="wide16", fold_=2),
    case("wide16.affine.shared", 3, 1, 1, 12, 64, 6, 24, A, G=2, shared=True, scale=0.5, accumulate=True, kernel="wide16"),
    case("wide16.bscale", 3, 1, 3, 20, 72, 6, 24, S, kernel="wide16"),
    case("wide8.plain.w8", 3, 1, 2, 8, 16, 8, 8, kernel="wide8", TW=8, TH=8),
    case("wide8.plain.w12", 3, 1, 3, 70, 72, 6, 12, splits=2, kernel="wide8"),
    case("wide8.affine.ragged", 3, 1, 2, 20, 72, 12, 12, A, kernel="wide8"),
    case("wide8.affine.g3", 3, 1, 2, 8, 64, 4, 8, A, G=3, kernel="wide8"),
    case("wide8.plain.g4.fold.shared", 3, 1, 1, 8, 64, 8, 8, G=4, shared=True, fold=2, kernel="wide8", fold_=2),
    case("wide8.bscale", 3, 1, 2, 12, 40, 4, 8, S, scale=0.5, accumulate=True, kernel="wide8"),
    case("wide8.plain.deep", 3, 1, 32, 8, 8, 8, 8, kernel="wide8", n_slabs=32, reducer="deep"),
    case("wide8.affine.g2.fold.deep", 3, 1, 32, 8, 64, 8, 8, A, G=2, fold=2, scale=0.5, accumulate=True, kernel="wide8", reducer="deep", fold_=2),
    case("wide16.plain.misdw", 3, 1, 1, 8, 16, 4, 16, misalign=("dw",), kernel="wide16", reducer="dword"),
    # -- the stride-2 form (Cout >= 96; grouped: Cout % 128 == 0), and what falls back to the tap kernel
    case("s2_16.plain.c96", 3, 2, 2, 8, 96, 8, 32, kernel="s2_16", TW=16, TH=4),
    case("s2_16.affine.c160", 3, 2, 2, 40, 160, 12, 40, A, scale=0.5, accumulate=True, kernel="s2_16"),
    case("s2_8.plain.c128", 3, 2, 2, 32, 128, 16, 16, kernel="s2_8", TW=8, TH=8),
    case("s2_8.affine.g2.fold", 3, 2, 1, 16, 128, 12, 16, A, G=2, fold=2, kernel="s2_8", fold_=2),
    case("s2_16.plain.g2", 3, 2, 1, 8, 128, 4, 32, G=2, kernel="s2_16"),
    case("taps2.cout80", 3, 2, 2, 8, 80, 16, 16, kernel="tap"),
    case("taps2.w4", 3, 2, 3, 40, 96, 8, 8, A, kernel="tap"),
    case("taps2.odd", 3, 2, 2, 8, 96, 9, 9, kernel="tap"),
    case("taps2.misx", 3, 2, 2, 8, 96, 16, 16, A, misalign=("x",), scale=0.5, accumulate=True, kernel="tap"),
    # -- the upsample-folded form: x is the low-resolution tensor
    case("up.bilinear.16x4", 3, 1, 2, 8, 16, 2, 8, up="bilinear", kernel="up", TW=16, TH=4),
    case("up.bilinear.w24", 3, 1, 2, 20, 72, 5, 12, up="bilinear", scale=0.5, accumulate=True, kernel="up"),
    case("up.fir.16x4", 3, 1, 2, 8, 16, 2, 8, S, up="fir", kernel="up"),
    case("up.fir.w24", 3, 1, 3, 12, 40, 4, 12, S, up="fir", kernel="up"),
    # -- the 1x1 GEMM, register-staged: ragged channels, stride 2, a misaligned tensor
    case("g1.s1.plain.m2n2", 1, 1, 2, 70, 130, 8, 8, kernel="gemm1x1", MT=2, NT=2),
    case("g1.s1.affine.m1n1", 1, 1, 1, 24, 40, 4, 8, A, kernel="gemm1x1", MT=1, NT=1, n_tiles=1),
    case("g1.s1.plain.m2n1.short", 1, 1, 3, 20, 72, 8, 12, splits=2, kernel="gemm1x1", MT=2, NT=1, n_tiles=9, tiles_per_split=5, splits_=2),
    case("g1.s1.affine.m1n2", 1, 1, 2, 70, 64, 8, 8, A, scale=0.5, accumulate=True, kernel="gemm1x1", MT=1, NT=2),
    case("g1.s1.mis", 1, 1, 2, 64, 64, 8, 8, misalign=("x",), kernel="gemm1x1", MT=1, NT=1),
    case("g1.s2.plain.m1n1", 1, 2, 2, 64, 64, 16, 16, kernel="gemm1x1", MT=1, NT=1),
    case("g1.s2.affine.m2n2", 1, 2, 2, 70, 130, 16, 16, A, kernel="gemm1x1", MT=2, NT=2),
    case("g1.s2.plain.m1n2.g2", 1, 2, 1, 72, 64, 8, 16, G=2, kernel="gemm1x1", MT=1, NT=2),
    case("g1.s2.affine.m2n1", 1, 2, 2, 20, 128, 8, 16, A, scale=0.5, accumulate=True, kernel="gemm1x1", MT=2, NT=1),
    case("g1.s1.slabs32.dword", 1, 1, 16, 6, 8, 16, 16, kernel="gemm1x1", n_slabs=32, reducer="dword"),
    case("g1.s1.deep", 1, 1, 16, 8, 8, 16, 16, kernel="gemm1x1", n_slabs=32, reducer="deep", taps=1),
    # -- its LDS-DMA twin: whole blocks, aligned, stride 1
    case("dma.m1n1.onetile", 1, 1, 1, 64, 64, 4, 8, kernel="gemm1x1_dma", MT=1, NT=1, n_tiles=1),
    case("dma.m1n2.affine", 1, 1, 3, 128, 64, 8, 12, A, kernel="gemm1x1_dma", MT=1, NT=2, n_tiles=9),       # 3 k-tiles per image
    case("dma.m2n1", 1, 1, 2, 64, 128, 8, 8, scale=0.5, accumulate=True, kernel="gemm1x1_dma", MT=2, NT=1),
    case("dma.m2n2.affine", 1, 1, 2, 128, 128, 4, 8, A, kernel="gemm1x1_dma", MT=2, NT=2),
    case("dma.g2.fold", 1, 1, 5, 64, 64, 8, 12, G=2, fold=2, splits=2, kernel="gemm1x1_dma", MT=1, NT=1, fold_=2),           # k-tiles cross images
    # -- the tap kernel on a 1x1: H W % 32 != 0
    case("tap1.s1.5x5", 1, 1, 3, 20, 24, 5, 5, kernel="tap"),
    case("tap1.s1.affine.5x5", 1, 1, 2, 70, 72, 5, 5, A, scale=0.5, accumulate=True, kernel="tap"),
    case("tap1.s1.1x1", 1, 1, 70, 40, 24, 1, 1, kernel="tap", TW=1, TH=1, TB=64),
    case("tap1.s2.odd.affine", 1, 2, 2, 40, 24, 9, 9, A, kernel="tap"),
    case("tap1.s2.plain", 1, 2, 3, 8, 72, 10, 10, kernel="tap"),
    # -- 4x4 stride 2 in row passes: the weight gradient of ConvTranspose2d(4, s2, p1) (g = the layer's input, x = its output gradient)
    case("k4.rowpass", 4, 2, 2, 20, 40, 12, 16, kernel="tap", taps=16),
    case("k4.rowpass.ragged", 4, 2, 3, 40, 72, 8, 8, scale=0.5, accumulate=True, kernel="tap", taps=16),
    # -- the stem form (7x7 s2, 3 -> 64 per group, plain, output W % 4 == 0, aligned g) and the packed tap form behind it
    case("stem.g1", 7, 2, 3, 3, 64, 20, 40, kernel="stem", taps=1),
    case("stem.g2.own", 7, 2, 2, 3, 64, 16, 24, G=2, scale=0.5, accumulate=True, kernel="stem"),
    case("stem.g2.shared.fold", 7, 2, 2, 3, 64, 18, 72, G=2, shared=True, fold=2, kernel="stem", fold_=2),
    case("stem.slabs.over", 7, 2, 1, 3, 64, 8, 16, splits=7, kernel="stem", n_tiles=1, n_slabs=1),
    case("k7.cout40", 7, 2, 2, 3, 40, 16, 24, kernel="tap", taps=49),
    case("k7.w11", 7, 2, 2, 3, 64, 18, 22, kernel="tap"),
    case("k7.cin4", 7, 2, 2, 4, 64, 16, 16, scale=0.5, accumulate=True, kernel="tap"),
    case("k7.misg", 7, 2, 2, 3, 64, 16, 24, misalign=("g",), kernel="tap"),
    case("k7.affine", 7, 2, 2, 3, 64, 16, 24, A, kernel="tap"),
    # -- the Winograd route: routing only (its arithmetic is held to fp64 in tests/test_wino_gpu.py)
    case("wino.route", 3, 1, 1, 64, 64, 4, 16, wino=True, kernel="wino", taps=9),
]
for _c in CASES:                 # (``splits`` / ``fold`` are also case fields: their declared twins carry a trailing underscore)
    _c["declares"] = {k.rstrip("_"): v for k, v in _c["declares"].items()}
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# launches spk_conv2d_wgrad must keep refusing: (case, a fragment of the error)
REFUSALS = [
    (case("no.bscale.w4", 3, 1, 2, 8, 16, 4, 4, S, kernel="-"), "IN_BATCH_SCALE does not take this shape"),
    (case("no.up.w12", 3, 1, 2, 8, 16, 4, 6, up="bilinear", kernel="-"), "UPSAMPLE2X does not take this shape"),
    (case("no.grouped.cout40", 3, 1, 2, 8, 40, 4, 6, G=2, kernel="-"), "grouped launches need Cout"),
    (case("no.k7.cin5", 7, 2, 2, 5, 64, 16, 16, kernel="-"), "packs"),
]
