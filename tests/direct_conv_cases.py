"""Case tables and fp64 reference of the direct f32 MFMA conv (csrc/conv_mfma_f32.hpp) and of the split-K finishers
(csrc/conv_api.hip) -- test infrastructure, CPU only; the role tests/bf16x3_emulation.py has for the bf16x3 conv.

A case names a launch (shape, forced tile config, requested ksplit, operands, which tensors sit 4 bytes off a 16-byte boundary)
and DECLARES the form it reaches; ``spk_conv2d_launch_form`` -- the launch path's own statements -- decides whether it does
(tests/test_direct_conv_forms_cpu.py without a GPU, tests/test_direct_conv_branches_gpu.py again with the real pointers).

``reference(case)`` evaluates the whole operator in fp64 and, the same chain, in fp32 on the CPU:
    input stage (bilinear x2 | affine + ReLU | batch scale) -> conv * out_scale * out_scale_dev * demod -> + bias + noise_w * noise
    + residual -> LeakyReLU * act_gain -> y_pre -> style (rows wider than 2 Cy) -> + y (accumulate) -> + the half-resolution
    tensor at the even pixels (accum_half) -> BatchNorm sums.
The bound is measured on the reference, never on the kernel: max(4 x rel-L2(fp32 chain, fp64 chain), sqrt(kh kw Cin) 2^-24),
the bf16x3 file's rule with this kernel's contraction length; a single element: |y - ref| <= MAX_FACTOR x bound x rms(ref)."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle.weights_recipe import recipe_input, recipe_tensor

TOL_OP = 2e-5                   # the aggregate rel-L2 the older conv tests use: no case's bound may exceed it
MAX_FACTOR = 8.0                # as tests/bf16x3_emulation.py
STATS_REL = 1e-6                # rel-L2 of the sums over channels (tests/test_encoder_gpu.py)
OUT_SCALE, SLOPE, ACT_GAIN, SCALE_DEV = 0.37, 0.2, 2.0 ** 0.5, 1.25
MODES = {"plain": 0, "x2": 1, "affine": 2, "bscale": 3, "x2_bscale": 4, "plain_stats": 5, "plain_residual": 6}
EPILOGUES = {0: "dword", 1: "staged", 2: "halved"}
FINISHERS = {0: "none", 1: "scalar", 2: "vec"}
FULL = ("bias", "noise", "lrelu", "style", "y_pre", "accum", "scale_dev")       # the full flag set of an ungrouped launch


def case(name, family, k, stride, B, Cin, Cout, Hs, Ws, config, ksplit=1, G=1, shared=False, opts=(), stats=None, misalign=(),
         hw=None, like=None, **declares):
    """``Hs x Ws``: the size of x.  ``opts``: bias noise lrelu style y_pre accum scale_dev x2 affine bscale demod residual, and for
    tests/gemm_conv_cases.py accum_half (y(2h, 2w) += t(h, w)), transposed (the operator is the 1x1 of w^T -- the data gradient; Cin /
    Cout are the OPERATOR's, the weight is [Cin, Cout, 1, 1]) and unit_scale (out_scale = 1).
    ``stats``: None, "own" (one copy of the sums per pixel tile) or "atomic" (one copy).  ``misalign``: of out / out_pre / noise /
    residual, the tensors that start 4 bytes off.  ``hw``: the destination size of a stride-2 data gradient (default 2 Hs - 1 x 2 Ws - 1).
    ``like``: the case whose operands this one shares.  ``declares``: fields of spk_conv2d_form the case says it reaches (``slices``: the resolved ksplit)."""
    return dict(name=name, family=family, k=k, stride=stride, B=B, Cin=Cin, Cout=Cout, Hs=Hs, Ws=Ws, config=config, ksplit=ksplit,
                G=G, shared=shared, opts=frozenset(opts), stats=stats, misalign=frozenset(misalign), hw=hw, like=like, declares=declares)


def out_hw(c):
    k, s, Hs, Ws = c["k"], c["stride"], c["Hs"], c["Ws"]
    if c["family"] == "transpose4x4" or "x2" in c["opts"]:
        return 2 * Hs, 2 * Ws
    if c["family"] in ("dgrad_s2", "dgrad13"):
        return c["hw"] or (2 * Hs - 1, 2 * Ws - 1)
    p = (k - 1) // 2
    return (Hs + 2 * p - k) // s + 1, (Ws + 2 * p - k) // s + 1


def mode_of(c):
    o = c["opts"]
    if "residual" in o:
        return "plain_residual"
    if "affine" in o:
        return "affine"
    if "x2" in o:
        return "x2_bscale" if "bscale" in o else "x2"
    if "bscale" in o:
        return "bscale"
    return "plain_stats" if (c["stats"] and c["k"] == 3 and c["stride"] == 1) else "plain"


# ---- operands ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = BY_NAME[name]
    B, Cin, Cout, Hs, Ws, G, k, o = c["B"], c["Cin"], c["Cout"], c["Hs"], c["Ws"], c["G"], c["k"], c["opts"]
    H, W = out_hw(c)
    Cx, Cy = (Cin if c["shared"] else G * Cin), G * Cout
    tag = f"dcc.{c['like'] or name}"
    t = dict(x=recipe_input(f"{tag}.x", (B, Cx, Hs, Ws)))
    if c["family"] == "transpose4x4":          # the module's [Cin, Cout, 4, 4] parameter
        t["w"] = [recipe_tensor(f"{tag}.w", (Cin, Cout, 4, 4), (4 * Cin) ** -0.5)]
    elif c["family"] in ("dgrad_s2", "dgrad13"):   # the FORWARD conv's weight [channels of g = Cin][channels of dx = Cout][3][3]
        t["w"] = [recipe_tensor(f"{tag}.w{g}", (Cin, Cout, 3, 3), (2.25 * Cin) ** -0.5) for g in range(G)]
    elif "transposed" in o:                    # the forward 1x1's weight: [its Cout = the contraction][its Cin = the output rows]
        t["w"] = [recipe_tensor(f"{tag}.w{g}", (Cin, Cout, 1, 1), Cin ** -0.5) for g in range(G)]
    else:
        t["w"] = [recipe_tensor(f"{tag}.w{g}", (Cout, Cin, k, k), (k * k * Cin) ** -0.5) for g in range(G)]
    if "bias" in o:
        t["bias"] = recipe_tensor(f"{tag}.b", (Cy,), 0.3)
    if "noise" in o:
        t["noise_w"] = recipe_tensor(f"{tag}.nw", (Cy,), 0.2)
        t["noise"] = recipe_input(f"{tag}.nz", (B, 1, H, W))
    if "style" in o:                           # rows [s0 (Cy) | s1 (Cy) | 3 unused floats]: style_stride > 2 Cy
        t["style"] = recipe_input(f"{tag}.st", (B, 2 * Cy + 3)) * 0.3
    if "accum" in o:
        t["y0"] = recipe_input(f"{tag}.y0", (B, Cy, H, W)) * 0.5
    if "residual" in o:
        t["residual"] = recipe_input(f"{tag}.res", (B, Cy, H, W)) * 0.5
    if "accum_half" in o:
        t["half"] = recipe_input(f"{tag}.half", (B, Cy, (H + 1) // 2, (W + 1) // 2)) * 0.5
    if "affine" in o:
        t["in_scale"] = 1.0 + 0.2 * recipe_input(f"{tag}.ia", (Cx,))
        t["in_shift"] = 0.1 * recipe_input(f"{tag}.ib", (Cx,))
    if "bscale" in o:
        t["bscale"] = 1.0 + 0.3 * recipe_input(f"{tag}.s", (B, Cin), "uniform")
    if "demod" in o:
        t["demod"] = 0.5 + recipe_input(f"{tag}.d", (B, Cout), "uniform").abs()
    return t


def inputs(c):
    return _inputs(c["name"])


def scalars(c):
    """(out_scale, out_scale_dev | None, slope | None, act_gain) as the launch passes them."""
    o = c["opts"]
    plain = c["family"] in ("dgrad_s2", "dgrad13", "transpose4x4", "stem")
    return (1.0 if (c["family"] in ("transpose4x4", "stem") or "unit_scale" in o) else OUT_SCALE, SCALE_DEV if "scale_dev" in o else None, SLOPE if "lrelu" in o else None,
            ACT_GAIN if ("lrelu" in o and not plain) else 1.0)


# ---- the operator chain ----------------------------------------------------------------------------------------------------------
def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def chain(c, dtype, *, t=None, drop_ci=None, shift_tap_row=None, swap=None, double_ci=None, residual_late=False, edge_pad=None):
    """(y_pre, y) of the whole operator in ``dtype``.  The keyword arguments seed faults for the sensitivity checks:
    ``drop_ci``: input channels (per group) left out of the contraction; ``shift_tap_row``: output row computed with the tap one
    row below; ``swap`` = (operand, c0, c1): two channels of bias / style / demod exchanged; ``double_ci``: input channels counted
    twice; ``residual_late``: the residual added after the activation; ``edge_pad`` = "row" / "col": the padding below / right of the
    image repeats the last row / column instead of being zero."""
    t = dict(inputs(c) if t is None else t)
    o, G, Cin, Cout, k, s = c["opts"], c["G"], c["Cin"], c["Cout"], c["k"], c["stride"]
    H, W = out_hw(c)
    Cy = G * Cout
    if swap is not None:
        name, c0, c1 = swap
        v = t[name].clone()
        if name == "style":
            for base in (0, Cy):
                v[:, [base + c0, base + c1]] = v[:, [base + c1, base + c0]]
        elif name == "demod":
            v[:, [c0, c1]] = v[:, [c1, c0]]
        else:
            v[[c0, c1]] = v[[c1, c0]]
        t[name] = v
    x = t["x"].to(dtype)
    if "affine" in o:
        x = torch.relu(x * t["in_scale"].to(dtype).view(1, -1, 1, 1) + t["in_shift"].to(dtype).view(1, -1, 1, 1))
    if "bscale" in o:
        x = x * t["bscale"].to(dtype).view(x.shape[0], -1, 1, 1)
    if "x2" in o:
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    outs = []
    for g in range(G):
        xg = x if c["shared"] else x[:, g * Cin:(g + 1) * Cin]
        w = t["w"][g].to(dtype)
        if "transposed" in o:
            w = w.transpose(0, 1)
        if drop_ci is not None or double_ci is not None:
            keep = torch.ones(Cin, dtype=dtype)
            keep[list(drop_ci or ())] = 0
            keep[list(double_ci or ())] = 2
            xg = xg * keep.view(1, -1, 1, 1)
        if c["family"] == "transpose4x4":
            outs.append(F.conv_transpose2d(xg, w, stride=2, padding=1))
        elif c["family"] in ("dgrad_s2", "dgrad13"):
            op = (H - (2 * c["Hs"] - 1), W - (2 * c["Ws"] - 1))
            outs.append(F.conv_transpose2d(xg, w, stride=2, padding=1, output_padding=op))
        elif edge_pad is not None:
            p = (k - 1) // 2
            xp = F.pad(xg, (p, 0, p, 0))
            xp = F.pad(xp, (0, 0, 0, p), mode="replicate" if edge_pad == "row" else "constant")
            xp = F.pad(xp, (0, p, 0, 0), mode="replicate" if edge_pad == "col" else "constant")
            outs.append(F.conv2d(xp, w, stride=s))
        else:
            yg = F.conv2d(xg, w, stride=s, padding=(k - 1) // 2)
            if shift_tap_row is not None:      # that row with every tap taken one input row lower
                lower = F.conv2d(F.pad(xg, (0, 0, 0, s))[:, :, s:], w, stride=s, padding=(k - 1) // 2)
                yg = yg.clone()
                yg[:, :, shift_tap_row] = lower[:, :, shift_tap_row]
            outs.append(yg)
    v = torch.cat(outs, 1)
    assert tuple(v.shape[-2:]) == (H, W), (v.shape, H, W)
    out_scale, scale_dev, slope, gain = scalars(c)
    sc = _f32(out_scale) * (_f32(scale_dev) if scale_dev is not None else 1.0)
    v = v * (sc if dtype == torch.float64 else _f32(sc))
    B = v.shape[0]
    if "demod" in o:
        v = v * t["demod"].to(dtype).view(B, Cy, 1, 1)
    if "bias" in o:
        v = v + t["bias"].to(dtype).view(1, Cy, 1, 1)
    if "noise" in o:
        v = v + t["noise_w"].to(dtype).view(1, Cy, 1, 1) * t["noise"].to(dtype)
    if "residual" in o and not residual_late:
        v = v + t["residual"].to(dtype)
    if slope is not None:
        v = torch.where(v > 0, v, v * _f32(slope)) * _f32(gain)
    if "residual" in o and residual_late:
        v = v + t["residual"].to(dtype)
    pre = v
    if "style" in o:
        st = t["style"].to(dtype)
        v = v * (st[:, :Cy, None, None] + 1.0) + st[:, Cy:2 * Cy, None, None]
    if "accum" in o:
        v = v + t["y0"].to(dtype)
    if "accum_half" in o:                      # after the activation and the accumulate, before the sums (csrc/conv1x1_gemm2.hip)
        v = v.clone()
        v[:, :, ::2, ::2] += t["half"].to(dtype)
    return pre, v


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def sums(y):
    """Per-channel fp64 (sum, sum of squares) over (b, h, w)."""
    y = y.double()
    return y.sum((0, 2, 3)), y.pow(2).sum((0, 2, 3))


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = BY_NAME[name]
    pre, y = chain(c, torch.float64)
    pre32, y32 = chain(c, torch.float32)
    bound = max(4 * rel_l2(y32, y), math.sqrt(c["k"] * c["k"] * c["Cin"]) * 2.0 ** -24)
    ref = dict(y=y, y32=y32, pre=pre, bound=bound)
    if c["stats"]:
        ref["sum"], ref["sumsq"] = sums(y)
    return ref


def reference(c):
    """fp64 result ``y`` (and ``pre``, ``sum`` / ``sumsq``), the fp32 chain ``y32`` and the case's ``bound``.  Shared: do not write."""
    return _reference(c["name"])


# ---- the checks, shared by the GPU test (a kernel's output) and the CPU sensitivity test (a mutated reference) ---------------------
def figures(c, y, pre=None, stats=None):
    """-> {what: (figure, limit)}: every figure must stay at or below its limit."""
    ref = reference(c)
    bound = ref["bound"]
    out = {}

    def tensor(what, got, want):
        got = got.detach().cpu().double()
        assert got.shape == want.shape, (got.shape, want.shape)
        out[f"{what} rel-L2"] = (rel_l2(got, want), bound)
        out[f"{what} max|diff|"] = (float((got - want).abs().max()), MAX_FACTOR * bound * rms(want))

    tensor("y", y, ref["y"])
    if pre is not None:
        tensor("y_pre", pre, ref["pre"])
    if stats is not None:
        s, q = (v.detach().cpu().double() for v in stats)
        n = ref["y"].numel() // ref["y"].shape[1]                       # B * H * W
        lim = MAX_FACTOR * bound * rms(ref["y"]) * n
        out["sums rel-L2"] = (max(rel_l2(s, ref["sum"]), rel_l2(q, ref["sumsq"])), STATS_REL)
        out["sum max|diff|"] = (float((s - ref["sum"]).abs().max()), lim)
        out["sumsq max|diff|"] = (float((q - ref["sumsq"]).abs().max()), lim * 2 * float(ref["y"].abs().max()))
    return out


# ---- the descriptor, for the query without a device --------------------------------------------------------------------------------
def flags_of(c, L):
    o = c["opts"]
    f = {"dgrad_s2": L.CONV_DGRAD_S2, "dgrad13": L.CONV_DGRAD_S2, "transpose4x4": L.CONV_TRANSPOSE4X4_S2, "wino": L.CONV_WINOGRAD}.get(c["family"], 0)
    for name, bit in (("bias", L.EPI_BIAS), ("noise", L.EPI_NOISE), ("lrelu", L.EPI_LRELU), ("style", L.EPI_STYLE), ("x2", L.CONV_UPSAMPLE2X),
                      ("accum", L.EPI_ACCUM), ("affine", L.CONV_IN_AFFINE_RELU), ("bscale", L.CONV_IN_BATCH_SCALE), ("residual", L.EPI_RESIDUAL)):
        if name in o:
            f |= bit
    return f | (L.EPI_STATS if c["stats"] else 0)


def dummy_desc(c, L):
    """The case's ``spk_conv2d_desc`` with made-up pointers of the case's alignment (``spk_conv2d_launch_form`` reads no memory)."""
    o = c["opts"]
    H, W = out_hw(c)
    nxt = iter(range(0x100000, 0x10000000, 0x1000))
    ptr = lambda on=True, off=False: (next(nxt) + (4 if off else 0)) if on else None
    k, stride = {"dgrad_s2": (3, 2), "dgrad13": (3, 2), "transpose4x4": (4, 2)}.get(c["family"], (c["k"], c["stride"]))
    return L.Conv2dDesc(
        x=ptr(), w_packed=ptr(), bias=ptr("bias" in o), noise_w=ptr("noise" in o), noise=ptr("noise" in o, "noise" in c["misalign"]),
        style=ptr("style" in o), in_scale=ptr("affine" in o or "bscale" in o), in_shift=ptr("affine" in o), stats=ptr(bool(c["stats"])),
        y=ptr(True, "out" in c["misalign"]), y_pre=ptr("y_pre" in o, "out_pre" in c["misalign"]),
        B=c["B"], Cin=c["Cin"], Cout=c["Cout"], H=H, W=W, Hin=c["Hs"], Win=c["Ws"], kh=k, kw=k, stride=stride,
        style_stride=2 * c["G"] * c["Cout"] + 3 if "style" in o else 0, flags=flags_of(c, L), lrelu_slope=SLOPE, out_scale=OUT_SCALE,
        config=c["config"], ksplit=c["ksplit"], workspace=ptr(), workspace_bytes=1 << 40, out_scale_bc=ptr("demod" in o), act_gain=ACT_GAIN,
        groups=c["G"], group_in_stride=0 if (c["shared"] or c["G"] == 1) else c["Cin"],
        stats_slots=0 if c["stats"] != "own" else 65536, out_scale_dev=ptr("scale_dev" in o),
        residual=ptr("residual" in o, "residual" in c["misalign"]))


def query(c, L, desc=None):
    form = L.Conv2dForm()
    L.check(L.lib().spk_conv2d_launch_form(desc if desc is not None else dummy_desc(c, L), form), "spk_conv2d_launch_form")
    return {n: getattr(form, n) for n, _ in L.Conv2dForm._fields_}


def coverage_key(c, form):
    """(family, mode, geometry, epilogue, finisher) of a case, from the form the library answered."""
    if c["family"] in ("wino", "dgrad13"):
        return (c["family"], "-", "-", "-", FINISHERS[form["finisher"]])
    epi = "raw" if form["ksplit"] > 1 else EPILOGUES[form["staged"]]          # (a sliced launch stores raw partial sums)
    family = c["family"] + ("" if c["family"] != "3x3s1" else ("a" if form["config"] <= 3 else "b"))      # configs 0-3 / 4-7
    return (family, mode_of(c), "fg" if form["fixed_geometry"] else "generic", epi, FINISHERS[form["finisher"]])


# ---- the tables --------------------------------------------------------------------------------------------------------------------
# Tile configs: 0-3 (CI_T 8) and 4-7 (CI_T 4) are [128co x 128px, 64 x 256, 64 x 64, 32 x 128]; 8-11 the same tiles with CI_T 16.
# The fixed-geometry build (FG) exists for configs 4-7 on 3x3 kernels: TW 32, a full tile height, TB 1, no ragged chunk.
ST = ("bias", "lrelu")
CASES = [
    # -- 3x3 stride 1, configs 0-3: plain / x2 / affine; TW 2..32; TB > 1 with a ragged image group; partial tiles; Cin < CI_T
    case("s1a.plain.tw2", "3x3s1", 3, 1, 9, 5, 20, 2, 2, 2, opts=FULL, TW=2, TB=8, staged=0, fixed_geometry=0, ragged_last_chunk=1, n_chunks=1),
    case("s1a.plain.tw4", "3x3s1", 3, 1, 3, 16, 64, 4, 4, 2, opts=FULL, TW=4, TB=4, staged=1),
    case("s1a.plain.tw4.mispre", "3x3s1", 3, 1, 3, 16, 64, 4, 4, 2, opts=FULL, misalign=("out_pre",), TW=4, staged=0),
    case("s1a.plain.tw8", "3x3s1", 3, 1, 3, 12, 40, 6, 8, 0, opts=ST, TW=8, TH=8, TB=2, staged=1, ragged_last_chunk=1),
    case("s1a.plain.tw16", "3x3s1", 3, 1, 1, 8, 33, 10, 12, 3, opts=ST, TW=16, TH=8, TB=1, staged=1),
    case("s1a.plain.w18", "3x3s1", 3, 1, 2, 8, 24, 9, 18, 2, opts=FULL, TW=32, staged=0),                       # W % 4 != 0
    case("s1a.x2.1x1", "3x3s1", 3, 1, 3, 9, 16, 1, 1, 3, opts=("x2",) + FULL, TW=2, staged=0, mode=1),         # Hin = Win = 1
    case("s1a.x2", "3x3s1", 3, 1, 2, 16, 70, 5, 20, 1, opts=("x2",) + FULL, TW=32, TH=8, staged=1, mode=1),
    case("s1a.x2.hin1", "3x3s1", 3, 1, 1, 8, 32, 1, 6, 0, opts=("x2", "bias"), TW=16, staged=1, mode=1),
    case("s1a.affine", "3x3s1", 3, 1, 2, 20, 64, 12, 40, 0, opts=("affine",) + ST, stats="own", TW=32, TH=4, staged=1, mode=2),
    case("s1a.affine.misout", "3x3s1", 3, 1, 2, 20, 64, 12, 40, 0, opts=("affine",) + ST, stats="atomic", misalign=("out",), like="s1a.affine", staged=0, mode=2),
    case("s1a.stats.c1", "3x3s1", 3, 1, 2, 16, 64, 8, 32, 1, opts=ST, stats="own", mode=5, staged=1, TW=32, TH=8),
    case("s1a.stats.c3.dword", "3x3s1", 3, 1, 3, 8, 24, 7, 9, 3, opts=ST, stats="atomic", mode=5, staged=0),
    case("s1a.g2", "3x3s1", 3, 1, 2, 12, 40, 8, 8, 2, G=2, opts=ST + ("accum",), stats="own", mode=5, staged=1),
    case("s1a.g2.shared", "3x3s1", 3, 1, 2, 12, 40, 8, 8, 2, G=2, shared=True, opts=("affine",) + ST, stats="atomic", mode=2, staged=1),
    # -- 3x3 stride 1, configs 4-7: each input stage in the FG and in the generic build
    case("s1b.plain.fg", "3x3s1", 3, 1, 1, 8, 40, 4, 32, 4, opts=FULL, fixed_geometry=1, staged=1, TW=32, TH=4),
    case("s1b.plain.fg.partial", "3x3s1", 3, 1, 2, 8, 24, 10, 40, 5, opts=FULL, fixed_geometry=1, staged=2, TW=32, TH=8),
    case("s1b.plain.fg.partial.dword", "3x3s1", 3, 1, 2, 8, 24, 10, 40, 5, opts=FULL, misalign=("out",), like="s1b.plain.fg.partial", fixed_geometry=1, staged=0),
    case("s1b.plain.ragged", "3x3s1", 3, 1, 1, 18, 64, 10, 40, 6, opts=ST, fixed_geometry=0, ragged_last_chunk=1, TW=32, staged=1),
    case("s1b.x2.fg", "3x3s1", 3, 1, 1, 8, 64, 5, 20, 7, opts=("x2",) + FULL, fixed_geometry=1, mode=1, staged=1),
    case("s1b.x2.generic", "3x3s1", 3, 1, 2, 6, 30, 3, 6, 6, opts=("x2",) + FULL, fixed_geometry=0, mode=1, staged=1, TW=16),
    case("s1b.bscale.fg", "3x3s1", 3, 1, 2, 8, 40, 10, 40, 4, opts=("bscale", "demod") + FULL, fixed_geometry=1, mode=3, staged=1),
    case("s1b.bscale.generic", "3x3s1", 3, 1, 3, 10, 24, 6, 6, 5, opts=("bscale", "demod") + FULL, fixed_geometry=0, mode=3, staged=0),
    case("s1b.x2bscale.fg", "3x3s1", 3, 1, 2, 4, 64, 8, 16, 5, opts=("x2", "bscale", "demod") + FULL, fixed_geometry=1, mode=4, staged=2),
    case("s1b.x2bscale.generic", "3x3s1", 3, 1, 2, 7, 33, 4, 4, 7, opts=("x2", "bscale", "demod") + FULL, fixed_geometry=0, mode=4, staged=1),
    case("s1b.affine.fg", "3x3s1", 3, 1, 1, 12, 64, 8, 64, 6, opts=("affine",) + ST, stats="own", fixed_geometry=1, mode=2, staged=1),
    case("s1b.affine.generic", "3x3s1", 3, 1, 1, 12, 64, 8, 12, 6, opts=("affine",) + ST, stats="own", fixed_geometry=0, mode=2, staged=1),
    case("s1b.stats.halved.c40", "3x3s1", 3, 1, 1, 8, 40, 16, 32, 5, opts=ST, stats="own", mode=5, staged=2),   # upper 32-row tile partly empty
    case("s1b.stats.halved.c24", "3x3s1", 3, 1, 2, 8, 24, 16, 32, 5, opts=ST, stats="atomic", mode=5, staged=2),  # ... wholly empty
    case("s1b.stats.c4", "3x3s1", 3, 1, 1, 8, 72, 8, 32, 4, opts=ST, stats="own", mode=5, fixed_geometry=0, staged=1),      # (the stats build has no FG form)
    case("s1b.stats.c7.generic", "3x3s1", 3, 1, 2, 6, 32, 6, 10, 7, opts=ST, stats="atomic", mode=5, fixed_geometry=0, staged=0),
    # -- 3x3 stride 2, configs 4-7
    case("s2.plain.fg", "3x3s2", 3, 2, 1, 8, 64, 8, 64, 6, opts=ST, fixed_geometry=1, staged=1, TW=32),
    case("s2.plain.generic", "3x3s2", 3, 2, 3, 6, 40, 9, 13, 4, opts=ST, stats="own", fixed_geometry=0, staged=0),
    case("s2.affine.fg", "3x3s2", 3, 2, 1, 8, 32, 16, 80, 7, opts=("affine",) + ST, stats="atomic", fixed_geometry=1, mode=2),
    case("s2.affine.generic", "3x3s2", 3, 2, 2, 10, 24, 8, 16, 5, opts=("affine",) + ST, fixed_geometry=0, mode=2, staged=1, TW=8),
    # -- 7x7 stride 2 on the tap kernel (the stem kernel takes Cin 3 -> Cout 64 only): the one-slot ring and the ring
    case("k7.cin3", "7x7s2", 7, 2, 2, 3, 24, 18, 22, 6, opts=ST, one_slot_ring=1, n_chunks=1),
    case("k7.cin6", "7x7s2", 7, 2, 1, 6, 40, 16, 16, 7, opts=ST, one_slot_ring=0, n_chunks=2, staged=1),
    case("k4", "4x4s2", 4, 2, 2, 6, 33, 12, 16, 5, opts=ST, n_chunks=2, staged=1),
    # one chunk on the one-slot ring: 29 KB of LDS are 5 workgroups a CU, the half tile of the staged epilogue (33 KB) would make it 4
    case("k4.lds.dword", "4x4s2", 4, 2, 2, 4, 40, 8, 16, 5, opts=FULL, one_slot_ring=1, TW=8, staged=0),
    # -- 1x1, configs 8-11
    case("p1.s1.plain", "1x1", 1, 1, 3, 20, 40, 6, 8, 8, opts=FULL, staged=2, ragged_last_chunk=1),
    case("p1.s1.plain.dword", "1x1", 1, 1, 3, 20, 40, 6, 8, 8, opts=FULL, misalign=("noise",), staged=0),
    case("p1.s1.stats", "1x1", 1, 1, 2, 16, 24, 8, 16, 9, opts=ST, stats="own", staged=1),
    case("p1.s1.affine", "1x1", 1, 1, 2, 12, 33, 5, 7, 10, opts=("affine",) + ST, stats="atomic", mode=2, staged=0),
    case("p1.s2.plain", "1x1", 1, 2, 2, 16, 32, 9, 15, 11, opts=ST, staged=1),
    case("p1.s2.affine", "1x1", 1, 2, 1, 24, 64, 16, 16, 10, opts=("affine",) + ST, stats="own", mode=2, staged=1),
    case("p1.res", "1x1", 1, 1, 2, 16, 40, 8, 8, 8, opts=("residual", "accum") + ST, mode=6, staged=2),
    case("p1.res.mis", "1x1", 1, 1, 2, 16, 40, 8, 8, 10, opts=("residual",) + ST, misalign=("residual",), mode=6, staged=0),
    case("p1.res.g2", "1x1", 1, 1, 2, 16, 24, 4, 8, 10, G=2, opts=("residual",) + ST, mode=6, staged=1),
    # -- 2x2 parity kernels, configs 0-3: odd destinations clip Y / X; always the dword epilogue
    case("dg.c0", "dgrad_s2", 2, 1, 2, 12, 10, 5, 6, 0, opts=("accum",), staged=0, hw=(9, 11)),
    case("dg.c3", "dgrad_s2", 2, 1, 1, 8, 6, 4, 4, 3, staged=0, hw=(7, 8)),
    case("dg.c2.g2", "dgrad_s2", 2, 1, 2, 8, 12, 3, 5, 2, G=2, staged=0, hw=(5, 9)),
    case("tp.c1", "transpose4x4", 2, 1, 2, 10, 12, 5, 7, 1, opts=("bias",), staged=0),
    case("tp.c2", "transpose4x4", 2, 1, 1, 8, 20, 3, 3, 2, opts=("bias", "accum"), staged=0),
    # -- split-K: slicing, and every way into each finisher
    case("sk.even.vec64", "3x3s1", 3, 1, 1, 32, 40, 16, 16, 2, ksplit=2, opts=FULL, stats="atomic", finisher=2, finisher_seg=64,
         chunks_per_split=2, last_split_chunks=2),
    case("sk.ragged.vec16", "3x3s1", 3, 1, 2, 20, 24, 8, 8, 6, ksplit=3, opts=ST, stats="atomic", finisher=2, finisher_seg=16, n_chunks=5,
         chunks_per_split=2, last_split_chunks=1, slices=3),
    case("sk.over.vec4", "3x3s1", 3, 1, 3, 16, 33, 4, 4, 2, ksplit=8, opts=ST, stats="atomic", finisher=2, finisher_seg=4, n_chunks=2, slices=2),
    case("sk.vec1", "3x3s1", 3, 1, 5, 16, 20, 2, 2, 3, ksplit=2, opts=ST, stats="atomic", finisher=2, finisher_seg=1),
    case("sk.scalar.hw", "3x3s1", 3, 1, 2, 16, 24, 5, 7, 2, ksplit=2, opts=FULL, stats="atomic", finisher=1),            # H*W % 4 != 0
    case("sk.scalar.q36", "3x3s1", 3, 1, 1, 16, 24, 12, 12, 6, ksplit=2, opts=ST, stats="atomic", finisher=1),             # H*W/4 = 36
    case("sk.scalar.q100", "3x3s1", 3, 1, 1, 8, 16, 20, 20, 7, ksplit=2, opts=ST, stats="atomic", finisher=1),             # H*W/4 = 100
    case("sk.scalar.mis", "3x3s1", 3, 1, 2, 16, 24, 8, 8, 2, ksplit=2, opts=FULL, stats="atomic", misalign=("out_pre",), finisher=1),
    case("sk.res.vec", "1x1", 1, 1, 2, 64, 40, 8, 8, 10, ksplit=2, opts=("residual", "accum") + ST, mode=6, finisher=2, finisher_seg=16),
    case("sk.res.scalar", "1x1", 1, 1, 2, 64, 40, 8, 8, 10, ksplit=4, opts=("residual",) + ST, misalign=("residual",), mode=6, finisher=1),
    case("sk.g2.vec", "3x3s1", 3, 1, 2, 16, 20, 8, 8, 2, ksplit=2, G=2, opts=ST, stats="atomic", finisher=2, finisher_seg=16),
    case("sk.g2.scalar", "1x1", 1, 1, 1, 32, 24, 5, 5, 10, ksplit=2, G=2, opts=ST, stats="atomic", finisher=1),
    case("sk.rounds.vec", "1x1", 1, 1, 36, 32, 64, 32, 32, 8, ksplit=2, opts=ST, stats="atomic", finisher=2, finisher_seg=64),   # > 2048 x 256 float4s
    case("sk.rounds.scalar", "1x1", 1, 1, 9, 32, 64, 31, 31, 8, ksplit=2, opts=ST, stats="atomic", finisher=1),                  # > 2048 x 256 floats
    case("sk.s2", "3x3s2", 3, 2, 2, 16, 24, 16, 16, 6, ksplit=2, opts=ST, stats="atomic", finisher=2, finisher_seg=16),
    # -- the other kernels that end in the shared finisher
    case("wino.sliced", "wino", 3, 1, 1, 64, 40, 16, 16, -1, ksplit=2, opts=("bias", "noise", "lrelu", "style", "y_pre", "accum"), finisher=2, finisher_seg=64),
    case("dg13.sliced.vec", "dgrad13", 3, 1, 1, 256, 12, 8, 16, 13, ksplit=0, finisher=2, hw=(16, 32)),
    case("dg13.sliced.scalar", "dgrad13", 3, 1, 1, 256, 12, 8, 16, 13, ksplit=0, opts=("accum",), misalign=("out",), finisher=1, hw=(16, 32)),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# one shape per staged form, run staged and forced to the dword epilogue by a misaligned out: (staged case, its dword twin)
STAGED_VS_DWORD = [("s1a.affine", "s1a.affine.misout"), ("s1b.plain.fg.partial", "s1b.plain.fg.partial.dword")]
