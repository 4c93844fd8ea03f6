"""Case tables of the small forward kernels -- the FC forward and its grouped form (csrc/fc.hip), upfirdn2d (csrc/stylegan2_ops.hip),
the modulated toRGB 1x1 with and without a skip and the fromRGB expand (csrc/pointwise.hip) -- test infrastructure, CPU only.

A case is a dict: a ``name``, the shapes and flags, and ``labels``: the branches it is NAMED FOR.  ``query(c, L)`` asks the library
which form the launch would take (``spk_fc_fwd_form`` / ``spk_upfirdn2d_form`` / ``spk_conv1x1_small_form``: the functions the
launchers themselves dispatch by, nothing launched, made-up pointers of the case's alignment) and names the branches that form and
the case's operands reach.  tests/test_small_fwd_forms_cpu.py holds every case to its labels without a GPU;
tests/test_small_fwd_kernels_gpu.py runs every case against the float64 references built here."""
import functools
import math

import torch

from oracle import modconv_ref as M
from oracle.weights_recipe import recipe_input, recipe_tensor

SLOPES = (0.2, 1.0)
BMUL = 0.5


def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


# ---- FC forward ------------------------------------------------------------------------------------------------------------------
def fc(name, B, I, O, *labels, x_stride=None, x_col=0, x_off=0, w_off=0, out=None, bias=True):
    """x is columns [x_col, x_col + I) of a [B, x_stride] buffer that starts ``x_off`` floats past a 16-byte boundary (``w_off``: the weight); ``out``:
    None (a fresh [B, O]) or (rows, row stride, first row, first column) of a larger sentinel-filled buffer."""
    return dict(kind="fc", name=name, B=B, I=I, O=O, labels=set(labels), x_stride=x_stride or I, x_col=x_col, x_off=x_off, w_off=w_off, out=out, bias=bias)


FC_CASES = [
    fc("scalar.i7", 3, 7, 5, "fc.scalar.I%4", "fc.scalar.O%4=1"),
    fc("scalar.xoff", 2, 64, 6, "fc.scalar.x misaligned", "fc.scalar.O%4=2", x_off=1),
    fc("scalar.woff", 3, 64, 4, "fc.scalar.w misaligned", w_off=1),
    fc("scalar.stride73", 9, 68, 4, "fc.scalar.x_stride%4", x_stride=73, x_col=4),
    fc("scalar.o7", 2, 6, 7, "fc.scalar.O%4=3"),
    fc("vec.i36", 1, 36, 3, "fc.vec.one ragged trip", "fc.vec.O%4=3"),
    fc("vec.i260", 11, 260, 9, "fc.vec.two trips, ragged last", "fc.vec.O%4=1"),
    fc("vec.i1024", 8, 1024, 4, "fc.vec.four full trips"),
    fc("vec.o6", 2, 36, 6, "fc.vec.O%4=2"),
    fc("vec512.b1", 1, 512, 6, "fc.vec512.B1", "fc.vec512.O%4=2"),         # the min(b0 + b, B - 1) clamp on seven of eight slots
    fc("vec512.b8", 8, 512, 6, "fc.vec512.B8"),
    fc("vec512.b11", 11, 512, 6, "fc.vec512.B11"),                         # a ragged second pass
    fc("vec512.b16", 16, 512, 6, "fc.vec512.B16"),
    fc("vec512.o5", 3, 512, 5, "fc.vec512.O%4=1"),
    fc("vec512.o7", 3, 512, 7, "fc.vec512.O%4=3"),
    # wlat[:, 3] of a [B, 14, 512] latent buffer, written into a column block of a wider output
    fc("vec512.wlat", 5, 512, 10, "fc.vec512.strided x", "fc.out_stride>O", x_stride=14 * 512, x_col=3 * 512, out=(7, 23, 1, 8)),
    fc("wide.i2052", 3, 2052, 3, "fc.wide.one trip, I%1024"),
    fc("wide.i8192", 9, 8192, 2, "fc.wide.two trips"),
    fc("wide.i6148", 9, 6148, 1, "fc.wide.two trips, ragged"),
    fc("wide.i2048.o6", 2, 2048, 6, "fc.wide.wide4-eligible I, O%4"),
    fc("wide.nobias", 3, 2052, 3, "fc.wide.no bias", bias=False),
    fc("wide4.nobias", 3, 3072, 4, "fc.wide4.no bias", bias=False),
    fc("wide4.out", 11, 2048, 4, "fc.out_stride>O", out=(13, 9, 2, 3)),
] + [fc(f"wide4.u{U}.b{B}", B, 1024 * U, 4 if U % 2 else 8, f"fc.wide4.U{U}.B{B}") for U in (2, 3, 4, 5, 6) for B in (3, 8, 11)]

# one grouped launch: (I, O) per group; group 3 has no bias; every x is a strided view
FC_GROUPS = [(36, 5), (260, 9), (512, 130), (1024, 4), (512, 6)]
FC_GROUP_BATCHES = (3, 11)
FC_GROUP_NO_BIAS = 3


def fc_muls(I):
    return 1 / math.sqrt(I), BMUL


@functools.lru_cache(maxsize=None)
def fc_inputs(name):
    c = FC_BY_NAME[name]
    key = "sfw.fc." + name
    return dict(xbuf=recipe_input(key + ".x", (c["B"], c["x_stride"])), w=recipe_tensor(key + ".w", (c["O"], c["I"]), 1.0),
                bias=recipe_tensor(key + ".b", (c["O"],), 1.0) if c["bias"] else None)


def fc_x(c, xbuf):
    return xbuf[:, c["x_col"]:c["x_col"] + c["I"]]


def fc_reference(x, w, bias, wmul, bmul, slope, dtype=torch.float64):
    """(out, out_abs): the definition in ``dtype`` and the same contraction on absolute values.  LeakyReLU with a slope in [0, 1] is
    1-Lipschitz, so the pre-activation's bound holds for the output, a sign flip included."""
    x, w = x.to(dtype), w.to(dtype)
    pre, pre_abs = wmul * x @ w.t(), wmul * x.abs() @ w.abs().t()
    if bias is not None:
        pre, pre_abs = pre + bmul * bias.to(dtype), pre_abs + (bmul * bias.to(dtype)).abs()
    return lrelu(pre, slope), pre_abs


@functools.lru_cache(maxsize=None)
def fc_case_reference(name, slope):
    c, t = FC_BY_NAME[name], fc_inputs(name)
    return fc_reference(fc_x(c, t["xbuf"]), t["w"], t["bias"], *fc_muls(c["I"]), slope)


def fc_fake_pointers(c):
    return 0x100000 + 4 * (c["x_off"] + c["x_col"]), 0x800000 + 4 * c["w_off"]


def fc_form(L, x_ptr, x_stride, w_ptr, I, O, B):
    f = L.SmallForm()
    L.check(L.lib().spk_fc_fwd_form(x_ptr, x_stride, w_ptr, I, O, B, f), "spk_fc_fwd_form")
    return {n: getattr(f, n) for n, _ in L.SmallForm._fields_ if n != "reserved"}


def fc_branches(c, f, L):
    B, I, O = c["B"], c["I"], c["O"]
    k = L.FC_KERNELS[f["kernel"]]
    out = {f"fc.{k}"}
    assert f["batch_passes"] == -(-B // 8)
    if k in ("scalar", "vec", "vec512"):
        assert f["grid_x"] == -(-O // 4)
        if O % 4:
            out.add(f"fc.{k}.O%4={O % 4}")
    if k == "scalar":
        out.add("fc.scalar." + ("I%4" if I % 4 else ("x misaligned" if c["x_off"] % 4 else ("w misaligned" if c["w_off"] % 4 else
                                                                                              ("x_stride%4" if c["x_stride"] % 4 else "?")))))
    if k == "vec":
        ragged = I % 256 != 0
        out.add({(1, True): "fc.vec.one ragged trip", (2, True): "fc.vec.two trips, ragged last", (4, False): "fc.vec.four full trips"}
                .get((f["row_trips"], ragged), f"fc.vec.trips{f['row_trips']}"))
    if k == "vec512":
        out.add(f"fc.vec512.B{B}")
        if c["x_stride"] > I:
            out.add("fc.vec512.strided x")
    if k == "wide":
        assert f["grid_x"] == O
        if f["row_trips"] == 1 and I % 1024:
            out.add("fc.wide.one trip, I%1024")
        if f["row_trips"] == 2:
            out.add("fc.wide.two trips" + (", ragged" if I % 1024 else ""))
        if I % 1024 == 0 and I <= 6144:
            out.add("fc.wide.wide4-eligible I, O%4")
    if k == "wide4":
        assert f["grid_x"] * 4 == O and f["U"] * 1024 == I
        out.add(f"fc.wide4.U{f['U']}.B{B}")
    if not c["bias"]:
        out.add(f"fc.{k}.no bias")
    if c["out"] is not None and c["out"][1] > O:
        out.add("fc.out_stride>O")
    return out


def fc_selector_indices(I):
    """Columns a selector weight picks: the ends, the float4 seams, the 256-float trip seam, the 1024-float chunk seams and the
    seam between the wide kernel's two trips."""
    want = [0, 3, 4, 255, 256, I - 1, 1023, 1024, 6143, 6144, I - 4]
    return sorted({i for i in want if 0 <= i < I})


# kernel form -> (B, I): an exact selector test for each
FC_SELECTOR_SHAPES = {"scalar": (11, 70), "vec": (11, 1028), "vec512": (11, 512), "wide": (11, 2052), "wide.two trips": (11, 8192),
                      "wide4.U2": (11, 2048), "wide4.U6": (11, 6144)}


# ---- upfirdn2d -------------------------------------------------------------------------------------------------------------------
# dyadic, asymmetric 1-D factors with fx != fy: the outer product is exact in float32, so is separate()'s factorisation, and a
# transposed or unflipped filter changes the answer
FACTORS = {
    "a4": ([1, 2, 4, 8], 16, [1, 3, 5, 7], 16), "a3": ([1, 2, 4], 8, [3, 1, 4], 8), "a2": ([1, 3], 4, [5, 3], 8),
    "a5": ([1, 2, 4, 2, 1], 16, [1, 3, 5, 3, 2], 16), "a7": ([1, 2, 3, 4, 5, 6, 7], 32, [7, 1, 2, 8, 3, 1, 4], 32),
    "row0": ([0, 1, 2, 1], 4, [1, 3, 5, 7], 16),        # first row zero: separate()'s pivot is (1, 0)
    "col0": ([1, 2, 4, 8], 16, [0, 1, 2, 1], 4),        # first column zero: the pivot is (0, 1)
    "neg": ([1, -2, 4, 8], 16, [1, 3, -5, 7], 16),
}


def ufd_filter(name):
    """The 2-D filter f[i][j] = fy[i] * fx[j], float32."""
    if name == "nonsep3":                                # rank two: the outer product plus 1/8 at one corner
        f = ufd_filter("a3").clone()
        f[2, 0] += 0.125
        return f
    if name == "m123":                                   # not dyadic: rank one only to within rounding
        return M.make_kernel((1, 2, 3))
    fy, dy, fx, dx = FACTORS[name]
    return (torch.tensor(fy, dtype=torch.float32) / dy)[:, None] * (torch.tensor(fx, dtype=torch.float32) / dx)[None, :]


def ufd_out(n, up, down, pad, k):
    return (n * up + pad[0] + pad[1] - k) // down + 1


def _size_for(up, down, pad, k, lo, hi, sizes):
    for n in sizes:
        if lo <= ufd_out(n, up, down, pad, k) <= hi:
            return n
    raise ValueError((up, down, pad, k, lo, hi))


def ufd(name, up, down, pad, filt, planes, H, W, *labels):
    return dict(kind="ufd", name=name, up=up, down=down, pad=tuple(pad), filt=filt, planes=tuple(planes), H=H, W=W, labels=set(labels))


SG2_PADS = {(2, 1): ((2, 1),), (1, 2): ((1, 1),), (1, 1): ((2, 1), (1, 1)), (2, 2): ((3, 2),)}     # StyleGAN2's own: up, down, blur, both
WIDTHS = (("Wo<64", 40, 63), ("64<Wo<128", 65, 127), ("Wo>128", 129, 140))


def _sep_cases():
    out = []
    for (up, down), pads in SG2_PADS.items():
        for K in (4, 3, 2):
            for wi, (wname, lo, hi) in enumerate(WIDTHS):
                pad = pads[wi % len(pads)]
                if (up, down, K, wname) == (1, 1, 4, "Wo>128"):
                    wname, lo, hi = "Wo=128", 128, 128                  # two whole waves and nothing more, once
                H = next(h for h in range(5, 10) if ufd_out(h, up, down, pad, K) % 4)
                W = _size_for(up, down, pad, K, lo, hi, range(8, 300))
                out.append(ufd(f"sep{up}{down}{K}.{wname}", up, down, pad, f"a{K}", (1, 2 + wi % 2), H, W, f"ufd.sep<{up},{down},{K}>.{wname}"))
    return out


UFD_CASES = _sep_cases() + [
    # padding edges, one instantiation per UP, two waves wide
    ufd("pad0neg.up1", 1, 1, (-3, 1), "a4", (1, 2), 9, 80, "ufd.up1.pad0<0"),
    ufd("pad0big.up1", 1, 2, (6, 1), "a4", (1, 2), 7, 140, "ufd.up1.pad0>k"),
    ufd("pad1neg.up1", 1, 1, (2, -3), "a3", (2, 1), 9, 75, "ufd.up1.pad1<0"),
    ufd("pad0neg.up2", 2, 1, (-3, 1), "a4", (1, 2), 6, 40, "ufd.up2.pad0<0"),
    ufd("pad0big.up2", 2, 2, (7, 2), "a4", (1, 2), 5, 70, "ufd.up2.pad0>k"),
    ufd("pad1neg.up2", 2, 1, (2, -3), "a3", (2, 1), 5, 40, "ufd.up2.pad1<0"),
    # <2,2,3> with pad0 = 3 meets a sample under its centre tap alone; an even pad0 uses the outer two
    ufd("sep223.evenpad0", 2, 2, (2, 2), "a3", (1, 2), 6, 70, "ufd.sep<2,2,3>.even pad0"),
    # separate()'s edges
    ufd("pivot.row", 1, 1, (2, 1), "row0", (1, 2), 6, 70, "ufd.sep.pivot below row 0"),
    ufd("pivot.col", 2, 1, (2, 1), "col0", (1, 2), 6, 40, "ufd.sep.pivot right of column 0"),
    ufd("negtap", 1, 2, (1, 1), "neg", (1, 2), 7, 70, "ufd.sep.negative tap"),
    ufd("nondyadic", 1, 1, (1, 1), "m123", (1, 2), 7, 70, "ufd.sep.non-dyadic"),
    # the generic kernel
    ufd("gen.nonsep3", 1, 1, (1, 1), "nonsep3", (1, 2), 7, 70, "ufd.generic.rank two"),
    ufd("gen.k5", 1, 1, (2, 2), "a5", (1, 2), 7, 37, "ufd.generic.k5"),
    ufd("gen.k7", 2, 1, (4, 3), "a7", (1, 2), 5, 21, "ufd.generic.k7"),
    ufd("gen.up3", 3, 1, (2, 1), "a4", (1, 2), 5, 23, "ufd.generic.up3"),
    ufd("gen.down3", 1, 3, (2, 1), "a4", (1, 2), 11, 70, "ufd.generic.down3"),
    # the one deliberately large shape: more than 256 * 16 * 256 outputs, so every thread takes a second trip
    ufd("gen.gridloop", 1, 1, (1, 1), "nonsep3", (1, 5), 512, 512, "ufd.generic.grid loop"),
]

# exact impulse test: one-hot columns of a 130-wide row, the K = 4 filter on these (up, down, pad)
IMPULSE_W = 130
IMPULSE_COLS = (0, 31, 32, 63, 64, 65, IMPULSE_W - 1)
IMPULSE_FORMS = ((2, 1, (2, 1)), (1, 2, (1, 1)), (2, 2, (3, 2)), (1, 1, (2, 1)))


def impulse_input(c):
    x = torch.zeros(1, 1, 5, IMPULSE_W)
    x[0, 0, 2, c] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def ufd_input(name):
    c = UFD_BY_NAME[name]
    return recipe_input("sfw.ufd." + name, c["planes"] + (c["H"], c["W"]))


def ufd_reference(x, f, up, down, pad, dtype=torch.float64):
    """(y, y_abs, window): oracle.modconv_ref.upfirdn2d -- zero-insert, pad / crop, F.conv2d with the flipped filter, decimate -- on
    the filter values as passed, the same on absolute values, and the sum of |x| under each output's window."""
    x, f = x.to(dtype), f.to(dtype)
    return (M.upfirdn2d(x, f, up, down, pad), M.upfirdn2d(x.abs(), f.abs(), up, down, pad),
            M.upfirdn2d(x.abs(), torch.ones_like(f), up, down, pad))


@functools.lru_cache(maxsize=None)
def ufd_case_reference(name):
    c = UFD_BY_NAME[name]
    return ufd_reference(ufd_input(name), ufd_filter(c["filt"]), c["up"], c["down"], c["pad"])


def ufd_atol(c, window):
    """Only the non-dyadic filter has one: separate() accepts factors whose product is within 1e-6 * max|f| of every tap, so an
    output may differ from the 2-D filter's by that much times the |x| under its window.  Derived, not measured."""
    if c["filt"] != "m123":
        return 1e-30
    return 1e-6 * float(ufd_filter("m123").abs().max()) * window + 1e-30


def ufd_form(L, f2d, planes, H, W, up, down, pad):
    k = f2d.shape[0]
    arr = (L.C.c_float * (k * k))(*f2d.flatten().tolist())
    f = L.SmallForm()
    L.check(L.lib().spk_upfirdn2d_form(arr, k, planes, H, W, up, down, pad[0], pad[1], f), "spk_upfirdn2d_form")
    return {n: getattr(f, n) for n, _ in L.SmallForm._fields_ if n != "reserved"}


def ufd_branches(c, f, L):
    up, down, pad, k = c["up"], c["down"], c["pad"], ufd_filter(c["filt"]).shape[0]
    planes = c["planes"][0] * c["planes"][1]
    Ho, Wo = ufd_out(c["H"], up, down, pad, k), ufd_out(c["W"], up, down, pad, k)
    assert (f["Ho"], f["Wo"]) == (Ho, Wo)
    kern = L.UPFIRDN_KERNELS[f["kernel"]]
    out = {f"ufd.{kern}"}
    if pad[0] < 0:
        out.add(f"ufd.up{up}.pad0<0")
    if pad[0] > k:
        out.add(f"ufd.up{up}.pad0>k")
    if pad[1] < 0:
        out.add(f"ufd.up{up}.pad1<0")
    if kern == "sep":
        assert (f["UP"], f["DOWN"], f["K"]) == (up, down, k) and (f["grid_x"], f["grid_y"], f["grid_z"]) == (-(-Wo // 64), -(-Ho // 4), planes)
        inst = f"ufd.sep<{up},{down},{k}>"
        out.update({inst, f"ufd.sep.NLD{f['NLD']}"})
        if f["grid_x"] == 1 and Wo < 64:
            out.add(inst + ".Wo<64")
        if f["grid_x"] == 2 and Wo % 64:
            out.add(inst + ".64<Wo<128")                   # blockIdx.x = 1, a ragged last wave
        if f["grid_x"] == 2 and Wo == 128:
            out.add(inst + ".Wo=128")
        if f["grid_x"] == 3:
            out.add(inst + ".Wo>128")
        if (up, down, k) == (2, 2, 3) and pad[0] % 2 == 0:
            out.add(inst + ".even pad0")
        if Ho % 4:
            out.add("ufd.sep.Ho%4")                        # whole waves of the last workgroup leave early
        out.update({"row0": {"ufd.sep.pivot below row 0"}, "col0": {"ufd.sep.pivot right of column 0"}, "neg": {"ufd.sep.negative tap"},
                    "m123": {"ufd.sep.non-dyadic"}}.get(c["filt"], set()))
    else:
        assert f["grid_x"] == max(1, min(-(-planes * Ho * Wo // 256), 4096))
        if f["grid_loop"]:
            out.add("ufd.generic.grid loop")
        if c["filt"] == "nonsep3":
            out.add("ufd.generic.rank two")
        if k > 4:
            out.add(f"ufd.generic.k{k}")
        if up > 2:
            out.add(f"ufd.generic.up{up}")
        if down > 2:
            out.add(f"ufd.generic.down{down}")
    return out


# ---- the modulated toRGB 1x1, with and without a skip ----------------------------------------------------------------------------
def rgb(name, B, C, O, H, W, labels, skip_labels=None, bias=True, misaligned=False, skip_only=False):
    """``labels``: what the launch without a skip is named for, ``skip_labels``: the launch with one (None: the case runs only
    without; ``skip_only``: only with)."""
    return dict(kind="rgb", name=name, B=B, C=C, O=O, H=H, W=W, labels=set(labels), skip_labels=None if skip_labels is None else set(skip_labels),
                bias=bias, misaligned=misaligned, skip_only=skip_only)


RGB_CASES = [
    rgb("cs.q1", 2, 64, 3, 2, 2, ["rgb.mod.csplit.Q1"], ["rgb.skip.scalar.W%4==2"]),       # (a skip with W = 2 leaves no whole quad in a row)
    rgb("cs.q2", 1, 96, 2, 2, 4, ["rgb.mod.csplit.Q2"], ["rgb.skip.csplit.Q2", "rgb.skip.every pixel on the border"]),     # skip 1 x 2
    rgb("cs.q4", 2, 128, 4, 4, 4, ["rgb.mod.csplit.Q4", "rgb.mod.no bias"], ["rgb.skip.csplit.Q4", "rgb.skip.no bias"], bias=False),
    rgb("cs.q8", 1, 64, 1, 4, 8, ["rgb.mod.csplit.Q8"], ["rgb.skip.csplit.Q8", "rgb.skip.csplit.W8"]),
    rgb("cs.q16", 2, 100, 3, 12, 12, ["rgb.mod.csplit.Q16, ragged last workgroup", "rgb.mod.csplit.C%16"],
        ["rgb.skip.csplit.Q16, ragged last workgroup", "rgb.skip.csplit.C%16"]),
    rgb("vec.c32", 2, 32, 3, 16, 16, ["rgb.mod.vec.C<64"], ["rgb.skip.vec.C<64"]),
    rgb("vec.c64.b512", 512, 64, 3, 2, 4, ["rgb.mod.vec.C>=64, gate closed"], ["rgb.skip.vec.C>=64, gate closed"]),
    rgb("scalar.hw63", 2, 70, 4, 7, 9, ["rgb.mod.scalar.HW%4"]),
    rgb("scalar.xoff", 2, 64, 3, 16, 16, ["rgb.mod.scalar.misaligned"], ["rgb.skip.scalar.misaligned"], misaligned=True),
    rgb("skip.w10", 1, 70, 3, 6, 10, [], ["rgb.skip.scalar.W%4==2"], skip_only=True),
    rgb("skip.c64.512", 2, 64, 3, 512, 512, [], ["rgb.skip.vec.C>=64, gate closed", "rgb.skip.vec.one full grid"], skip_only=True),
    # more than 2048 * 256 quads / pixels of ONE image: the grid-stride loops' second trip (two channels keep it to 17 MB)
    rgb("vec.gridloop", 1, 2, 1, 1024, 2056, ["rgb.mod.vec.grid-stride loop"], ["rgb.skip.vec.grid-stride loop"]),
    rgb("scalar.gridloop", 1, 2, 1, 513, 1025, ["rgb.mod.scalar.grid-stride loop"]),
]


def rgb_runs():
    """(case, with_skip) for every launch of the table."""
    return [(c, s) for c in RGB_CASES for s in (False, True) if (c["skip_labels"] is not None if s else not c["skip_only"])]


@functools.lru_cache(maxsize=None)
def rgb_inputs(name):
    c = RGB_BY_NAME[name]
    key, B, C, O, H, W = "sfw.rgb." + name, c["B"], c["C"], c["O"], c["H"], c["W"]
    return dict(x=recipe_input(key + ".x", (B, C, H, W)), w=recipe_tensor(key + ".w", (O, C, 1, 1), 1.0),
                mod=1.0 + 0.3 * recipe_input(key + ".mod", (B, C)), bias=recipe_tensor(key + ".b", (O,), 0.3) if c["bias"] else None,
                skip=recipe_input(key + ".skip", (B, O, H // 2, W // 2)) if c["skip_labels"] is not None else None)


def rgb_reference(x, w, mod, bias, skip, in_scale, dtype=torch.float64):
    """(y, y_abs): einsum("oc,bc,bchw->bohw") * in_scale + bias + upsample2x(skip); the [1,3,3,1] filter is non-negative, so the
    skip's term on absolute values is upsample2x(|skip|)."""
    B, C, H, W = x.shape
    O = w.shape[0]
    wm = in_scale * w.reshape(1, O, C).to(dtype) * mod.to(dtype)[:, None, :]                # [B, O, C]
    xf = x.to(dtype).flatten(2)
    y, y_abs = torch.bmm(wm, xf).view(B, O, H, W), torch.bmm(wm.abs(), xf.abs()).view(B, O, H, W)
    if bias is not None:
        y, y_abs = y + bias.to(dtype).view(1, O, 1, 1), y_abs + bias.to(dtype).abs().view(1, O, 1, 1)
    if skip is not None:
        y, y_abs = y + M.upsample2x(skip.to(dtype)), y_abs + M.upsample2x(skip.to(dtype).abs())
    return y, y_abs


def rgb_form(L, x_ptr, y_ptr, B, C, O, HW, has_skip, W):
    f = L.SmallForm()
    L.check(L.lib().spk_conv1x1_small_form(x_ptr, y_ptr, B, C, O, HW, int(has_skip), W, f), "spk_conv1x1_small_form")
    return {n: getattr(f, n) for n, _ in L.SmallForm._fields_ if n != "reserved"}


def rgb_branches(c, f, L, with_skip):
    B, C, O, H, W = c["B"], c["C"], c["O"], c["H"], c["W"]
    kern, m = L.CONV1X1_SMALL_KERNELS[f["kernel"]], "rgb." + ("skip" if with_skip else "mod")
    n4 = H * W // 4
    out = {f"{m}.{kern}", f"{m}.O{O}"}
    assert f["grid_y"] == B
    if not c["bias"]:
        out.add(m + ".no bias")
    if kern == "csplit":
        Q = f["Q"]
        assert Q == min(16, 1 << (n4.bit_length() - 1)) and f["grid_x"] == -(-n4 // Q)
        assert f["lds_bytes"] == 4 * (((O * C + 3) & ~3) + (256 // Q) * 4 * Q * 4)
        out.add(f"{m}.csplit.Q{Q}" + (", ragged last workgroup" if Q == 16 and n4 % 16 and f["grid_x"] > 1 else ""))
        if C % 16:
            out.add(m + ".csplit.C%16")
        if W == 8:
            out.add(m + ".csplit.W8")
    else:
        assert f["lds_bytes"] == 4 * O * C
    if kern == "vec":
        assert f["grid_x"] == max(1, min(-(-n4 // 256), 2048))
        out.add(m + (".vec.C<64" if C < 64 else ".vec.C>=64, gate closed"))
        if n4 > 256 * f["grid_x"]:
            out.add(m + ".vec.grid-stride loop")
        if n4 == 256 * f["grid_x"] and f["grid_x"] > 1:
            out.add(m + ".vec.one full grid")
    if kern == "scalar":
        assert f["grid_x"] == max(1, min(-(-H * W // 256), 2048))
        if H * W > 256 * f["grid_x"]:
            out.add(m + ".scalar.grid-stride loop")
        out.add(m + ".scalar." + ("HW%4" if H * W % 4 else ("misaligned" if c["misaligned"] else ("W%4==2" if with_skip and W % 4 == 2 else "?"))))
    if with_skip and (H, W) == (2, 4):
        out.add(m + ".every pixel on the border")
    return out


# ---- fromRGB expand --------------------------------------------------------------------------------------------------------------
def expand(name, B, C, O, H, W, scale, bias, slope):
    n4 = H * W // 4
    labels = {f"exp.C{C}", f"exp.O{O}", f"exp.n4={n4}", f"exp.B{B}", "exp.scale" if scale else "exp.no scale", "exp.bias" if bias else "exp.no bias",
              f"exp.slope{slope}"}
    if not scale and not bias:
        labels.add("exp.neither scale nor bias")
    if n4 > 256:
        labels.add("exp.two workgroup columns, the second ragged")
    return dict(kind="expand", name=name, B=B, C=C, O=O, H=H, W=W, scale=scale, bias=bias, slope=slope, labels=labels)


EXPAND_CASES = [
    expand("c1.o1", 1, 1, 1, 2, 2, False, False, 1.0),
    expand("c2.o5", 3, 2, 5, 16, 16, True, True, 0.2),
    expand("c2.o33.bare", 1, 2, 33, 2, 2, False, False, 0.2),
    expand("c3.o33", 1, 3, 33, 32, 32, True, False, 0.2),
    expand("c3.o128", 3, 3, 128, 40, 40, False, True, 0.2),
    expand("c4.o5", 3, 4, 5, 40, 40, True, True, 1.0),
    expand("c4.o128", 1, 4, 128, 16, 16, True, True, 0.2),
    expand("c1.o5", 3, 1, 5, 32, 32, False, True, 1.0),
]


@functools.lru_cache(maxsize=None)
def expand_inputs(name):
    c = EXPAND_BY_NAME[name]
    key = "sfw.exp." + name
    return dict(x=recipe_input(key + ".x", (c["B"], c["C"], c["H"], c["W"])), w=recipe_tensor(key + ".w", (c["O"], c["C"], 1, 1), 1.0),
                bias=recipe_tensor(key + ".b", (c["O"],), 0.5) if c["bias"] else None,
                scale=torch.tensor([0.37], dtype=torch.float32) if c["scale"] else None)


def expand_reference(x, w, bias, scale, slope, dtype=torch.float64):
    O, C = w.shape[:2]
    w2 = w.reshape(O, C).to(dtype) * (scale.to(dtype) if scale is not None else 1.0)
    pre, pre_abs = torch.einsum("oc,bchw->bohw", w2, x.to(dtype)), torch.einsum("oc,bchw->bohw", w2.abs(), x.to(dtype).abs())
    if bias is not None:
        pre, pre_abs = pre + bias.to(dtype).view(1, O, 1, 1), pre_abs + bias.to(dtype).abs().view(1, O, 1, 1)
    return lrelu(pre, slope), pre_abs


FC_BY_NAME = {c["name"]: c for c in FC_CASES}
UFD_BY_NAME = {c["name"]: c for c in UFD_CASES}
RGB_BY_NAME = {c["name"]: c for c in RGB_CASES}
EXPAND_BY_NAME = {c["name"]: c for c in EXPAND_CASES}
for _t, _n in ((FC_CASES, FC_BY_NAME), (UFD_CASES, UFD_BY_NAME), (RGB_CASES, RGB_BY_NAME), (EXPAND_CASES, EXPAND_BY_NAME)):
    assert len(_t) == len(_n)


def query(c, L, with_skip=False):
    """The labels the library's own dispatch says ``c`` reaches (made-up pointers of the case's alignment; nothing is launched)."""
    if c["kind"] == "fc":
        x_ptr, w_ptr = fc_fake_pointers(c)
        return fc_branches(c, fc_form(L, x_ptr, c["x_stride"], w_ptr, c["I"], c["O"], c["B"]), L)
    if c["kind"] == "ufd":
        f2d = ufd_filter(c["filt"])
        return ufd_branches(c, ufd_form(L, f2d, c["planes"][0] * c["planes"][1], c["H"], c["W"], c["up"], c["down"], c["pad"]), L)
    if c["kind"] == "rgb":
        off = 4 if c["misaligned"] else 0
        return rgb_branches(c, rgb_form(L, 0x100000 + off, 0x800000 + off, c["B"], c["C"], c["O"], c["H"] * c["W"], with_skip, c["W"] if with_skip else 0),
                            L, with_skip)
    assert c["kind"] == "expand"
    return set(c["labels"])                               # one kernel, one launch form: the labels are the case's own shape
