"""Case table, fp64 reference, fp32 Winograd emulation and schedule model of the Winograd forward (csrc/conv3x3_wino_f32.hip) -- test
infrastructure, CPU only; the role tests/direct_conv_cases.py has for the direct conv.

A case names a launch (output size per image, channels, groups, requested ksplit, operands, a WALK TARGET) and DECLARES the fields of
``spk_wino_form`` it reaches; ``spk_conv2d_wino_form`` -- the launch's own planner -- decides whether it does
(tests/test_wino_forms_cpu.py without a GPU, tests/test_wino_branches_gpu.py again with the real pointers and the device's CU count).
The batch is not part of a case: ``batch_for(case, n_cu, L)`` is the smallest B at which the launch meets the walk target on a device
of ``n_cu`` compute units -- 2 images for "one item per workgroup", else the first B at which the most loaded persistent workgroup
walks >= ``walk`` items and the least loaded one fewer.

``reference(case, B)`` evaluates the whole operator in fp64:
    bilinear x2 | batch scale -> conv * out_scale * out_scale_dev * demod -> + bias + noise_w * noise -> LeakyReLU * act_gain -> y_pre
    -> style (rows wider than 2 Cy) -> + y (accumulate) -> the 1x1 to 3 channels + rgb bias.
``emulation(case)`` is the same chain in fp32 with the convolution as THIS kernel forms it (the direct form's rounding is not this
kernel's): U = G g G^T as pack_wino_kernel writes it, V = B^T d B rows first, M accumulated sequentially over ci, Y = A^T M A in the
epilogue's order of sums, on the case's first two images.  The bound is measured on the two references, never on the kernel: per
output tensor max(4 x rel-L2(emulation, fp64), sqrt(9 Cin) 2^-24) (a toRGB image is a second contraction behind the first and has its
own error; a LEAN_NOSTORE launch has no other output), the case's bound the largest of them; a single element:
|y - ref| <= MAX_FACTOR x bound x rms(ref).

``schedule(form)`` spells the kernel's dealing of work items to persistent workgroups out in Python.  It proves properties of CASES
(which images and slices a workgroup's consecutive items lie in); it is never a reference for values."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle.weights_recipe import recipe_input, recipe_tensor

TOL = 5e-6                      # the aggregate rel-L2 of tests/test_wino_gpu.py: no case's bound may exceed it
MAX_FACTOR = 8.0                # as tests/direct_conv_cases.py
OUT_SCALE, SLOPE, ACT_GAIN, SCALE_DEV = 0.37, 0.2, 2.0 ** 0.5, 1.25
WIDE, SQUARE = 0, 1
GENERIC, LEAN, LEAN_NOSTORE = 0, 1, 2
SIZE_CAP = 256 << 20            # bytes of x + y + the fp64 reference of y at 256 CUs
LEAN_SET = ("bias", "noise", "lrelu", "style", "scale_dev")     # the full flag set of a LEAN launch (and of a fused toRGB)
FULL = LEAN_SET + ("y_pre", "accum")                            # ... of a GENERIC one
MOD_SET = FULL + ("bscale", "demod")


def case(name, H, W, Cin, Cout, opts=(), G=1, want=1, walk=1, slope=SLOPE, misalign_x=False, like=None, **declares):
    """``H x W``: the OUTPUT size of one image (x2: x has half of it).  ``opts``: bias noise lrelu style y_pre accum scale_dev bscale demod
    x2 rgb nostore.  ``want``: the requested ksplit (1: unsliced).  ``walk``: 1 = one item per workgroup (B = 2), n > 1 = the most loaded workgroup walks >= n items and the least loaded
    one fewer.  ``slope``: the LeakyReLU's.  ``misalign_x``: x starts 4 bytes off a 16-byte boundary.  ``like``: the case whose operands
    this one shares.  ``declares``: fields of spk_wino_form."""
    return dict(name=name, H=H, W=W, Cin=Cin, Cout=Cout, opts=frozenset(opts), G=G, want=want, walk=walk, slope=slope,
                misalign_x=misalign_x, like=like, declares=declares)


def in_hw(c):
    return (c["H"] // 2, c["W"] // 2) if "x2" in c["opts"] else (c["H"], c["W"])


def regions_per_image(c, form):
    rh, rw = (16, 16) if form["shape"] == SQUARE else (8, 32)
    return (c["H"] // rh) * (c["W"] // rw)


# ---- operands ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _inputs(name, B):
    c = BY_NAME[name]
    Cin, Cout, G, H, W, o = c["Cin"], c["Cout"], c["G"], c["H"], c["W"], c["opts"]
    Hs, Ws = in_hw(c)
    Cy = G * Cout
    tag = f"wino.{c['like'] or name}"
    # (the recipes fill row-major from one stream: the first images of a larger batch are the smaller batch's)
    t = dict(x=recipe_input(f"{tag}.x", (B, G * Cin, Hs, Ws)))
    t["w"] = [recipe_tensor(f"{tag}.w{g}", (Cout, Cin, 3, 3), (9 * Cin) ** -0.5) for g in range(G)]
    if "bias" in o:
        t["bias"] = recipe_tensor(f"{tag}.b", (Cy,), 0.3)
    if "noise" in o:
        t["noise_w"] = recipe_tensor(f"{tag}.nw", (Cy,), 0.2)
        t["noise"] = recipe_input(f"{tag}.nz", (B, 1, H, W))
    if "style" in o:                           # rows [s0 (Cy) | s1 (Cy) | 3 unused floats]: style_stride > 2 Cy
        t["style"] = recipe_input(f"{tag}.st", (B, 2 * Cy + 3)) * 0.3
    if "accum" in o:
        t["y0"] = recipe_input(f"{tag}.y0", (B, Cy, H, W)) * 0.5
    if "bscale" in o:
        t["bscale"] = 1.0 + 0.3 * recipe_input(f"{tag}.s", (B, Cin), "uniform")
    if "demod" in o:
        t["demod"] = 0.5 + recipe_input(f"{tag}.d", (B, Cout), "uniform").abs()
    if "rgb" in o:
        t["rgb_w"] = recipe_tensor(f"{tag}.rw", (3, Cout, 1, 1), Cout ** -0.5)
        t["rgb_b"] = recipe_tensor(f"{tag}.rb", (3,), 0.3)
    return t


def inputs(c, B):
    """The case's operands at batch B (fp32, CPU).  Shared: do not write."""
    return _inputs(c["name"], B)


def scalars(c):
    """(out_scale, out_scale_dev | None, slope | None, act_gain) as the launch passes them."""
    o = c["opts"]
    return OUT_SCALE, SCALE_DEV if "scale_dev" in o else None, c["slope"] if "lrelu" in o else None, ACT_GAIN if "lrelu" in o else 1.0


# ---- the operator chain ----------------------------------------------------------------------------------------------------------
def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _staged_input(c, t, dtype):
    x = t["x"].to(dtype)
    if "bscale" in c["opts"]:            # (ungrouped launches only)
        x = x * t["bscale"].to(dtype).view(x.shape[0], -1, 1, 1)
    if "x2" in c["opts"]:
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    return x


def _epilogue(c, t, v, dtype):
    """-> (y_pre, y, rgb | None) from the bare convolution ``v`` [B, Cy, H, W]."""
    o, Cy = c["opts"], c["G"] * c["Cout"]
    B = v.shape[0]
    out_scale, scale_dev, slope, gain = scalars(c)
    sc = _f32(out_scale) * (_f32(scale_dev) if scale_dev is not None else 1.0)
    v = v * (sc if dtype == torch.float64 else _f32(sc))
    if "demod" in o:
        v = v * t["demod"].to(dtype).view(B, Cy, 1, 1)
    if "bias" in o:
        v = v + t["bias"].to(dtype).view(1, Cy, 1, 1)
    if "noise" in o:
        v = v + t["noise_w"].to(dtype).view(1, Cy, 1, 1) * t["noise"].to(dtype)
    if slope is not None:
        v = torch.where(v > 0, v, v * _f32(slope)) * _f32(gain)
    pre = v
    if "style" in o:
        st = t["style"].to(dtype)
        v = v * (st[:, :Cy, None, None] + 1.0) + st[:, Cy:2 * Cy, None, None]
    if "accum" in o:
        v = v + t["y0"].to(dtype)
    rgb = None
    if "rgb" in o:
        rgb = F.conv2d(v, t["rgb_w"].to(dtype), t["rgb_b"].to(dtype))
    return pre, v, rgb


def chain64(c, t):
    """(y_pre, y, rgb) of the whole operator in fp64 on the operands ``t``."""
    x = _staged_input(c, t, torch.float64)
    Cin = c["Cin"]
    v = torch.cat([F.conv2d(x[:, g * Cin:(g + 1) * Cin], t["w"][g].double(), padding=1) for g in range(c["G"])], 1)
    return _epilogue(c, t, v, torch.float64)


def _g1(a0, a1, a2):
    """Rows of G = [1,0,0], [.5,.5,.5], [.5,-.5,.5], [0,0,1] in the packer's order of operations."""
    return [a0, 0.5 * ((a0 + a2) + a1), 0.5 * ((a0 + a2) - a1), a2]


def _bt1(d0, d1, d2, d3):
    return [d0 - d2, d1 + d2, d2 - d1, d1 - d3]


def wino_conv32(x, w, mod=None):
    """conv3x3(x, w, pad 1) in fp32 as F(2x2, 3x3): x [B, Cin, H, W], w [Cout, Cin, 3, 3], both fp32 -> [B, Cout, H, W].  ``mod`` [B, Cin]:
    the modulated conv, conv3x3(x * mod): the kernel multiplies the transformed patches, B^T (d s) B = s B^T d B."""
    assert x.dtype == torch.float32 and w.dtype == torch.float32
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    t = _g1(w[:, :, 0, :], w[:, :, 1, :], w[:, :, 2, :])                                    # (G g)[i]: [Cout, Cin, 3]
    U = torch.stack([u for i in range(4) for u in _g1(t[i][..., 0], t[i][..., 1], t[i][..., 2])])        # [16 = 4 i + j, Cout, Cin]
    xp = F.pad(x, (1, 1, 1, 1))
    d = [[xp[:, :, r:r + H:2, q:q + W:2] for q in range(4)] for r in range(4)]                # the tiles' 4 x 4 patches, [B, Cin, H/2, W/2] each
    tq = [_bt1(d[0][q], d[1][q], d[2][q], d[3][q]) for q in range(4)]                        # B^T d over the rows: tq[column][i]
    V = torch.stack([v for i in range(4) for v in _bt1(tq[0][i], tq[1][i], tq[2][i], tq[3][i])])         # [16, B, Cin, H/2, W/2]
    if mod is not None:
        V = V * mod.view(1, B, Cin, 1, 1)
    M = torch.zeros((16, B, Cout, H // 2, W // 2), dtype=torch.float32)
    for ci in range(Cin):                                                                 # sequentially over ci, fp32
        M += U[:, None, :, ci, None, None] * V[:, :, ci, None]
    m = [[M[4 * i + j] for j in range(4)] for i in range(4)]
    s0 = [(m[i][0] + m[i][1]) + m[i][2] for i in range(4)]
    s1 = [(m[i][1] - m[i][2]) - m[i][3] for i in range(4)]
    y = torch.empty((B, Cout, H, W), dtype=torch.float32)
    y[:, :, 0::2, 0::2] = (s0[0] + s0[1]) + s0[2]
    y[:, :, 0::2, 1::2] = (s1[0] + s1[1]) + s1[2]
    y[:, :, 1::2, 0::2] = (s0[1] - s0[2]) - s0[3]
    y[:, :, 1::2, 1::2] = (s1[1] - s1[2]) - s1[3]
    return y


def chain32(c, t):
    """The chain in fp32 with the Winograd arithmetic of the kernel."""
    Cin, G = c["Cin"], c["G"]
    x = _staged_input(dict(c, opts=c["opts"] - {"bscale"}), t, torch.float32)
    mod = t["bscale"] if "bscale" in c["opts"] else None
    outs = [wino_conv32(x[:, g * Cin:(g + 1) * Cin].contiguous(), t["w"][g], mod) for g in range(G)]
    return _epilogue(c, t, torch.cat(outs, 1), torch.float32)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def outputs(c):
    """Names of the tensors the launch writes, in the order (y, y_pre, rgb)."""
    o = c["opts"]
    return [n for n, on in (("y", "nostore" not in o), ("pre", "y_pre" in o), ("rgb", "rgb" in o)) if on]


@functools.lru_cache(maxsize=None)
def _bounds(name):
    c = BY_NAME[name]
    t = inputs(c, 2)
    ref = dict(zip(("pre", "y", "rgb"), chain64(c, t)))
    emu = dict(zip(("pre", "y", "rgb"), chain32(c, t)))
    floor = math.sqrt(9 * c["Cin"]) * 2.0 ** -24
    per = {n: max(4 * rel_l2(emu[n], ref[n]), floor) for n in outputs(c)}
    return dict(per=per, bound=max(per.values()), ref=ref, emu=emu)


def bounds(c):
    """``per``: the bound of every output tensor; ``bound``: the case's; ``ref`` / ``emu``: the two chains on the first two images."""
    return _bounds(c["name"])


@functools.lru_cache(maxsize=2)
def _reference(name, B):
    c = BY_NAME[name]
    return dict(zip(("pre", "y", "rgb"), chain64(c, inputs(c, B))))


def reference(c, B):
    """fp64 ``y`` / ``pre`` / ``rgb`` of the case at batch B.  Shared: do not write."""
    return _reference(c["name"], B)


def figures(c, got, want):
    """``got`` / ``want``: {y, pre, rgb} of the same images -> {what: (figure, limit)}: every figure must stay at or below its limit."""
    per = bounds(c)["per"]
    out = {}
    for n in outputs(c):
        g, w = got[n].detach().cpu().double(), want[n]
        assert g.shape == w.shape, (n, g.shape, w.shape)
        out[f"{n} rel-L2"] = (rel_l2(g, w), per[n])
        out[f"{n} max|diff|"] = (float((g - w).abs().max()), MAX_FACTOR * per[n] * rms(w))
    return out


# ---- the descriptor, for the query without a device --------------------------------------------------------------------------------
def flags_of(c, L):
    o = c["opts"]
    f = L.CONV_WINOGRAD
    for name, bit in (("bias", L.EPI_BIAS), ("noise", L.EPI_NOISE), ("lrelu", L.EPI_LRELU), ("style", L.EPI_STYLE), ("x2", L.CONV_UPSAMPLE2X),
                      ("accum", L.EPI_ACCUM), ("bscale", L.CONV_IN_BATCH_SCALE), ("rgb", L.EPI_TORGB)):
        if name in o:
            f |= bit
    return f


def dummy_desc(c, L, B):
    """The case's ``spk_conv2d_desc`` at batch B with made-up pointers of the case's alignment (``spk_conv2d_wino_form`` reads no memory)."""
    o = c["opts"]
    Hs, Ws = in_hw(c)
    nxt = iter(range(0x100000, 0x10000000, 0x1000))
    ptr = lambda on=True, off=False: (next(nxt) + (4 if off else 0)) if on else None
    return L.Conv2dDesc(
        x=ptr(True, c["misalign_x"]), w_packed=ptr(), bias=ptr("bias" in o), noise_w=ptr("noise" in o), noise=ptr("noise" in o),
        style=ptr("style" in o), in_scale=ptr("bscale" in o), y=ptr("nostore" not in o), y_pre=ptr("y_pre" in o),
        B=B, Cin=c["Cin"], Cout=c["Cout"], H=c["H"], W=c["W"], Hin=Hs, Win=Ws, kh=3, kw=3, stride=1,
        style_stride=2 * c["G"] * c["Cout"] + 3 if "style" in o else 0, flags=flags_of(c, L), lrelu_slope=c["slope"], out_scale=OUT_SCALE,
        config=-1, ksplit=c["want"], workspace=ptr(), workspace_bytes=1 << 40, out_scale_bc=ptr("demod" in o), act_gain=ACT_GAIN,
        groups=c["G"], group_in_stride=0 if c["G"] == 1 else c["Cin"], out_scale_dev=ptr("scale_dev" in o),
        rgb_w=ptr("rgb" in o), rgb_bias=ptr("rgb" in o), rgb_y=ptr("rgb" in o), rgb_channels=3 if "rgb" in o else 0)


def query(c, L, n_cu, B=None, desc=None):
    form = L.WinoForm()
    L.check(L.lib().spk_conv2d_wino_form(desc if desc is not None else dummy_desc(c, L, B), n_cu, form), "spk_conv2d_wino_form")
    return {n: getattr(form, n) for n, _ in L.WinoForm._fields_}


def meets_walk(c, form):
    if c["walk"] == 1:
        return form["walk_max"] == 1
    return form["walk_max"] >= c["walk"] and form["walk_min"] < form["walk_max"]


@functools.lru_cache(maxsize=None)
def _batch_for(name, n_cu, L):
    c = BY_NAME[name]
    if c["walk"] == 1:
        return 2
    for B in range(1, 4096):
        if meets_walk(c, query(c, L, n_cu, B)):
            return B
    raise AssertionError(f"{name}: no batch below 4096 meets the walk target on {n_cu} CUs")


def batch_for(c, n_cu, L):
    """The smallest B at which the case meets its walk target on ``n_cu`` compute units (the query supplies the grid)."""
    return _batch_for(c["name"], n_cu, L)


# ---- the kernel's dealing of work items, in Python -----------------------------------------------------------------------------
def schedule(form):
    """-> per workgroup (blockIdx.x) the list of (region, slice) it walks, in order.  The item list [region][slice], slice fastest, is
    cut into 8 contiguous shares (the first items % 8 one longer); workgroup wg serves share wg & 7 and takes its items
    begin + (wg >> 3) + k * (grid_x >> 3)."""
    items, gx, ks = form["items"], form["grid_x"], form["ksplit"]
    assert gx % 8 == 0 and gx >= 8
    q, r, wpx = items >> 3, items & 7, gx >> 3
    walks = []
    for wg in range(gx):
        xcd = wg & 7
        begin = xcd * q + min(xcd, r)
        end = begin + q + (1 if xcd < r else 0)
        walks.append([(it // ks, it % ks) for it in range(begin + (wg >> 3), end, wpx)])
    return walks


def walk_pairs(c, form):
    """Every (image, slice) -> (image, slice) step between consecutive items of one workgroup."""
    rpi = regions_per_image(c, form)
    return [((a[0] // rpi, a[1]), (b[0] // rpi, b[1])) for w in schedule(form) for a, b in zip(w, w[1:])]


# ---- the tables --------------------------------------------------------------------------------------------------------------------
def _kernel(mod=0, rgb=0, up=0, shape=WIDE, epi=GENERIC, **more):
    return dict(mod=mod, rgb=rgb, up=up, shape=shape, epi=epi, **more)


RGB_SET = LEAN_SET + ("rgb",)
CASES = [
    # ---- one item per workgroup (B = 2): all 22 kernel instantiations, each with the full flag set its form allows.  WIDE: 16 x 64, 2 x 2
    # regions -- every edge kind and the interior region borders; SQUARE: 32 x 16 / 48 x 16, regions stacked
    case("mod.wide", 16, 64, 32, 64, MOD_SET, **_kernel(mod=1, n_chunks=4, ksplit=1, walk_max=1, co_tiles=1, groups=1)),
    case("mod.square", 48, 16, 32, 40, MOD_SET, **_kernel(mod=1, shape=SQUARE)),
    case("plain.wide.lean", 16, 64, 32, 128, LEAN_SET, **_kernel(epi=LEAN, co_tiles=2, items=8, grid_x=8, lds_bytes=155648, finisher=0)),
    case("plain.square.lean", 32, 16, 16, 64, LEAN_SET, **_kernel(shape=SQUARE, epi=LEAN)),
    case("x2.wide.lean", 16, 64, 32, 64, LEAN_SET + ("x2",), **_kernel(up=1, epi=LEAN)),
    case("x2.square.lean", 48, 16, 16, 128, LEAN_SET + ("x2",), **_kernel(up=1, shape=SQUARE, epi=LEAN)),
    case("plain.wide.generic", 16, 64, 32, 64, FULL, **_kernel()),
    case("plain.square.generic", 48, 16, 16, 64, FULL, **_kernel(shape=SQUARE)),
    case("x2.wide.generic", 16, 64, 16, 64, FULL + ("x2",), **_kernel(up=1)),
    case("x2.square.generic", 32, 16, 32, 64, FULL + ("x2",), **_kernel(up=1, shape=SQUARE)),
    # the GENERIC rows, one cause at a time
    case("generic.cout40", 16, 64, 16, 40, LEAN_SET, **_kernel(co_tiles=1)),
    case("generic.cout200", 8, 32, 16, 200, LEAN_SET, **_kernel(co_tiles=4)),
    case("generic.y_pre", 16, 64, 16, 64, LEAN_SET + ("y_pre",), **_kernel()),
    case("generic.accum", 16, 64, 16, 64, LEAN_SET + ("accum",), **_kernel()),
    case("generic.slope", 16, 64, 16, 64, LEAN_SET, slope=1.25, **_kernel()),
    case("generic.slope.negative", 8, 32, 16, 64, ("bias", "lrelu"), slope=-0.5, **_kernel()),
    case("x2.generic.cout200", 16, 64, 16, 200, LEAN_SET + ("x2",), **_kernel(up=1, co_tiles=4)),
    # the fused toRGB: GENERIC by a partial tile (Cout 48) and by the slope, LEAN (Cout 64), LEAN_NOSTORE (Cout 64 and a partial tile)
    case("rgb.wide.generic", 16, 64, 16, 48, RGB_SET, **_kernel(rgb=1)),
    case("rgb.wide.lean", 16, 64, 32, 64, RGB_SET, **_kernel(rgb=1, epi=LEAN)),
    case("rgb.wide.nostore", 16, 64, 32, 64, RGB_SET + ("nostore",), like="rgb.wide.lean", **_kernel(rgb=1, epi=LEAN_NOSTORE)),
    case("rgb.square.generic", 32, 16, 16, 64, RGB_SET, slope=1.25, **_kernel(rgb=1, shape=SQUARE)),
    case("rgb.square.lean", 48, 16, 16, 64, RGB_SET, **_kernel(rgb=1, shape=SQUARE, epi=LEAN)),
    case("rgb.square.nostore", 48, 16, 16, 48, RGB_SET + ("nostore",), **_kernel(rgb=1, shape=SQUARE, epi=LEAN_NOSTORE)),
    case("rgb.x2.wide.generic", 16, 64, 32, 48, RGB_SET + ("x2",), **_kernel(rgb=1, up=1)),
    case("rgb.x2.wide.lean", 16, 64, 16, 64, RGB_SET + ("x2",), **_kernel(rgb=1, up=1, epi=LEAN)),
    case("rgb.x2.wide.nostore", 16, 64, 16, 64, RGB_SET + ("x2", "nostore"), like="rgb.x2.wide.lean", **_kernel(rgb=1, up=1, epi=LEAN_NOSTORE)),
    case("rgb.x2.square.generic", 48, 16, 16, 40, RGB_SET + ("x2",), **_kernel(rgb=1, up=1, shape=SQUARE)),
    case("rgb.x2.square.lean", 32, 16, 32, 64, RGB_SET + ("x2",), **_kernel(rgb=1, up=1, shape=SQUARE, epi=LEAN)),
    case("rgb.x2.square.nostore", 32, 16, 32, 64, RGB_SET + ("x2", "nostore"), like="rgb.x2.square.lean", **_kernel(rgb=1, up=1, shape=SQUARE, epi=LEAN_NOSTORE)),
    # x 4 bytes off a 16-byte boundary (the planner asks for 4-byte alignment of x only)
    case("plain.wide.lean.misx", 16, 64, 32, 128, LEAN_SET, misalign_x=True, like="plain.wide.lean", **_kernel(epi=LEAN)),
    case("x2.wide.generic.misx", 16, 64, 16, 64, FULL + ("x2",), misalign_x=True, like="x2.wide.generic", **_kernel(up=1)),
    # sliced, one item per workgroup: the partial sums leave through the LEAN rows, the epilogue runs in the finisher
    case("sliced.ks2", 16, 64, 64, 64, FULL, want=2, **_kernel(epi=LEAN, ksplit=2, chunks_per_slice=4, n_chunks=8, finisher=2)),

    # ---- walks: walk_max >= 3, walk_min < walk_max.  Cout 256 (4 channel tiles: 64 workgroups a tile on 256 CUs) keeps the batch small;
    # the toRGB's one channel tile needs > 2 x 256 regions.  Plain, x2 and MOD WIDE at 1, 2 and 3 chunk pairs per item
    case("walk.plain.wide.lean.c16", 16, 64, 16, 256, LEAN_SET, walk=3, **_kernel(epi=LEAN, n_chunks=2)),
    case("walk.plain.wide.lean.c32", 16, 64, 32, 256, LEAN_SET, walk=3, **_kernel(epi=LEAN, n_chunks=4)),
    case("walk.plain.wide.lean.c48", 24, 96, 48, 256, LEAN_SET, walk=3, **_kernel(epi=LEAN, n_chunks=6)),
    case("walk.plain.wide.generic", 16, 64, 32, 200, FULL, walk=3, **_kernel(n_chunks=4, co_tiles=4)),
    case("walk.plain.square.lean", 32, 16, 16, 256, LEAN_SET, walk=3, **_kernel(shape=SQUARE, epi=LEAN)),
    case("walk.plain.square.generic", 48, 16, 32, 256, FULL, walk=3, **_kernel(shape=SQUARE)),
    case("walk.x2.wide.lean.c16", 16, 64, 16, 256, LEAN_SET + ("x2",), walk=3, **_kernel(up=1, epi=LEAN, n_chunks=2)),
    case("walk.x2.wide.lean.c32", 24, 96, 32, 256, LEAN_SET + ("x2",), walk=3, **_kernel(up=1, epi=LEAN, n_chunks=4)),
    case("walk.x2.wide.lean.c48", 16, 64, 48, 256, LEAN_SET + ("x2",), walk=3, **_kernel(up=1, epi=LEAN, n_chunks=6)),
    case("walk.x2.wide.generic", 16, 64, 32, 200, FULL + ("x2",), walk=3, **_kernel(up=1, n_chunks=4)),
    case("walk.x2.square.lean", 48, 16, 16, 256, LEAN_SET + ("x2",), walk=3, **_kernel(up=1, shape=SQUARE, epi=LEAN)),
    case("walk.x2.square.generic", 32, 16, 32, 256, FULL + ("x2",), walk=3, **_kernel(up=1, shape=SQUARE)),
    case("walk.mod.wide.c16", 16, 64, 16, 256, MOD_SET, walk=3, **_kernel(mod=1, n_chunks=2)),
    case("walk.mod.wide.c32", 16, 64, 32, 200, MOD_SET, walk=3, **_kernel(mod=1, n_chunks=4)),
    case("walk.mod.wide.c48", 24, 96, 48, 256, MOD_SET, walk=3, **_kernel(mod=1, n_chunks=6)),
    case("walk.mod.square", 32, 16, 32, 256, MOD_SET, walk=3, **_kernel(mod=1, shape=SQUARE)),
    case("walk.rgb.lean", 16, 64, 16, 64, RGB_SET, walk=3, **_kernel(rgb=1, epi=LEAN)),
    case("walk.rgb.nostore", 16, 64, 16, 64, RGB_SET + ("nostore",), walk=3, like="walk.rgb.lean", **_kernel(rgb=1, epi=LEAN_NOSTORE)),
    case("walk.rgb.generic", 16, 64, 32, 48, RGB_SET, walk=3, **_kernel(rgb=1)),
    case("walk.rgb.x2.lean", 16, 64, 32, 64, RGB_SET + ("x2",), walk=3, **_kernel(rgb=1, up=1, epi=LEAN)),
    case("walk.rgb.x2.nostore", 16, 64, 32, 64, RGB_SET + ("x2", "nostore"), walk=3, like="walk.rgb.x2.lean", **_kernel(rgb=1, up=1, epi=LEAN_NOSTORE)),
    case("walk.rgb.x2.generic", 16, 64, 16, 48, RGB_SET + ("x2",), walk=3, **_kernel(rgb=1, up=1)),
    # sliced: the operands of an unsliced launch (every epilogue flag: it runs in the finisher), item = (region, slice).  Cout 256: 8
    # workgroups a share, a workgroup keeps its slice; Cout 192: 10 a share, the slice changes from item to item
    case("walk.sliced.ks2", 16, 64, 64, 256, FULL, want=2, walk=3, **_kernel(epi=LEAN, ksplit=2, chunks_per_slice=4, finisher=2)),
    case("walk.sliced.ks4", 16, 64, 128, 192, FULL, want=4, walk=3, **_kernel(epi=LEAN, ksplit=4, chunks_per_slice=4, co_tiles=3, finisher=2)),
    case("walk.sliced.x2.ks2", 16, 64, 64, 192, FULL + ("x2",), want=2, walk=3, **_kernel(up=1, epi=LEAN, ksplit=2, chunks_per_slice=4)),
    # grouped (the encoders' data gradients): three groups side by side, accumulate
    case("walk.groups3", 16, 64, 32, 64, ("accum",), G=3, walk=3, **_kernel(groups=3, co_tiles=3)),
    case("walk.groups3.cout40", 32, 16, 16, 40, (), G=3, walk=3, **_kernel(groups=3, co_tiles=3, shape=SQUARE)),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# (LEAN_NOSTORE case, the LEAN case of the same operands): the toRGB images must agree bit for bit
NOSTORE_VS_LEAN = [(c["name"], c["like"]) for c in CASES if "nostore" in c["opts"] and c["like"]]


def kernel_key(form):
    return (form["mod"], form["rgb"], form["up"], form["shape"], form["epi"])


# the 22 instantiations of wino_kernel: MOD x shape; {plain, x2} x shape x {GENERIC, LEAN}; toRGB x {plain, x2} x shape x {GENERIC, LEAN, LEAN_NOSTORE}
KERNELS = ({(1, 0, 0, s, GENERIC) for s in (WIDE, SQUARE)} | {(0, 0, u, s, e) for u in (0, 1) for s in (WIDE, SQUARE) for e in (GENERIC, LEAN)} |
           {(0, 1, u, s, e) for u in (0, 1) for s in (WIDE, SQUARE) for e in (GENERIC, LEAN, LEAN_NOSTORE)})
assert len(KERNELS) == 22
# the forms that are walked: (mod, rgb, up, shape, epi, sliced, grouped)
WALKED = ({(0, 0, u, s, e, 0, 0) for u in (0, 1) for s in (WIDE, SQUARE) for e in (GENERIC, LEAN)} | {(1, 0, 0, s, GENERIC, 0, 0) for s in (WIDE, SQUARE)} |
          {(0, 1, u, WIDE, e, 0, 0) for u in (0, 1) for e in (GENERIC, LEAN, LEAN_NOSTORE)} |
          {(0, 0, 0, WIDE, LEAN, 1, 0), (0, 0, 1, WIDE, LEAN, 1, 0), (0, 0, 0, WIDE, GENERIC, 0, 1), (0, 0, 0, SQUARE, GENERIC, 0, 1)})
