"""Case table of the GEMM forms of a stride-1 1x1 conv (csrc/conv1x1_gemm.hip: tile config 12; csrc/conv1x1_gemm2.hip: configs 14
and 15) and of the 7x7 stride-2 stem kernel (csrc/conv7x7_stem.hip: config 16) -- test infrastructure, CPU only.

The cases are ``direct_conv_cases.case`` records and go through that module's machinery (``inputs``, ``reference``, ``figures``):
they are entered into its ``BY_NAME``.  A case forces its config, names its operands and DECLARES the fields of ``spk_gemm_form``
it reaches; ``spk_conv2d_gemm_form`` -- the planners those launches run (plan_1x1_gemm / plan_1x1_gemm2 / plan_stem) -- decides whether it does
(tests/test_gemm_conv_forms_cpu.py without a GPU, tests/test_gemm_conv_branches_gpu.py again with the real pointers).
``branches(c, form)`` names what a case covers, from the form the library answered and the case's operands."""
import numpy as np

import direct_conv_cases as D

GEMM, STEM = "gemm1x1", "stem"


def g(name, config, B, Cin, Cout, H, W, **kw):
    return D.case(name, GEMM, 1, 1, B, Cin, Cout, H, W, config, **kw)


def stem(name, B, Hin, Win, **kw):
    return D.case(name, STEM, 7, 2, B, 3, 64, Hin, Win, 16, **kw)


OFF = ("unit_scale",)                                   # every flag off, out_scale 1
RES = ("residual", "lrelu", "accum")                    # residual -> lrelu * act_gain -> accumulate, out_scale 0.37
AFF = ("affine", "bias", "lrelu")
CASES = [
    # -- config 12: 32-channel k-tiles (a ragged last one is zero-filled), 128co x 128px blocks, HW % 32 == 0
    g("c12.k1", 12, 4, 4, 40, 4, 8, opts=OFF, build=0, k_tiles=1, last_k_channels=4, last_k_overlap=0, co_tiles=1, last_co_rows=40,
      px_tiles=1, last_px_count=128, tile_spans_images=1, grid_x=1, grid_y=1),
    g("c12.k1.aff", 12, 2, 4, 40, 8, 8, opts=AFF, build=1, k_tiles=1, last_k_channels=4, px_tiles=1, last_px_count=128, tile_spans_images=1),
    g("c12.k2.aff", 12, 3, 52, 136, 8, 8, opts=AFF, stats="own", build=1, k_tiles=2, last_k_channels=20, co_tiles=2, last_co_rows=8,
      px_tiles=2, last_px_count=64, tile_spans_images=1, stats_own=1, grid_y=2),
    g("c12.k3.res", 12, 2, 68, 128, 8, 12, opts=RES + ("bias",), build=0, k_tiles=3, last_k_channels=4, co_tiles=1, last_co_rows=128,
      px_tiles=2, last_px_count=64, tile_spans_images=1, residual=1),
    g("c12.k3.aff", 12, 2, 96, 40, 8, 8, opts=AFF, build=1, k_tiles=3, last_k_channels=32, px_tiles=1, last_px_count=128),
    g("c12.k5.aff", 12, 2, 160, 40, 8, 16, opts=AFF, stats="atomic", build=1, k_tiles=5, last_k_channels=32, px_tiles=2, stats_own=0,
      tile_spans_images=0),
    g("c12.k7", 12, 1, 224, 40, 4, 8, opts=("bias",), build=0, k_tiles=7, last_k_channels=32, px_tiles=1, last_px_count=32),
    g("c12.g2", 12, 2, 36, 40, 4, 8, G=2, opts=AFF, stats="atomic", build=1, k_tiles=2, last_k_channels=4, px_tiles=1, last_px_count=64,
      stats_own=1, grid_y=2),                                                                   # (one pixel tile owns the one copy)
    g("c12.g2.shared", 12, 2, 36, 136, 4, 8, G=2, shared=True, opts=("bias", "lrelu"), build=0, co_tiles=2, last_co_rows=8, grid_y=4),
    g("c12.tf", 12, 2, 40, 20, 4, 8, opts=OFF + ("transposed",), build=0, k_tiles=2, last_k_channels=8, last_co_rows=20),
    # -- configs 14 (128co) / 15 (64co): 16-channel k-tiles on a three-slot ring, a ragged last one moved back to end at Cin
    g("g14.k1.c40", 14, 32, 16, 40, 2, 2, opts=OFF, build=0, k_tiles=1, last_k_overlap=0, last_k_channels=16, co_tiles=1, last_co_rows=40,
      passes=2, last_pass_rows=0, px_tiles=1, last_px_count=128, tile_spans_images=1, grid_x=1, grid_y=1),
    g("g14.k2.c72.res", 14, 3, 28, 72, 5, 8, opts=RES + ("bias",), build=0, k_tiles=2, last_k_overlap=4, last_k_channels=12,
      last_co_rows=72, last_pass_rows=8, px_tiles=1, last_px_count=120, tile_spans_images=1, residual=1),
    g("g14.k3.c128.aff", 14, 2, 36, 128, 12, 16, opts=AFF, stats="own", build=1, k_tiles=3, last_k_overlap=12, last_k_channels=4,
      last_co_rows=128, last_pass_rows=64, px_tiles=3, last_px_count=128, tile_spans_images=1, stats_own=1, grid_x=3),
    g("g14.k3.c40", 14, 3, 48, 40, 4, 8, opts=("bias", "lrelu"), build=0, k_tiles=3, last_k_overlap=0, last_k_channels=16, px_tiles=1,
      last_px_count=96, last_pass_rows=0),
    g("g14.k4.c136", 14, 5, 52, 136, 12, 12, opts=("bias", "lrelu"), stats="atomic", build=0, k_tiles=4, last_k_overlap=12, co_tiles=2,
      last_co_rows=8, last_pass_rows=0, px_tiles=6, last_px_count=80, stats_own=0, grid_x=12),
    g("g14.k7.aff", 14, 2, 100, 40, 10, 8, opts=AFF, stats="own", build=1, k_tiles=7, last_k_overlap=12, px_tiles=2, last_px_count=32,
      stats_own=1, grid_x=2),
    g("g14.g3", 14, 1, 16, 136, 4, 4, G=3, opts=("bias",), build=0, co_tiles=2, last_co_rows=8, px_tiles=1, last_px_count=16, grid_x=6),
    g("g14.tf", 14, 2, 20, 40, 4, 8, opts=OFF + ("transposed",), build=0, k_tiles=2, last_k_overlap=12, last_k_channels=4),
    g("g14.half.odd.bias", 14, 3, 28, 72, 5, 8, opts=("accum_half", "bias"), build=0, accum_half=1, tile_spans_images=1, last_px_count=120,
      last_pass_rows=8),
    g("g15.k7.c8", 15, 1, 112, 8, 2, 2, opts=OFF, build=0, k_tiles=7, last_k_overlap=0, last_k_channels=16, co_tiles=1, last_co_rows=8,
      passes=1, last_pass_rows=8, px_tiles=1, last_px_count=4),
    g("g15.k4.c64.aff", 15, 2, 64, 64, 16, 8, opts=AFF, stats="atomic", build=1, k_tiles=4, last_k_overlap=0, last_co_rows=64, px_tiles=2,
      last_px_count=128, tile_spans_images=0, stats_own=0),
    g("g15.k2.c8.aff", 15, 2, 28, 8, 6, 8, opts=AFF, stats="atomic", build=1, k_tiles=2, last_k_overlap=4, last_co_rows=8, px_tiles=1,
      last_px_count=96, stats_own=1),                                                            # (one pixel tile owns the one copy)
    g("g15.k2.c72.res", 15, 9, 28, 72, 8, 16, opts=("residual", "lrelu"), build=0, k_tiles=2, last_k_overlap=4, co_tiles=2, last_co_rows=8,
      px_tiles=9, grid_x=18, residual=1),
    g("g15.g3.aff", 15, 5, 16, 72, 4, 8, G=3, opts=AFF, stats="atomic", build=1, co_tiles=2, last_co_rows=8, px_tiles=2, last_px_count=32,
      stats_own=0, grid_x=12),
    g("g15.shared.aff", 15, 2, 36, 64, 4, 4, G=2, shared=True, opts=AFF, build=1, k_tiles=3, last_k_overlap=12, grid_x=2),
    g("g15.tf", 15, 2, 20, 40, 4, 8, opts=OFF + ("transposed",), build=0, k_tiles=2, last_k_overlap=12),
    g("g15.hw4.res", 15, 33, 16, 64, 2, 2, opts=("residual", "bias"), build=0, px_tiles=2, last_px_count=4, tile_spans_images=1, residual=1),
    g("g15.half.even", 15, 2, 16, 64, 8, 16, opts=OFF + ("accum_half",), build=0, accum_half=1, tile_spans_images=0, last_px_count=128),
    g("g15.half.odd", 15, 1, 16, 8, 7, 4, opts=("accum_half", "accum", "lrelu"), build=0, accum_half=1, last_px_count=28),
    # -- the stem, config 16: 16 x 32 output tiles of one image, all 64 channels of a group per workgroup
    stem("stem.tiny", 2, 9, 7, build=0, tiles_x=1, tiles_y=1, last_tile_cols=4, last_tile_rows=5, px_tiles=2, grid_x=2, grid_y=1),
    stem("stem.odd.stats", 2, 33, 63, stats="own", build=1, tiles_x=1, tiles_y=2, last_tile_cols=32, last_tile_rows=1, px_tiles=4, stats_own=1),
    stem("stem.odd.stats.atomic", 2, 33, 63, stats="atomic", like="stem.odd.stats", build=1, stats_own=0),
    stem("stem.partx", 1, 50, 72, build=0, tiles_x=2, tiles_y=2, last_tile_cols=4, last_tile_rows=9),
    stem("stem.partx.g2.epi", 2, 50, 72, G=2, opts=("bias", "lrelu"), build=2, tiles_x=2, tiles_y=2, px_tiles=8, grid_y=2),
    stem("stem.partx.g3.bias", 1, 50, 72, G=3, shared=True, opts=("bias",), build=2, grid_y=3),
    stem("stem.partx.lrelu", 1, 50, 72, opts=("lrelu",), build=2, grid_y=1),
    stem("stem.interior", 1, 95, 191, stats="own", build=1, tiles_x=3, tiles_y=3, last_tile_cols=32, last_tile_rows=16, px_tiles=9, stats_own=1),
]
for _c in CASES:
    assert _c["name"] not in D.BY_NAME
    D.BY_NAME[_c["name"]] = _c
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# one shape that configs 12, 14, 15 and a tap config (8) all host, with the same operands
CROSS_FORM = [D.case(f"cross.c{cfg}", GEMM if cfg >= 12 else "1x1", 1, 1, 3, 52, 72, 8, 8, cfg, opts=("bias", "lrelu"), like="cross.c12")
              for cfg in (12, 14, 15, 8)]
for _c in CROSS_FORM:
    D.BY_NAME[_c["name"]] = _c


# ---- the descriptor, for the query without a device ----------------------------------------------------------------------------------
def flags_of(c, L):
    return D.flags_of(c, L) | (L.EPI_ACCUM_HALF if "accum_half" in c["opts"] else 0)


def dummy_desc(c, L, off=()):
    """The case's ``spk_conv2d_desc`` with made-up pointers (``spk_conv2d_gemm_form`` reads no memory); ``off``: of x / w / out /
    residual / in_scale / in_shift / half, the tensors that start 4 bytes off a 16-byte boundary."""
    o = c["opts"]
    H, W = D.out_hw(c)
    nxt = iter(range(0x100000, 0x10000000, 0x1000))
    ptr = lambda on=True, name=None: (next(nxt) + (4 if name in off else 0)) if on else None
    out_scale, _, slope, gain = D.scalars(c)
    return L.Conv2dDesc(
        x=ptr(True, "x"), w_packed=ptr(True, "w"), bias=ptr("bias" in o), in_scale=ptr("affine" in o, "in_scale"), in_shift=ptr("affine" in o, "in_shift"),
        stats=ptr(bool(c["stats"])), y=ptr(True, "out"), B=c["B"], Cin=c["Cin"], Cout=c["Cout"], H=H, W=W, Hin=c["Hs"], Win=c["Ws"],
        kh=c["k"], kw=c["k"], stride=c["stride"], flags=flags_of(c, L), lrelu_slope=slope if slope is not None else 1.0, out_scale=out_scale,
        config=c["config"], ksplit=0, act_gain=gain, groups=c["G"], group_in_stride=0 if (c["shared"] or c["G"] == 1) else c["Cin"],
        stats_slots=0 if c["stats"] != "own" else 65536, accum_half=ptr("accum_half" in o, "half"), residual=ptr("residual" in o, "residual"))


def query(c, L, desc=None, off=()):
    form = L.GemmForm()
    L.check(L.lib().spk_conv2d_gemm_form(desc if desc is not None else dummy_desc(c, L, off), form), "spk_conv2d_gemm_form")
    return {n: getattr(form, n) for n, _ in L.GemmForm._fields_ if n != "reserved"}


def branches(c, f):
    """The names of what a case covers, from the form ``f`` the library answered for it and the case's operands."""
    o, cfg = c["opts"], f["config"]
    H, W = D.out_hw(c)
    out = set()
    add = lambda *names: out.update(f"{fam}.{n}" for n in names)
    if cfg == 16:
        fam = "stem"
        add("build." + ("plain", "stats", "epi")[f["build"]])
        if f["build"] == 1:
            add("stats." + ("own" if f["stats_own"] else "atomic"))
        if f["build"] == 2:
            add("epi." + "+".join(n for n in ("bias", "lrelu") if n in o))
        add(f"in.{c['Hs']}x{c['Ws']}")
        if c["Hs"] % 2 and c["Ws"] % 2:
            add("odd input")
        if f["tiles_x"] >= 3 and f["tiles_y"] >= 3:
            add("interior tile")
        if f["tiles_x"] == f["tiles_y"] == 1 and f["last_px_count"] * 8 <= 16 * 32:
            add("mostly empty tile")
        if f["tiles_y"] == 2 and f["last_tile_rows"] == 1:
            add("second tile row nearly empty")
        if f["tiles_x"] >= 2 and f["last_tile_cols"] < 32:
            add("partial tile in x")
        if c["G"] > 1:
            add(f"G{c['G']}." + ("shared" if c["shared"] else "own"))
            if c["B"] > 1:
                add("grouped with B > 1")
        return out
    fam = str(cfg) if cfg == 12 else "g2"
    build = ("plain", "affine")[f["build"]]
    kt = f["k_tiles"]
    if cfg == 12:
        add(f"{build}.kt{kt if kt <= 3 else ('odd>=5' if kt % 2 else 'even>=4')}")
        if f["last_k_channels"] < 32 and kt > 1:
            add(f"ragged k {f['last_k_channels']}")
        add("co." + ("whole" if f["last_co_rows"] == 128 else ("one ragged" if f["co_tiles"] == 1 else "two, second ragged")))
        add(f"hw{H * W}")
        if c["G"] == 2:
            add("G2." + ("shared" if c["shared"] else "own"))
        epi = "residual+lrelu+accum" if {"residual", "lrelu", "accum"} <= o else ("off" if "unit_scale" in o and not (o - {"unit_scale", "transposed"}) else
                                                                                  ("bias+out_scale" if "bias" in o else None))
        if epi:
            add("epi." + epi)
    else:
        fam = "g2"
        add(f"{cfg}.{build}", f"{build}.kt{kt}", f"{cfg}.cout{c['Cout']}")
        if f["last_k_overlap"]:
            add(f"overlap{f['last_k_overlap']}")
        if cfg == 14 and f["last_pass_rows"] < 64:
            add("second pass " + ("empty" if f["last_pass_rows"] == 0 else f"{f['last_pass_rows']} rows"))
        add("px." + ("full" if f["last_px_count"] == 128 else "masked"))
        if H * W == 4:
            add("hw4")
        if (H, W) == (5, 8):
            add("hw40")
        n = f["grid_x"]
        add("grid<8" if n < 8 else ("grid%8==0" if n % 8 == 0 else ("grid 9..16" if n <= 16 else "grid>=17")), f"grid{n}")
        if f["accum_half"]:
            add("half." + ("odd H" if H % 2 else "even H"))
            if f["tile_spans_images"]:
                add("half.spans images")
            if "bias" in o:
                add("half.bias")
        if f["residual"]:
            add("residual")
            if cfg == 14 and f["last_co_rows"] > 64:
                add("residual over two passes")
        if c["G"] == 3 and f["co_tiles"] == 2 and f["last_co_rows"] < (128 if cfg == 14 else 64):
            add("G3 ragged second co tile")
        if c["shared"]:
            add("shared input")
        if "transposed" in o and f["last_k_overlap"]:
            add(f"{cfg}.transposed ragged k")
    if "transposed" in o:
        add("transposed")
    if c["stats"]:
        add("stats." + ("own" if f["stats_own"] else "atomic") + ("" if f["last_px_count"] == 128 or cfg == 12 else ".partial"))
    if f["last_px_count"] < 128:
        add("partial px tile")
    if f["tile_spans_images"]:
        add("tile spans images")
    return out


# ---- the documented layouts of the packed weights, restated --------------------------------------------------------------------------
def pack_expected(w, config, tf):
    """The packed image of ``w`` ([Cout, Cin, k, k], a float32 numpy array) as include/spk.h and the kernels' headers document it."""
    if config == 16:                                     # [148][64]: row k = (ci, ky, kx) flattened, row 147 zero
        img = np.zeros((148, 64), np.float32)
        img[:147] = w.reshape(64, 147).T
        return img.reshape(-1)
    m = w[:, :, 0, 0]
    op = m.T if tf else m                                # [operator Cout][operator Cin]
    if config == 12:                                     # the operator itself, row-major
        return np.ascontiguousarray(op).reshape(-1)
    co_t = 128 if config == 14 else 64
    Co, Ci = op.shape
    n_co, n_kt = -(-Co // co_t), -(-Ci // 16)
    img = np.zeros((n_co, n_kt, 16, co_t), np.float32)   # [co tile][k tile][16][CO_T]
    for kt in range(n_kt):
        k0 = min(16 * kt, Ci - 16)                       # a ragged last tile moves back to end at Cin ...
        for k in range(16):
            ci = k0 + k
            if ci < 16 * kt:                             # ... and what the previous tile has stays zero
                continue
            for cot in range(n_co):
                rows = op[cot * co_t:(cot + 1) * co_t, ci]
                img[cot, kt, k, :len(rows)] = rows
    return img.reshape(-1)


PACK_SHAPES = [(cfg, Cout, Cin, tf) for cfg in (12, 14, 15) for tf in (0, 1)
               for Cout, Cin in ((40, 28), (136, 36), (20, 52), (72, 100), (64, 16))]     # [Cout, Cin, 1, 1] of the weight
