"""Every host-side decision of the forward conv family for one build of the library, one line per descriptor of a fixed, seeded
sweep -- no GPU.  Two builds that print the same lines refuse the same descriptors with the same words and launch the same kernels
on the same grids with the same splits, finishers and workspace checks.

    python tools/dump_conv_decisions.py [--lib path/to/libspk_hip.so] > new.txt
    python tools/dump_conv_decisions.py --compare old.txt new.txt

The sweep: every case of tests/direct_conv_cases.py and tests/gemm_conv_cases.py (CASES, CROSS_FORM); a few thousand descriptors
drawn over the kinds (direct, Winograd, DGRAD_S2, TRANSPOSE4X4_S2, bf16x3), k in {1, 2, 3, 4, 7} and stride, config in {-1, 0..16},
ksplit in {0, 1, 2, 7}, B up to 32, ragged and whole channel counts, planes from 1 x 1 to 256 wide, groups with a shared or a
strided input, the input-stage flags, subsets of the epilogue flags, y_pre, stats with 0 / 1 / exactly enough / more slots, residual,
accum_half, out_scale_dev, out_scale_bc, SPK_EPI_TORGB and each misalignment subset of the pointers; a fixed share of wild
combinations that are mostly refused.  A line holds the return code and spk_last_error() of spk_conv2d_launch_form and of
spk_conv2d_gemm_form, every field of both forms, and the answers of spk_conv2d_pick_config, spk_conv2d_workspace_bytes_grouped,
spk_conv2d_wino_workspace_bytes, spk_conv2d_dgrad_s2_workspace_bytes and spk_conv2d_stats_slots for the same shape.  Every accepted
sliced descriptor is asked again with its workspace one byte short and with none.  The dump ends with the forms it reached, and fails
if a key of REQUIRED (tests/test_direct_conv_forms_cpu.py) or a GEMM / stem build is not among them.

--compare demands identical lines and prints the counts: descriptors accepted and refused per family, short and no-workspace lines."""
import argparse
import collections
import importlib
import itertools
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CHANNELS = (3, 4, 5, 8, 16, 20, 24, 40, 52, 64, 70, 72, 96, 128, 130, 256, 512)
SIDES = (1, 2, 3, 4, 5, 6, 8, 9, 12, 13, 16, 18, 20, 24, 32, 36, 40, 48, 64, 72, 128, 256)
POINTERS = ("x", "w_packed", "y", "y_pre", "noise", "residual", "in_scale", "in_shift", "accum_half", "workspace", "rgb_y")
MODES = ("plain", "x2", "affine", "bscale", "x2_bscale", "plain_stats", "plain_residual")
GEMM_BUILDS = {(12, 0), (12, 1), (14, 0), (14, 1), (15, 0), (15, 1), (16, 0), (16, 1), (16, 2)}


def drawn(L, rnd, i):
    """One descriptor of the sweep: (family label, spk_conv2d_desc)."""
    wild = rnd.random() < 0.12                      # any combination, mostly refused
    kind = rnd.choice(("direct",) * 11 + ("wino",) * 3 + ("dgrad_s2",) * 3 + ("transpose4x4",) * 2 + ("bf16x3",))
    B, G = rnd.choice((1, 2, 3, 5, 8, 16, 32)), rnd.choice((1, 1, 1, 2, 3))
    Cin, Cout, Hs, Ws = rnd.choice(CHANNELS), rnd.choice(CHANNELS), rnd.choice(SIDES[:-2]), rnd.choice(SIDES)
    flags, config, x2 = 0, -1, False
    if kind == "direct":
        k = rnd.choice((1, 1, 1, 3, 3, 3, 3, 7, 4) + ((2,) if wild else ()))
        stride = rnd.choice((1, 2)) if k in (1, 3) or wild else (2 if k in (4, 7) else 1)
        if k == 7 and rnd.random() < 0.7:
            Cin, Cout, Ws = 3, 64, rnd.choice((8, 16, 32, 36, 64, 128))
        valid = {(1, 1): (8, 9, 10, 11, 12, 14, 15), (1, 2): (8, 9, 10, 11), (3, 1): range(8), (3, 2): (4, 5, 6, 7), (7, 2): (4, 5, 6, 7, 16),
                 (4, 2): (4, 5, 6, 7)}.get((k, stride), ())
        config = rnd.choice(range(17)) if wild or not valid else rnd.choice(list(valid) + [-1] * max(2, len(valid) // 2))
        if k == 1 and stride == 1 and config in (-1, 12, 14, 15) and rnd.random() < 0.7:      # shapes the GEMM forms take
            Cin, Cout, Hs, Ws = rnd.choice((16, 20, 64, 128, 256)), rnd.choice((8, 40, 64, 128, 256)), rnd.choice((2, 4, 8, 16)), rnd.choice((2, 4, 8, 16, 32))
        stage = rnd.choice(("plain",) * 4 + ("affine", "affine", "bscale", "x2", "x2", "x2_bscale", "x2_fir"))
        if not wild:
            if (k, stride) != (3, 1) and stage != "affine" or (k in (4, 7) and stage == "affine" and rnd.random() < 0.8):
                stage = "plain"
            if "bscale" in stage and 0 <= config < 4:
                config += 4
        x2 = "x2" in stage
        flags |= (L.CONV_IN_AFFINE_RELU if stage == "affine" else 0) | (L.CONV_IN_BATCH_SCALE if "bscale" in stage else 0)
        flags |= (L.CONV_UPSAMPLE2X if x2 else 0) | (L.CONV_UP_FIR1331 if stage == "x2_fir" else 0)
        p = (k - 1) // 2
        H, W = (2 * Hs, 2 * Ws) if x2 else ((Hs + 2 * p - k) // stride + 1, (Ws + 2 * p - k) // stride + 1)
        if H < 1 or W < 1:
            Hs, Ws = Hs + k, Ws + k
            H, W = (Hs + 2 * p - k) // stride + 1, (Ws + 2 * p - k) // stride + 1
    elif kind in ("wino", "bf16x3"):
        k, stride = 3, 1
        if not wild:
            Cin, Hs, Ws = rnd.choice((16, 32, 64, 128, 256)), rnd.choice((8, 16, 32, 64)), rnd.choice((16, 32, 64, 128))
        x2 = rnd.random() < 0.25
        H, W = (2 * Hs, 2 * Ws) if x2 else (Hs, Ws)
        flags |= (L.CONV_WINOGRAD if kind == "wino" else L.CONV_BF16X3) | (L.CONV_UPSAMPLE2X if x2 else 0)
        flags |= L.CONV_IN_BATCH_SCALE if rnd.random() < 0.2 else 0
        flags |= L.EPI_TORGB if kind == "wino" and rnd.random() < 0.2 else 0
        if not wild and (x2 or flags & (L.CONV_IN_BATCH_SCALE | L.EPI_TORGB) or kind == "bf16x3"):
            G = 1
        if flags & L.EPI_TORGB and not wild:
            Cout = rnd.choice((16, 40, 64))
    elif kind == "dgrad_s2":
        k, stride = 3, 2
        H, W = 2 * Hs - rnd.choice((0, 1)), 2 * Ws - rnd.choice((0, 1))
        flags |= L.CONV_DGRAD_S2
        config = rnd.choice(range(17)) if wild else rnd.choice((-1, -1, 0, 1, 2, 3, 13, 13))
        if not wild and rnd.random() < 0.5:         # few workgroups and a deep contraction: the sliced form of config 13
            B, Cin, Hs, Ws = rnd.choice((1, 2)), rnd.choice((128, 256, 512)), rnd.choice((4, 8, 16)), rnd.choice((12, 16))
            H, W = 2 * Hs, 2 * Ws
    else:
        k, stride, G = 4, 2, 1 if not wild else G
        H, W = 2 * Hs, 2 * Ws
        flags |= L.CONV_TRANSPOSE4X4_S2
        config = rnd.choice(range(17)) if wild else rnd.choice((-1, 0, 1, 2, 3))
    if H < 1 or W < 1:
        H, W = max(H, 1), max(W, 1)
    # epilogue: a subset of the flags the kind takes (any subset when wild)
    plain_epi = kind in ("direct", "wino", "bf16x3") and (G == 1 or kind == "direct")
    takes = {"bias": plain_epi or kind == "transpose4x4", "noise": plain_epi and G == 1, "lrelu": plain_epi, "style": plain_epi and G == 1,
             "accum": kind != "bf16x3"}
    on = {n for n, ok in takes.items() if (ok or wild) and rnd.random() < 0.4}
    for n, bit in (("bias", L.EPI_BIAS), ("noise", L.EPI_NOISE), ("lrelu", L.EPI_LRELU), ("style", L.EPI_STYLE), ("accum", L.EPI_ACCUM)):
        flags |= bit if n in on else 0
    y_pre = (plain_epi and G == 1 or wild) and rnd.random() < 0.15
    stats = (kind == "direct" or wild) and rnd.random() < 0.3
    residual = (kind == "direct" and k == 1 and stride == 1 and not stats and not y_pre and not on & {"noise", "style"} and
                not flags & L.CONV_IN_AFFINE_RELU or wild) and rnd.random() < 0.3
    half = (kind == "direct" and k == 1 and stride == 1 and config in (-1, 14, 15) and not residual or wild) and rnd.random() < 0.12
    flags |= (L.EPI_STATS if stats else 0) | (L.EPI_RESIDUAL if residual else 0) | (L.EPI_ACCUM_HALF if half else 0)
    scale_dev = rnd.random() < 0.1 and (wild or kind != "bf16x3")
    demod = rnd.random() < (0.5 if flags & L.CONV_IN_BATCH_SCALE else (0.1 if wild else 0.0))
    off = {n for n in POINTERS if rnd.random() < 0.07} if rnd.random() < 0.4 else set()
    nxt = iter(range(0x100000, 0x10000000, 0x1000))
    ptr = lambda name, on=True: (next(nxt) + (4 if name in off else 0)) if on else None
    gin = 0 if G == 1 or rnd.random() < 0.35 else Cin + rnd.choice((0, 0, 8))
    ksplit = rnd.choice((0, 0, 1, 2, 7))
    slots = 0
    if stats:
        exact = L.lib().spk_conv2d_stats_slots(config, k, k, stride, B, Cin, Cout, H, W)
        slots = rnd.choice((0, 1, max(exact, 1), max(exact, 1) + 3))
    affine, scaled = bool(flags & L.CONV_IN_AFFINE_RELU), bool(flags & L.CONV_IN_BATCH_SCALE)
    d = L.Conv2dDesc(
        x=ptr("x"), w_packed=ptr("w_packed"), bias=ptr("bias", "bias" in on), noise_w=ptr("noise_w", "noise" in on), noise=ptr("noise", "noise" in on),
        style=ptr("style", "style" in on), in_scale=ptr("in_scale", affine or scaled), in_shift=ptr("in_shift", affine), stats=ptr("stats", stats),
        y=ptr("y"), y_pre=ptr("y_pre", y_pre), B=B, Cin=Cin, Cout=Cout, H=H, W=W, Hin=Hs, Win=Ws, kh=k, kw=k, stride=stride,
        style_stride=2 * G * Cout + 3 if "style" in on else 0, flags=flags, lrelu_slope=rnd.choice((0.2, 0.01, 1.0, 1.5)),
        out_scale=1.0 if k == 7 and rnd.random() < 0.8 else rnd.choice((1.0, 0.37)), config=config, ksplit=ksplit, workspace=ptr("workspace"),
        workspace_bytes=1 << 40, out_scale_bc=ptr("out_scale_bc", demod), act_gain=rnd.choice((0.0, 1.0, 1.4142135)), groups=G,
        group_in_stride=gin, stats_slots=slots, accum_half=ptr("accum_half", half), out_scale_dev=ptr("out_scale_dev", scale_dev),
        rgb_w=ptr("rgb_w", bool(flags & L.EPI_TORGB)), rgb_bias=ptr("rgb_bias", bool(flags & L.EPI_TORGB) and rnd.random() < 0.5),
        rgb_y=ptr("rgb_y", bool(flags & L.EPI_TORGB)), rgb_channels=3 if flags & L.EPI_TORGB else 0, residual=ptr("residual", residual))
    fam = kind if kind != "direct" else {12: "gemm12", 14: "gemm2", 15: "gemm2", 16: "stem"}.get(config, "tap" if config >= 0 else "picked")
    return ("wild." if wild else "") + fam, d


def sweep(L):
    import direct_conv_cases as D
    import gemm_conv_cases as Gc
    for c in D.CASES:
        yield c["name"], "table." + c["family"], D.dummy_desc(c, L)
    for c in list(Gc.CASES) + list(Gc.CROSS_FORM):
        yield c["name"], "table." + str(c["family"]), Gc.dummy_desc(c, L)
    rnd = random.Random(20261020)
    for i in range(6000):
        fam, d = drawn(L, rnd, i)
        yield f"sweep{i}", fam, d


def ask(L, d):
    lib = L.lib()
    cf, gf = L.Conv2dForm(), L.GemmForm()
    rc_c = lib.spk_conv2d_launch_form(d, cf)
    err_c = lib.spk_last_error().decode() if rc_c else ""
    rc_g = lib.spk_conv2d_gemm_form(d, gf)
    err_g = lib.spk_last_error().decode() if rc_g else ""
    text = (f"launch_form rc={rc_c} err={err_c!r} " + " ".join(f"{n}={getattr(cf, n)}" for n, _ in L.Conv2dForm._fields_) +
            f" | gemm_form rc={rc_g} err={err_g!r} " + " ".join(f"{n}={getattr(gf, n)}" for n, _ in L.GemmForm._fields_))
    return rc_c, cf, rc_g, gf, text


def reached_key(L, d, cf):
    """The coverage key of tests/direct_conv_cases.py for an accepted launch form."""
    fin = ("none", "scalar", "vec")[cf.finisher]
    if d.flags & L.CONV_WINOGRAD:
        return ("wino", "-", "-", "-", fin)
    if cf.config == 13:
        return ("dgrad13", "-", "-", "-", fin)
    family = ("dgrad_s2" if d.flags & L.CONV_DGRAD_S2 else "transpose4x4" if d.flags & L.CONV_TRANSPOSE4X4_S2 else
              "1x1" if d.kh == 1 else f"{d.kh}x{d.kh}s{d.stride}" + (("a" if cf.config <= 3 else "b") if (d.kh, d.stride) == (3, 1) else ""))
    return (family, MODES[cf.mode], "fg" if cf.fixed_geometry else "generic", "raw" if cf.ksplit > 1 else ("dword", "staged", "halved")[cf.staged], fin)


def dump(L, out):
    lib = L.lib()
    reached = collections.Counter()
    for name, fam, d in sweep(L):
        rc_c, cf, rc_g, gf, text = ask(L, d)
        G = max(d.groups, 1)
        q = (f"pick={lib.spk_conv2d_pick_config(d.kh, d.kw, d.stride, d.B, d.Cin, d.Cout, d.H, d.W)} "
             f"ws={lib.spk_conv2d_workspace_bytes_grouped(d.config, d.ksplit, d.kh, d.kw, d.stride, d.B, d.Cin, d.Cout, d.H, d.W, G)} "
             f"ws_wino={lib.spk_conv2d_wino_workspace_bytes(d.ksplit, d.B, d.Cin, G * d.Cout, d.H, d.W)} "
             f"ws_dgrad={lib.spk_conv2d_dgrad_s2_workspace_bytes(d.B, d.Cin, d.Cout, d.Hin, d.Win, d.H, d.W, G)} "
             f"slots={lib.spk_conv2d_stats_slots(d.config, d.kh, d.kw, d.stride, d.B, d.Cin, d.Cout, d.H, d.W)}")
        tag = " ".join(f"{n}={getattr(d, n)}" for n, _ in L.Conv2dDesc._fields_ if n != "reserved")
        out.write(f"desc {name} fam={fam} [{tag}] | {text} | {q}\n")
        if rc_c == 0:
            reached[reached_key(L, d, cf)] += 1
        if rc_g == 0:
            reached[("gemm", gf.config, gf.build)] += 1
        if rc_c == 0 and cf.ksplit > 1:            # the workspace check: one byte short, and no workspace at all
            d.workspace_bytes = cf.ksplit * d.B * G * d.Cout * d.H * d.W * 4 - 1
            out.write(f"short {name} fam={fam} | {ask(L, d)[4]}\n")
            d.workspace = None
            out.write(f"nows {name} fam={fam} | {ask(L, d)[4]}\n")
    for key, n in sorted(reached.items(), key=lambda kv: tuple(map(str, kv[0]))):
        out.write(f"reached {' '.join(map(str, key))} x{n}\n")
    from test_direct_conv_forms_cpu import REQUIRED
    missing = sorted(REQUIRED - set(reached)) + sorted(("gemm",) + b for b in GEMM_BUILDS if ("gemm",) + b not in reached)
    switched = [e for e in ("SPK_CONV_FG", "SPK_CONV_STAGED_EPI") if os.environ.get(e) == "0"]      # (these take forms away)
    if missing and not switched:
        sys.exit(f"the sweep does not reach: {missing}")


def compare(old_path, new_path):
    old, new = open(old_path).read().splitlines(), open(new_path).read().splitlines()
    assert len(old) == len(new), (len(old), len(new))
    counts = collections.Counter()
    for a, b in zip(old, new):
        assert a == b, (a, b)
        kind = a.split()[0]
        if kind == "desc":
            fam = a.split()[2].split("=")[1]
            served = "rc=0" in (a.split(" | ")[1].split()[1], a.split(" | gemm_form ")[1].split()[0])
            counts[f"{fam}:{'accepted' if served else 'refused'}"] += 1
        counts[kind] += 1
    print(" ".join(f"{k}={v}" for k, v in sorted(counts.items())))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="another build of libspk_hip.so (default: the tree's)")
    ap.add_argument("--compare", nargs=2, metavar=("OLD", "NEW"))
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare)
    else:
        L = importlib.import_module("speak-hack_amd")._lib
        if args.lib:
            L.LIB_PATH = os.path.abspath(args.lib)
        dump(L, sys.stdout)
