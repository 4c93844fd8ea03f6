"""Every host-side decision of the weight gradient for one build of the library, one line per descriptor of a fixed, seeded sweep --
no GPU.  Two builds that print the same lines launch the same kernels on the same grids with the same workspace checks.

    python tools/dump_wgrad_decisions.py [--lib path/to/libspk_hip.so] > new.txt
    python tools/dump_wgrad_decisions.py --compare old.txt new.txt

The sweep: every case and refusal of tests/wgrad_cases.py; a few thousand descriptors drawn over k in {1, 3, 4, 7}, stride, B up to
32, ragged and whole channel counts, planes from 1 x 1 to 128 wide, every mode and ``up`` flavour, groups / shared / fold, splits in
{0, 1, 2, 7}, each misalignment subset and the Winograd flag; descriptors with a missing or short workspace; and
spk_wgrad_reduce_form over slab counts, channel counts, taps, fold and alignments.  A line holds the return code, spk_last_error()
when refused, every field of spk_wgrad_form and the answer of spk_conv2d_wgrad_workspace_bytes.

--compare holds two dumps to the rule of a refactor: return codes, error texts, form fields and reducer answers identical; the
workspace answer never below the form's workspace_bytes and never above the old answer."""
import argparse
import importlib
import itertools
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CHANNELS = (3, 4, 5, 8, 20, 24, 40, 64, 70, 72, 96, 128, 130, 160, 256)
MISALIGN = [s for r in range(4) for s in itertools.combinations(("g", "x", "dw"), r)]


def sweep(Wc):
    for c in Wc.CASES:
        yield c
    for c, _ in Wc.REFUSALS:
        yield c
    rnd = random.Random(20260501)
    for i in range(4000):
        wild = rnd.random() < 0.15          # any combination, mostly refused; else one the library has a form for, mostly
        k = rnd.choice((1, 3, 3, 3, 4, 7))
        stride = 2 if k in (4, 7) and not wild else rnd.choice((1, 2))
        s1_3x3 = k == 3 and stride == 1
        G = rnd.choice((1, 1, 1, 2, 3, 4))
        mode = rnd.choice(("plain", "plain", "affine", "bscale"))
        if mode == "bscale" and not wild and not (s1_3x3 and G == 1):
            mode = "plain"
        if mode == "affine" and k == 4 and not wild:
            mode = "plain"
        up = rnd.choice((None, None, None, "bilinear", "fir"))
        if not wild and (not s1_3x3 or mode == "affine" or (up == "fir") != (mode == "bscale")):
            up = None
        fold = rnd.choice((1, 1, 2))
        if not wild and G % fold:
            fold = 1
        Ws = rnd.choice((1, 2, 3, 4, 5, 6, 8, 9, 12, 13, 16, 20, 24, 32, 36, 40, 64, 72, 128))
        Hs = rnd.choice((1, 2, 3, 4, 5, 6, 8, 9, 12, 16, 18, 32, 64))
        Cin = 3 if k == 7 and rnd.random() < 0.8 else rnd.choice(CHANNELS)
        Cout = rnd.choice((64, 128, 256)) if G > 1 and not wild else rnd.choice(CHANNELS)
        misalign, wino = rnd.choice(MISALIGN), rnd.random() < 0.08
        if not wild and rnd.random() < 0.5:          # the shapes the aligned, whole-block forms ask for (wide, s2, GEMM, LDS-DMA, Winograd)
            Ws, Hs, Cin = rnd.choice((8, 12, 16, 32, 64)), rnd.choice((4, 8, 16, 32)), Cin if k == 7 else rnd.choice((64, 128, 256))
            Cout, misalign = rnd.choice((64, 128, 256)), rnd.choice(((), (), ("dw",)))
        if wino and not wild and (not s1_3x3 or up):
            wino = False
        yield Wc.case(f"sweep{i}", k, stride, rnd.choice((1, 2, 3, 5, 8, 16, 32)), Cin, Cout, Hs, Ws, mode, up=up, G=G, shared=rnd.random() < 0.3,
                      fold=fold, splits=rnd.choice((0, 1, 2, 7)), misalign=misalign, wino=wino, kernel="-")


def form_line(L, d):
    form = L.WgradForm()
    rc = L.lib().spk_conv2d_wgrad_launch_form(d, form)
    err = L.lib().spk_last_error().decode() if rc else ""
    return rc, form, f"rc={rc} err={err!r} " + " ".join(f"{n}={getattr(form, n)}" for n, _ in L.WgradForm._fields_)


def dump(L, Wc, out):
    for c in sweep(Wc):
        d = Wc.dummy_desc(c, L)
        rc, form, text = form_line(L, d)
        tag = " ".join(f"{k}={sorted(v) if isinstance(v, frozenset) else v}" for k, v in c.items() if k not in ("name", "declares"))
        out.write(f"desc {c['name']} [{tag}] | {text} | ws_query={Wc.workspace_bytes(c, L)}\n")
        if rc == 0:                 # the workspace check: one byte short, and no workspace at all
            d.workspace_bytes = form.workspace_bytes - 1
            out.write(f"short {c['name']} | {form_line(L, d)[2]}\n")
            d.workspace = None
            out.write(f"nows {c['name']} | {form_line(L, d)[2]}\n")
    for n_slabs, Cout, Cin, taps, fold, off_s, off_d in itertools.product((0, 1, 3, 4, 8, 31, 32, 33, 133), (8, 64, 72, 512), (3, 4, 64, 70, 147, 512),
                                                                        (1, 9, 16, 49), (0, 1, 2, 3), (0, 4), (0, 4)):
        form = L.WgradForm()
        rc = L.lib().spk_wgrad_reduce_form(0x100000 + off_s, 0x200000 + off_d, n_slabs, Cout, Cin, taps, fold, form)
        err = L.lib().spk_last_error().decode() if rc else ""
        out.write(f"reduce n_slabs={n_slabs} Cout={Cout} Cin={Cin} taps={taps} fold={fold} off={off_s},{off_d} | rc={rc} err={err!r} "
                  f"reducer={form.reducer} fold={form.fold} taps={form.taps} n_slabs={form.n_slabs}\n")


def compare(old_path, new_path):
    old, new = open(old_path).read().splitlines(), open(new_path).read().splitlines()
    assert len(old) == len(new), (len(old), len(new))
    counts = dict(desc=0, refused=0, short=0, nows=0, reduce=0, ws_equal=0, ws_tighter=0)
    for a, b in zip(old, new):
        kind = a.split()[0]
        counts[kind] += 1
        if kind != "desc":
            assert a == b, (a, b)
            continue
        (head_a, form_a, ws_a), (head_b, form_b, ws_b) = a.split(" | "), b.split(" | ")
        assert head_a == head_b and form_a == form_b, (a, b)
        ws_a, ws_b = int(ws_a.split("=")[1]), int(ws_b.split("=")[1])
        need = int(form_b.split("workspace_bytes=")[1])
        assert ws_b <= ws_a, ("the workspace query grew", a, b)
        if form_b.startswith("rc=0 "):
            assert ws_b >= need > 0, ("the workspace query is below the launcher's check", b)
        else:
            counts["refused"] += 1
        counts["ws_equal" if ws_a == ws_b else "ws_tighter"] += 1
    print(" ".join(f"{k}={v}" for k, v in counts.items()))


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
        import wgrad_cases
        dump(L, wgrad_cases, sys.stdout)
