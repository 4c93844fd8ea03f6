"""A digest of every weight gradient the four pipelined 3x3 kernels compute for one build of the tree, on the GPU: every case of
tests/wgrad_cases.py whose declared kernel is pipe, wide16, wide8, up, s2_16 or s2_8, with the case's seeded inputs, launched as
tests/test_wgrad_branches_gpu.py launches it (``ops.wgrad_desc`` + ``spk_conv2d_wgrad``, the declared tensors 4 bytes off a 16-byte
boundary).  One line per case: name, the form ``spk_conv2d_wgrad_launch_form`` answers for the launched descriptor, SHA-256 of the
dw bytes.  Two builds whose files are equal compute the same bits on every case; SPK_LAB_LIB selects another build of the library.

    python tools/dump_wgrad_outputs.py --out new.txt
    python tools/dump_wgrad_outputs.py --compare old.txt new.txt
"""
import argparse
import ctypes as C
import hashlib
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

KERNELS = ("pipe", "wide16", "wide8", "up", "s2_16", "s2_8")
# as tests/conftest.py: the case table declares the upsample-folded form for every shape it can take (the library reads this once)
os.environ.setdefault("SPK_WGRAD_UP_MIN_W", "16")


def placed(t, dev, off):
    """``t`` on the device, 16-byte aligned or 4 bytes off."""
    buf = torch.zeros(t.numel() + 8, device=dev)
    v = buf[1 if off else 0:][:t.numel()]
    assert v.data_ptr() % 16 == (4 if off else 0)
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


def dump_case(pkg, dev, Wc, c):
    ops, L = pkg.ops, pkg._lib
    t = Wc.inputs(c)
    g, x = placed(t["g"], dev, "g" in c["misalign"]), placed(t["x"], dev, "x" in c["misalign"])
    on = {k: t[k].to(dev) for k in ("a", "b", "s", "d") if k in t}
    shape = Wc.dw_shape(c)
    dw = placed(t["base"] if c["accumulate"] else torch.full(shape, float("nan")), dev, "dw" in c["misalign"])
    ws = torch.full((Wc.workspace_bytes(c, L) // 4,), float("nan"), device=dev)
    d, _ = ops.wgrad_desc(g, x, c["Cout"], c["Cin"], c["k"], c["stride"], upsample=bool(c["up"]), up_fir=c["up"] == "fir",
                          in_affine=(on["a"], on["b"]) if c["mode"] == "affine" else None, batch_scale=on.get("s"), g_scale=on.get("d"),
                          scale=c["scale"], out=dw, accumulate=c["accumulate"], splits=c["splits"], groups=c["G"],
                          shared_input=c["shared"], fold=c["fold"], workspace=ws)
    form = Wc.query(c, L, d)
    assert form["kernel"] == c["declares"]["kernel"], (c["name"], form["kernel"])
    L.check(L.lib().spk_conv2d_wgrad(C.byref(d), L.stream_ptr()), "spk_conv2d_wgrad")
    torch.cuda.synchronize()
    digest = hashlib.sha256(dw.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
    return f"{c['name']} {form['kernel']}.{form['mode']}.{form['TW']}x{form['TH']}.splits{form['splits']}.{form['reducer']} {digest}"


def compare(old_path, new_path):
    old, new = (open(p).read().splitlines() for p in (old_path, new_path))
    differ = [f"- {a}\n+ {b}" for a, b in zip(old, new) if a != b]
    print(f"{len(old)} / {len(new)} cases: {len(differ)} differ")
    if differ or len(old) != len(new):
        sys.exit("\n".join(differ) or "the files list different cases")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", metavar="FILE.txt")
    ap.add_argument("--compare", nargs=2, metavar=("OLD", "NEW"))
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare)
    else:
        if not args.out:
            ap.error("--out FILE.txt or --compare OLD NEW")
        if not torch.cuda.is_available():
            sys.exit("tools/dump_wgrad_outputs.py needs a HIP device")
        import wgrad_cases as Wc
        Wc.require_default_dispatch()
        pkg = importlib.import_module("speak-hack_amd")
        if os.environ.get("SPK_LAB_LIB"):          # another build of the library, as tools/bench_wgrad.py
            pkg._lib.LIB_PATH = os.path.abspath(os.environ["SPK_LAB_LIB"])
        pkg._lib.lib()
        dev = torch.device("cuda:0")
        lines = [dump_case(pkg, dev, Wc, c) for c in Wc.CASES if c["declares"]["kernel"] in KERNELS]
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"{args.out}: {len(lines)} cases")
