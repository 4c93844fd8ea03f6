#!/usr/bin/env python3
"""The decoder's noise draw: ``spk_noise_fill`` (csrc/noise.hip, the first op of a seeded ``plan.DecoderPlan``) against the
``normal_()`` of an unseeded plan on the same flat buffer -- the 13 planes of a 256^2 synthesis pass, 174 736 floats a frame --
at B = 8 (1 397 888 floats) and B = 1.  HIP events around ``--iters`` back-to-back calls after warm-up, the two alternating,
``--repeats`` times; the median and the spread of each are printed.  The fill is also run in its fixed-noise form.

    python tools/bench_noise.py [--iters 200] [--repeats 7] [--out profiles/noise_bench.txt]
"""
import argparse
import ctypes
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_time(fn, n, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_noise needs a HIP device: nothing is measured without one")
    pkg = importlib.import_module("speak-hack_amd")
    ops, L = pkg.ops, pkg._lib
    lib = L.lib()
    dev = torch.device("cuda:0")
    lines = [f"bench_noise: {torch.cuda.get_device_name(0)}, {args.iters} calls per timing, {args.repeats} alternating repeats"]
    for B in (8, 1):
        shapes = pkg.SynthesisNetwork(resolution=256).noise_shapes(B)
        hw = [s[2] * s[3] for s in shapes]
        flat = torch.empty(B * sum(hw), device=dev, dtype=torch.float32)
        stream = L.stream_ptr()
        fresh = ops.noise_fill_args(flat.data_ptr(), hw, B, seed=1234)
        fixed = ops.noise_fill_args(flat.data_ptr(), hw, B, seed=1234, fixed=True)

        def fill(a=fresh):
            L.check(lib.spk_noise_fill(ctypes.byref(a), stream), "spk_noise_fill")

        forms = {"spk_noise_fill (fresh)": fill, "spk_noise_fill (fixed)": lambda: fill(fixed), "normal_()": flat.normal_}
        times = {k: [] for k in forms}
        for _ in range(args.repeats):                      # alternating: drift hits all alike
            for k, fn in forms.items():
                times[k].append(device_time(fn, args.iters))
        lines.append(f"B = {B}: {flat.numel()} floats ({flat.numel() * 4 / 1e6:.2f} MB), 13 planes, one launch each")
        for k, ts in times.items():
            ts = sorted(ts)
            med = statistics.median(ts)
            lines.append(f"  {k:24s} median {med * 1e6:7.2f} us  min {ts[0] * 1e6:7.2f}  max {ts[-1] * 1e6:7.2f}  "
                         f"-> {flat.numel() * 4 / med / 1e9:7.1f} GB/s written")
        lines.append(f"  fill / normal_() = {statistics.median(times['spk_noise_fill (fresh)']) / statistics.median(times['normal_()']):.3f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
