"""Inference entry point against the hand-assembled composition, alternating in one process.

(a) ``m.eval(); Gd(cat(Ei(id).expand, Ee(v), Ep(v)))`` chunk by chunk under ``no_grad``: the trunks on the eager eval path
    (``encoder.GroupedTrunks._run``: a launch + ``bn_finalize`` per conv, ``bn_add_relu`` per block), the decoder on its plan;
(b) ``m.reenact``: the trunks on their BatchNorm-folded launch plans (``plan.EncoderPlan``), the same decoder plan.
T = 64 frames of 256^2 in chunks of 8, recipe weights, device-synchronised, after warm-up.  Reports frames/s of both, the time
of the encoders alone in each, and the spread over the repeats.

    python tools/bench_reenact.py [--frames 64] [--chunk 8] [--repeats 7] [--out profiles/reenact_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["eager", "reenact"], default=None, help="one path only, once (for a kernel trace)")
    args = ap.parse_args()
    import model
    from oracle import irfd_ref as IR
    from oracle.weights_recipe import fill_state_dict, recipe_input

    dev = torch.device("cuda:0")
    m = model.IRFD()
    sd = IR.irfd_recipe_state_dict()
    sd.update({"Gd." + k: v for k, v in fill_state_dict(m.Gd.state_dict(), prefix="Gd.").items()})
    m.load_state_dict(sd, strict=False)
    m.to(dev).eval()
    T, chunk = args.frames, args.chunk
    ident = recipe_input("bench.id", (1, 3, 256, 256), "uniform").to(dev)
    video = recipe_input("bench.video", (T, 3, 256, 256), "uniform").to(dev)

    def eager_encoders():
        fi = m.Ei(ident)
        return fi, [(m.Ee(video[t:t + chunk]), m.Ep(video[t:t + chunk])) for t in range(0, T, chunk)]

    def eager():
        fi = m.Ei(ident)
        out = []
        for t in range(0, T, chunk):
            v = video[t:t + chunk]
            fe, fp = m.Ee(v), m.Ep(v)
            out.append(m.Gd(m._prepare_generator_input(fi.expand(v.size(0), -1, -1, -1), fe, fp)))
        return torch.cat(out, 0)

    def plan_encoders():
        fi = m.encode(ident, "Ei")
        return fi, [(m.encode(video[t:t + chunk], "Ee"), m.encode(video[t:t + chunk], "Ep")) for t in range(0, T, chunk)]

    def reenact():
        return m.reenact(ident, video, chunk=chunk)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    with torch.no_grad():
        if args.only:
            fn = eager if args.only == "eager" else reenact
            for _ in range(args.warmup):
                fn()
            print(f"{args.only}: {timed(fn) * 1e3:.2f} ms for {T} frames")
            return
        names = ("eager", "reenact", "eager_encoders", "plan_encoders")
        fns = dict(zip(names, (eager, reenact, eager_encoders, plan_encoders)))
        for _ in range(args.warmup):
            for n in names:
                fns[n]()
        times = {n: [] for n in names}
        for _ in range(args.repeats):                       # alternating: drift hits every path alike
            for n in names:
                times[n].append(timed(fns[n]))
    lines = [f"bench_reenact: {torch.cuda.get_device_name(0)}, T={T} frames of 256^2, chunk={chunk}, {args.repeats} alternating repeats "
             f"after {args.warmup} warm-up rounds, recipe weights, fp32"]
    for n in names:
        ts = sorted(times[n])
        med = statistics.median(ts)
        lines.append(f"{n:15s} median {med * 1e3:8.2f} ms  min {ts[0] * 1e3:8.2f}  max {ts[-1] * 1e3:8.2f}  "
                     f"spread {(ts[-1] - ts[0]) / med * 100:5.1f} %  -> {T / med:8.1f} frames/s")
    me, mr = statistics.median(times["eager"]), statistics.median(times["reenact"])
    ee, pe = statistics.median(times["eager_encoders"]), statistics.median(times["plan_encoders"])
    lines.append(f"encoder share: eager {ee / me * 100:.1f} % of {me * 1e3:.2f} ms, reenact {pe / mr * 100:.1f} % of {mr * 1e3:.2f} ms; "
                 f"reenact / eager = {mr / me:.3f} (encoders alone {pe / ee:.3f})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
