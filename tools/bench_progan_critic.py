#!/usr/bin/env python3
"""Time the ProGAN critic (stylegan.Discriminator(512), img_channels 3) on the HIP path at batch 8: ms per forward without
grad, per forward + backward (d/dx and every parameter) and per WGAN-GP penalty step (recorded d/dx, then the penalty's
backward), with algorithmic TFLOP/s from the layer shapes (2 * MAC; x3 for forward + backward).  Also times the 2x2 pool
of the new pool-and-blend kernel against spk_blur2d_fwd with a 2x2 filter of 0.25 at stride 2 on [8,128,256,256].

    python tools/bench_progan_critic.py [--steps 4 6] [--reps 10]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/bench_progan_critic.py --steps 6 --forward-only --reps 20
        then  python tools/bench_progan_critic.py --shares DIR     (each new kernel's share of the kernel time)
"""
import argparse
import csv
import glob
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FACTORS = [1, 1, 1, 1, 1 / 2, 1 / 4, 1 / 8, 1 / 16, 1 / 32]
NEW_KERNELS = ("avgpool2x_blend", "mbstd_")


def critic_gflop(steps, C=512, img=3):
    """Forward GFLOP per image of Discriminator(C) at ``steps`` (2 * MAC of every conv / FC; pools and blends not counted)."""
    n = len(FACTORS) - 1
    cur = n - steps
    r = 4 * 2 ** steps
    cin = lambda i: int(C * FACTORS[n - i])                        # noqa: E731  prog_blocks[i]: cin(i) -> cin(i + 1)
    mac = img * (cin(cur) if steps else C) * r * r                  # fromRGB
    if steps:
        mac += img * cin(cur + 1) * (r // 2) ** 2                   # the downscaled branch's fromRGB
    for i in range(cur, n):
        ci, co = cin(i), (cin(i + 1) if i + 1 < n else C)
        mac += 9 * r * r * (ci * co + co * co)
        r //= 2
    mac += 9 * 16 * (C + 1) * C + 16 * C * C + C                   # final block: 3x3 on 513 channels, 4x4 valid, 1x1 -> 1
    return 2 * mac / 1e9


def ev_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def shares(d):
    """Per-kernel share of the kernel time in a rocprofv3 --stats run: the new kernels, and everything else."""
    path = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))[-1]
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"{'kernel':60s} {'calls':>6s} {'total ms':>9s} {'share %':>8s}")
    for r in rows:
        if any(k in r["Name"] for k in NEW_KERNELS):
            print(f"{r['Name'][:60]:60s} {r['Calls']:>6s} {float(r['TotalDurationNs']) / 1e6:9.3f} "
                  f"{100 * float(r['TotalDurationNs']) / total:8.2f}")
    conv = sum(float(r["TotalDurationNs"]) for r in rows if not any(k in r["Name"] for k in NEW_KERNELS))
    print(f"{'all other kernels':60s} {'':>6s} {conv / 1e6:9.3f} {100 * conv / total:8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, nargs="+", default=[4, 6])
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--forward-only", action="store_true", help="time the no-grad forward alone (for a kernel-share profile)")
    ap.add_argument("--shares", help="summarise a rocprofv3 --stats output directory instead of timing")
    args = ap.parse_args()
    if args.shares:
        return shares(args.shares)
    prog = importlib.import_module("speak-hack_amd.progan")
    ops = importlib.import_module("speak-hack_amd.ops")
    import progan_critic_ref as CR
    dev = torch.device("cuda:0")
    B = args.batch
    d = prog.Discriminator(512)
    d.load_state_dict(CR.critic_recipe_state_dict(d.state_dict()))
    d.to(dev)
    rows = []
    for steps in args.steps:
        r = 4 * 2 ** steps
        g = torch.Generator(device="cpu").manual_seed(steps)
        x = (torch.rand((B, 3, r, r), generator=g) * 2 - 1).to(dev)
        fake = (torch.rand((B, 3, r, r), generator=g) * 2 - 1).to(dev)
        eps = torch.rand((B, 1, 1, 1), generator=g).to(dev)

        def fwd():
            with torch.no_grad():
                d(x, args.alpha, steps)

        def fwd_bwd():
            xi = x.detach().requires_grad_(True)
            d(xi, args.alpha, steps).sum().backward()

        def penalty():
            gp, _ = CR.wgan_gp(lambda t: d(t, args.alpha, steps), x, fake, eps)
            gp.backward()

        gf = critic_gflop(steps) * B
        if args.forward_only:
            t_f = ev_ms(fwd, args.reps)
            print(json.dumps(dict(steps=steps, res=r, batch=B, ms_fwd=round(t_f, 3), tflops_fwd=round(gf / t_f, 2))))
            continue
        t_f, t_fb, t_gp = ev_ms(fwd, args.reps), ev_ms(fwd_bwd, args.reps), ev_ms(penalty, args.reps)
        rows.append(dict(steps=steps, res=r, batch=B, gflop_fwd=round(gf, 2), ms_fwd=round(t_f, 3),
                         tflops_fwd=round(gf / t_f, 2), ms_fwd_bwd=round(t_fb, 3), tflops_fwd_bwd=round(3 * gf / t_fb, 2),
                         ms_penalty_step=round(t_gp, 3)))
        print(json.dumps(rows[-1]))
    if args.forward_only:
        return
    # the pool alone: the new kernel (16-byte path) against the FIR blur with a 2x2 box filter at stride 2
    xp = torch.randn((8, 128, 256, 256), device=dev)
    box = [[0.25, 0.25], [0.25, 0.25]]
    assert torch.equal(ops.avgpool2x_blend(xp), ops.blur2d(xp, box, 2)) or \
        float((ops.avgpool2x_blend(xp) - ops.blur2d(xp, box, 2)).abs().max()) < 1e-6
    t_new = ev_ms(lambda: ops.avgpool2x_blend(xp), 4 * args.reps)
    t_blur = ev_ms(lambda: ops.blur2d(xp, box, 2), 4 * args.reps)
    gb = xp.numel() * 4 * 1.25 / 1e9
    print(json.dumps(dict(pool_shape=[8, 128, 256, 256], ms_avgpool2x_blend=round(t_new, 4), ms_blur2d_box=round(t_blur, 4),
                          gbps_avgpool2x_blend=round(gb / t_new * 1e3, 1), gbps_blur2d_box=round(gb / t_blur * 1e3, 1))))


if __name__ == "__main__":
    main()
