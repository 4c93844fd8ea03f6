#!/usr/bin/env python3
"""Per-MFMA-gap issue budget of a kernel's hottest loop, from the device assembly (with one wave per SIMD the
issue costs of everything that sits between two f32 MFMAs add up, and a gap runs at max(MFMA time, their sum)).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -o k.s speak-hack_amd/csrc/conv3x3_wino_f32.hip
    python tools/isa_gap_budget.py k.s _ZN7spkwino11wino_kernelILb0ELi0ELb0ELb0EEEvNS_4ArgsE [--dma-x4 30] [--gaps]

The loop is the span of a backward branch inside the symbol that holds the most MFMAs (ties: the shortest span, i.e. the innermost
loop).  It is cut at every MFMA: gap g = MFMA g and everything up to the next MFMA (the loop's instructions in front of its first
MFMA belong to the last gap: the loop wraps).  Classes and default costs in cycles (the microarchitecture guide's measured issue
costs for one wave per SIMD; every one has an option):

    mfma 8 | valu 4 | salu 4 | nop 4 (s_nop) | lds 4 (ds_*) | dma-x4 60 (global_load_lds_dwordx4: a 1 KiB piece)
    dma-x2 30 | dma-x1 60 (a dword `... lds` load: a 64-lane gather) | vmem 4 (other global_/buffer_/flat_/scratch_)
    wait 4 (s_waitcnt) | ctrl 0 (s_barrier, branches) | budget 64 (the f32 32x32x2 MFMA's pipe time)

Prints per chunk (--chunk MFMAs, default 64; a loop of several chunks is averaged): instruction counts by class, gaps over budget
and the summed overflow; with --gaps one line per gap."""
from __future__ import annotations

import argparse
import re
import sys
from collections import Counter

CLASSES = ("mfma", "valu", "salu", "nop", "lds", "dma_x4", "dma_x2", "dma_x1", "vmem", "wait", "ctrl")
DEFAULT_COST = {"mfma": 8, "valu": 4, "salu": 4, "nop": 4, "lds": 4, "dma_x4": 60, "dma_x2": 30, "dma_x1": 60, "vmem": 4, "wait": 4, "ctrl": 0}
DEFAULT_BUDGET = 64


def classify(ins: str) -> str:
    """Class of one instruction line (mnemonic and operands, no comment)."""
    op = ins.split()[0]
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        if op.startswith("global_load_lds_") or (op.startswith("buffer_load_") and re.search(r"\blds\b", ins[len(op):])):
            if "dwordx4" in op:
                return "dma_x4"
            if "dwordx2" in op or "dwordx3" in op:
                return "dma_x2"
            return "dma_x1"
        return "vmem"
    if op == "s_nop":
        return "nop"
    if op == "s_waitcnt" or op.startswith("s_waitcnt_"):
        return "wait"
    if op == "s_barrier" or op.startswith(("s_branch", "s_cbranch")):
        return "ctrl"
    if op.startswith("s_"):
        return "salu"
    raise ValueError(f"unclassified instruction: {ins!r}")


def instructions(lines):
    """(index, text) of the instruction lines: no labels, directives, comments or the compiler's asm markers."""
    out = []
    for i, l in enumerate(lines):
        t = l.split(";", 1)[0].strip()
        if not t or t.endswith(":") or t.startswith("."):
            continue
        out.append((i, t))
    return out


def kernel_body(text: str, symbol: str):
    lines = text.split("\n")
    start = next((i for i, l in enumerate(lines) if l.startswith(symbol + ":")), None)
    if start is None:
        raise SystemExit(f"symbol {symbol} not found")
    end = next((i for i in range(start + 1, len(lines)) if lines[i].startswith(".Lfunc_end")), len(lines))
    return lines[start + 1:end]


def hottest_loop(body):
    """The lines of the backward-branch span with the most MFMAs (ties: the shortest)."""
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^([.\w$]+):", l)
        if m:
            labels[m.group(1)] = i
    best = None
    for i, l in enumerate(body):
        m = re.match(r"^\s+s_(?:cbranch_\w+|branch)\s+([.\w$]+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            seg = body[labels[m.group(1)]:i + 1]
            nm = sum(1 for _, t in instructions(seg) if classify(t) == "mfma")
            key = (-nm, len(seg))
            if nm and (best is None or key < best[0]):
                best = (key, seg)
    if best is None:
        raise SystemExit("no loop with an MFMA in the symbol")
    return best[1]


def gaps_of(loop_lines):
    """One Counter of classes per gap, and the instruction texts per gap."""
    ins = [t for _, t in instructions(loop_lines)]
    cls = [classify(t) for t in ins]
    first = cls.index("mfma")
    order = list(range(first, len(ins))) + list(range(first))        # the loop wraps: its head joins the last gap
    gaps, texts = [], []
    for k in order:
        if cls[k] == "mfma":
            gaps.append(Counter())
            texts.append([])
        gaps[-1][cls[k]] += 1
        texts[-1].append(ins[k])
    return gaps, texts


def price(gap: Counter, cost) -> int:
    return sum(cost[c] * n for c, n in gap.items())


def analyse(text: str, symbol: str, cost=None, budget=DEFAULT_BUDGET, chunk=64):
    cost = dict(DEFAULT_COST, **(cost or {}))
    gaps, texts = gaps_of(hottest_loop(kernel_body(text, symbol)))
    costs = [price(g, cost) for g in gaps]
    n_chunks = max(1, len(gaps) // chunk)
    total = Counter()
    for g in gaps:
        total.update(g)
    return {
        "gaps": gaps, "texts": texts, "costs": costs, "n_chunks": n_chunks,
        "per_chunk": {c: total[c] / n_chunks for c in CLASSES},
        "over": sum(1 for c in costs if c > budget) / n_chunks,
        "overflow": sum(max(0, c - budget) for c in costs) / n_chunks,
        "dma_gaps": sum(1 for g in gaps if g["dma_x4"] + g["dma_x2"] + g["dma_x1"]) / n_chunks,
        "multi_dma_gaps": sum(1 for g in gaps if g["dma_x4"] + g["dma_x2"] + g["dma_x1"] > 1) / n_chunks,
        "budget": budget, "cost": cost,
    }


def fmt(x: float) -> str:
    return f"{x:g}"


def report(r, show_gaps=False, out=sys.stdout):
    if show_gaps:
        for k, (g, c) in enumerate(zip(r["gaps"], r["costs"])):
            what = " ".join(f"{cl}={g[cl]}" for cl in CLASSES if g[cl])
            print(f"gap {k % (len(r['gaps']) // r['n_chunks']):3d} chunk {k // (len(r['gaps']) // r['n_chunks'])}: {what:60s} cost {c:4d}"
                  f"{'  +' + str(c - r['budget']) if c > r['budget'] else ''}", file=out)
    print(f"loop: {len(r['gaps'])} MFMA gaps = {r['n_chunks']} chunk(s); per chunk: "
          + ", ".join(f"{cl} {fmt(r['per_chunk'][cl])}" for cl in CLASSES if r["per_chunk"][cl]), file=out)
    print(f"per chunk: gaps with a DMA {fmt(r['dma_gaps'])} (more than one: {fmt(r['multi_dma_gaps'])}), gaps over the budget of "
          f"{r['budget']}: {fmt(r['over'])}, summed overflow {fmt(r['overflow'])} cycles", file=out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("symbol")
    for c in CLASSES:
        ap.add_argument("--" + c.replace("_", "-"), type=int, default=DEFAULT_COST[c], help=f"cycles per {c} instruction")
    ap.add_argument("--budget", type=int, default=DEFAULT_BUDGET, help="cycles of a gap that cost nothing (the MFMA's pipe time)")
    ap.add_argument("--chunk", type=int, default=64, help="MFMAs per chunk")
    ap.add_argument("--gaps", action="store_true", help="one line per gap")
    a = ap.parse_args(argv)
    r = analyse(open(a.asm).read(), a.symbol, {c: getattr(a, c) for c in CLASSES}, a.budget, a.chunk)
    report(r, a.gaps)
    return r


if __name__ == "__main__":
    main()
