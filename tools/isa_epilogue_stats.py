#!/usr/bin/env python3
"""Instruction counts of the Winograd kernel's region epilogue, from the device assembly.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -o k.s speak-hack_amd/csrc/conv3x3_wino_f32.hip
    python tools/isa_epilogue_stats.py k.s                      # every wino_kernel of the file
    python tools/isa_epilogue_stats.py k.s _ZN7spkwino11wino_kernelILb0ELi0ELb0ELb0ELi1EEEvNS_4ArgsE

The window of a symbol runs from its first `v_accvgpr_read_b32` to its last `global_store_dwordx2`, both included, in program order.
Counted inside it: instructions, `s_waitcnt` with vmcnt(1) / vmcnt(0) / any vmcnt, conditional branches (`s_cbranch_*`), 64-bit
vector address operations (`v_lshl_add_u64`, `v_mad_u64_u32`), f32 compares (`v_cmp_*_f32`), `v_cndmask_*`, `s_nop`, `v_mov_b32`,
accumulator reads and the stores.  From the file's metadata (`amdhsa.kernels`): `vgpr_spill_count` and `private_segment_fixed_size`
of every kernel whose name contains --match (default `wino_kernelI`: the template's instantiations)."""
from __future__ import annotations

import argparse
import re
import sys

COUNTS = ("instructions", "vmcnt1", "vmcnt0", "vmcnt", "branches", "addr64", "cmp_f32", "cndmask", "nop", "mov", "acc_reads", "stores")


def kernel_body(text: str, symbol: str):
    lines = text.split("\n")
    start = next((i for i, l in enumerate(lines) if l.startswith(symbol + ":")), None)
    if start is None:
        raise SystemExit(f"symbol {symbol} not found")
    end = next((i for i in range(start + 1, len(lines)) if lines[i].startswith(".Lfunc_end")), len(lines))
    return lines[start + 1:end]


def instructions(lines):
    """The instruction lines, in order: no labels, directives, comments or the compiler's asm markers."""
    out = []
    for l in lines:
        t = l.split(";", 1)[0].strip()
        if not t or t.endswith(":") or t.startswith("."):
            continue
        out.append(t)
    return out


def window(ins):
    """first accumulator read .. last 8-byte global store"""
    first = next((i for i, t in enumerate(ins) if t.startswith("v_accvgpr_read_b32")), None)
    last = next((i for i in range(len(ins) - 1, -1, -1) if ins[i].startswith("global_store_dwordx2")), None)
    if first is None or last is None or last < first:
        raise ValueError("no epilogue window: the symbol has no v_accvgpr_read_b32 followed by a global_store_dwordx2")
    return ins[first:last + 1]


def count(win):
    c = dict.fromkeys(COUNTS, 0)
    c["instructions"] = len(win)
    for t in win:
        op = t.split()[0]
        if op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", t)
            if m:
                c["vmcnt"] += 1
                if m.group(1) == "1":
                    c["vmcnt1"] += 1
                if m.group(1) == "0":
                    c["vmcnt0"] += 1
        elif op.startswith("s_cbranch_"):
            c["branches"] += 1
        elif op.startswith(("v_lshl_add_u64", "v_mad_u64_u32")):
            c["addr64"] += 1
        elif re.match(r"v_cmpx?_\w+_f32", op):
            c["cmp_f32"] += 1
        elif op.startswith("v_cndmask"):
            c["cndmask"] += 1
        elif op == "s_nop":
            c["nop"] += 1
        elif op.startswith("v_mov_b32"):
            c["mov"] += 1
        elif op.startswith("v_accvgpr_read_b32"):
            c["acc_reads"] += 1
        elif op.startswith("global_store_"):
            c["stores"] += 1
    return c


def epilogue_stats(text: str, symbol: str):
    return count(window(instructions(kernel_body(text, symbol))))


def metadata(text: str, match: str = "wino_kernelI"):
    """{kernel name: {"vgpr_spill_count": n, "private_segment_fixed_size": n}} from the amdhsa.kernels list."""
    out = {}
    m = re.search(r"^amdhsa\.kernels:\s*$", text, re.M)
    if not m:
        return out
    for entry in re.split(r"^  - ", text[m.end():], flags=re.M)[1:]:
        entry = entry.split("\namdhsa.", 1)[0]
        name = re.search(r"^\s*\.name:\s*(\S+)", entry, re.M)
        if not name or match not in name.group(1):
            continue
        rec = {}
        for key in ("vgpr_spill_count", "private_segment_fixed_size"):
            v = re.search(rf"^\s*\.{key}:\s*(\d+)", entry, re.M)
            rec[key] = int(v.group(1)) if v else None
        out[name.group(1)] = rec
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("symbols", nargs="*", help="default: every kernel of the metadata that matches")
    ap.add_argument("--match", default="wino_kernelI")
    args = ap.parse_args(argv)
    text = open(args.asm).read()
    meta = metadata(text, args.match)
    for sym in args.symbols or sorted(meta):
        c = epilogue_stats(text, sym)
        print(sym)
        print("    " + "  ".join(f"{k} {c[k]}" for k in COUNTS))
    for name in sorted(meta):
        print(f"{name}: vgpr_spill_count {meta[name]['vgpr_spill_count']}  private_segment_fixed_size {meta[name]['private_segment_fixed_size']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
