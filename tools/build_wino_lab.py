#!/usr/bin/env python3
"""LAB: builds of the library whose Winograd forward kernel (csrc/conv3x3_wino_f32.hip) is compiled with -DSPK_WINO_LAB -- the cycle
stamps tools/lab_wino_phases.py reads -- and, one library each, one knock-out of its K loop (-DSPK_WINO_KO=bit):

    tools/_bin/libspk_hip_winolab.so        stamps only
    tools/_bin/libspk_hip_winolab_ko1.so    no U pieces                                  (results are wrong in every ko library:
    tools/_bin/libspk_hip_winolab_ko2.so    no raw gathers                                only the time is read)
    tools/_bin/libspk_hip_winolab_ko4.so    no transform vector ops
    tools/_bin/libspk_hip_winolab_ko8.so    no V writes
    tools/_bin/libspk_hip_winolab_ko16.so   U pieces without their scalar companions

Every other object is the shipped one (speak-hack_amd/_build, built first if need be).
    python tools/build_wino_lab.py [--ko 0 1 2 4 8 16] [-D NAME=VALUE ...] [--tag NAME]"""
import argparse
import importlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ko", type=int, nargs="*", default=[0, 1, 2, 4, 8, 16])
    ap.add_argument("-D", dest="defs", action="append", default=[], help="further -D definitions for the Winograd source")
    ap.add_argument("--tag", default="", help="suffix of the library names (with -D)")
    ap.add_argument("--no-lab", action="store_true", help="without -DSPK_WINO_LAB (an A/B arm of the shipped kernel)")
    args = ap.parse_args()
    bld = importlib.import_module("speak-hack_amd.build")
    bld.build_lib()
    out_dir = os.path.join(ROOT, "tools", "_bin")
    os.makedirs(out_dir, exist_ok=True)
    src = os.path.join(bld.CSRC, "conv3x3_wino_f32.hip")
    others = [os.path.join(bld.OBJ, os.path.basename(s)[:-4] + ".o") for s in bld.sources() if s != src]
    hipcc = bld._hipcc()

    def one(ko):
        name = "winolab" + (f"_{args.tag}" if args.tag else "") + (f"_ko{ko}" if ko else "")
        obj, lib = os.path.join(out_dir, name + ".o"), os.path.join(out_dir, f"libspk_hip_{name}.so")
        defs = ([] if args.no_lab else ["-DSPK_WINO_LAB"]) + ([f"-DSPK_WINO_KO={ko}"] if ko else []) + ["-D" + d for d in args.defs]
        subprocess.run([hipcc, *bld.FLAGS, *bld._file_flags(src), *defs, "-c", src, "-o", obj], check=True)
        subprocess.run([hipcc, "-shared", "-fPIC", f"--offload-arch={bld.ARCH}", "-o", lib, obj, *others], check=True)
        return lib

    with ThreadPoolExecutor(max_workers=6) as ex:
        for lib in ex.map(one, args.ko):
            print(lib)


if __name__ == "__main__":
    main()
