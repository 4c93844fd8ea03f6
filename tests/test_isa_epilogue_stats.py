"""tools/isa_epilogue_stats.py: its parser on a hand-written assembly text whose answers can be counted on paper, and the bounds the
Winograd forward kernel's region epilogue is held to on the assembly the build's own flags produce."""
import importlib
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("isa_epilogue_stats", os.path.join(ROOT, "tools", "isa_epilogue_stats.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# toy_wino_kernelIxE: a K loop, then two "rows"; one accumulator read and one store of another symbol that must be ignored, a store in
# front of the first read (outside the window) and work behind the last store (outside as well).
ASM = """
\t.text
other_wino_kernelIyE:
\tv_accvgpr_read_b32 v1, a0
\ts_cbranch_scc0 .LBB9_1
.LBB9_1:
\tglobal_store_dwordx2 v[0:1], v[2:3], off
\ts_endpgm
.Lfunc_end9:
toy_wino_kernelIxE:                     ; @toy_wino_kernelIxE
\tglobal_store_dwordx2 v[0:1], v[2:3], off
\ts_waitcnt vmcnt(0)
.LBB0_1:
\tv_mfma_f32_32x32x2_f32 a[0:15], v1, v2, a[0:15]
\ts_cbranch_scc0 .LBB0_1
\t;;#ASMSTART
\tv_accvgpr_read_b32 v4, a0
\tv_accvgpr_read_b32 v5, a16
\tv_add_f32 v4, v4, v5
\t;;#ASMEND
\ts_waitcnt vmcnt(1)
\tv_fma_f32 v4, v4, v6, v7
\tv_cmp_lt_f32_e32 vcc, 0, v4
\tv_cndmask_b32_e32 v4, v8, v4, vcc
\ts_nop 0
\tv_mov_b32_e32 v9, v4
\tv_mad_u64_u32 v[10:11], s[0:1], s2, v12, 0
\tv_lshl_add_u64 v[10:11], v[10:11], 2, s[4:5]
\ts_cbranch_scc1 .LBB0_3
\tglobal_store_dwordx2 v[10:11], v[8:9], off
.LBB0_3:
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tv_accvgpr_read_b32 v4, a1
\tv_max_f32_e32 v4, v4, v5
\ts_waitcnt lgkmcnt(0)
\tglobal_store_dwordx2 v13, v[4:5], s[6:7] offset:16
\ts_waitcnt vmcnt(0)
\ts_cbranch_vccz .LBB0_1
\ts_endpgm
.Lfunc_end0:
\t.section\t.rodata
amdhsa.kernels:
  - .args:
      - .offset:         0
        .size:           8
    .name:           other_wino_kernelIyE
    .private_segment_fixed_size: 80
    .vgpr_count:     12
    .vgpr_spill_count: 19
  - .args:
      - .offset:         0
    .name:           pack_wino_kernel
    .private_segment_fixed_size: 4
    .vgpr_spill_count: 1
  - .args:
      - .offset:         0
    .name:           toy_wino_kernelIxE
    .private_segment_fixed_size: 0
    .vgpr_spill_count: 0
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
"""


def test_window_runs_from_first_accumulator_read_to_last_store():
    t = _tool()
    win = t.window(t.instructions(t.kernel_body(ASM, "toy_wino_kernelIxE")))
    assert win[0] == "v_accvgpr_read_b32 v4, a0" and win[-1] == "global_store_dwordx2 v13, v[4:5], s[6:7] offset:16"
    assert len(win) == 18
    with pytest.raises(ValueError):
        t.window(["v_add_f32 v1, v2, v3", "global_store_dwordx2 v[0:1], v[2:3], off"])
    with pytest.raises(ValueError):
        t.window(["global_store_dwordx2 v[0:1], v[2:3], off", "v_accvgpr_read_b32 v4, a0"])


def test_counts_of_the_window():
    t = _tool()
    c = t.epilogue_stats(ASM, "toy_wino_kernelIxE")
    assert c == {"instructions": 18, "vmcnt1": 1, "vmcnt0": 1, "vmcnt": 2, "branches": 1, "addr64": 2, "cmp_f32": 1, "cndmask": 1, "nop": 1,
                 "mov": 1, "acc_reads": 3, "stores": 2}
    o = t.epilogue_stats(ASM, "other_wino_kernelIyE")
    assert (o["instructions"], o["branches"], o["acc_reads"], o["stores"], o["vmcnt"]) == (3, 1, 1, 1, 0)


def test_metadata_and_report(capsys, tmp_path):
    t = _tool()
    meta = t.metadata(ASM)
    assert meta == {"other_wino_kernelIyE": {"vgpr_spill_count": 19, "private_segment_fixed_size": 80},
                    "toy_wino_kernelIxE": {"vgpr_spill_count": 0, "private_segment_fixed_size": 0}}         # (pack_wino_kernel: no instantiation)
    assert set(t.metadata(ASM, "wino_kernel")) == {"other_wino_kernelIyE", "pack_wino_kernel", "toy_wino_kernelIxE"}
    f = tmp_path / "toy.s"
    f.write_text(ASM)
    assert t.main([str(f)]) == 0
    out = capsys.readouterr().out
    assert "toy_wino_kernelIxE\n    instructions 18  vmcnt1 1  vmcnt0 1  vmcnt 2  branches 1  addr64 2" in out
    assert "other_wino_kernelIyE: vgpr_spill_count 19  private_segment_fixed_size 80" in out and "pack_wino_kernel:" not in out


# ---- the compiled kernel ----
def _forms(names):
    """{(MOD, SHAPE, RGB, UP, EPI): symbol} of the wino_kernel instantiations"""
    out = {}
    for n in names:
        m = re.fullmatch(r"_ZN7spkwino11wino_kernelILb([01])ELi([01])ELb([01])ELb([01])ELi([0-2])EEEvNS_4ArgsE", n)
        assert m, n
        out[tuple(int(v) for v in m.groups())] = n
    return out


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_compiled_kernel_epilogue_bounds(tmp_path):
    """The kernel's translation unit, compiled to assembly with the library's flags.  LEAN rows (EPI 1, and EPI 2: the toRGB form that
    does not store the activation): no branch, at most two vmcnt waits, no 64-bit vector address arithmetic, no f32 compare.  The x2
    fused-toRGB forms the decoder runs (lean): no branch, at most four vmcnt waits.  The non-x2 toRGB forms and the generic forms
    are printed, not bounded.  Every instantiation: no scratch, no spilled register."""
    t = _tool()
    sys.path.insert(0, ROOT)
    bld = importlib.import_module("speak-hack_amd.build")
    src = os.path.join(bld.CSRC, "conv3x3_wino_f32.hip")
    asm = tmp_path / "wino.s"
    subprocess.run([bld._hipcc(), *bld.FLAGS, *bld._file_flags(src), "--cuda-device-only", "-S", src, "-o", str(asm)], check=True,
                   capture_output=True)
    text = asm.read_text()
    meta = t.metadata(text)
    forms = _forms(meta)
    GENERIC, LEAN, LEAN_NOSTORE = 0, 1, 2
    # what the launcher can pick: plain {shape} x {up} x {generic, lean}; toRGB the same plus the no-store form; modulated generic only
    want = {(0, s, 0, u, e) for s in (0, 1) for u in (0, 1) for e in (GENERIC, LEAN)} | \
           {(0, s, 1, u, e) for s in (0, 1) for u in (0, 1) for e in (GENERIC, LEAN, LEAN_NOSTORE)} | {(1, s, 0, 0, GENERIC) for s in (0, 1)}
    assert set(forms) == want
    stats = {k: t.epilogue_stats(text, n) for k, n in forms.items()}
    for k in sorted(stats):
        print(k, "  ".join(f"{a} {b}" for a, b in stats[k].items()), meta[forms[k]])
    for (mod, shape, rgb, up, epi), c in stats.items():
        if epi != GENERIC and not rgb:
            assert c["branches"] == 0 and c["vmcnt"] <= 2 and c["addr64"] == 0 and c["cmp_f32"] == 0, ((mod, shape, rgb, up, epi), c)
        if epi != GENERIC and rgb and up:
            assert c["branches"] == 0 and c["vmcnt"] <= 4, ((mod, shape, rgb, up, epi), c)
        if epi != GENERIC:
            assert c["acc_reads"] == 256 and c["stores"] == (2 if epi == LEAN_NOSTORE else 34 if rgb else 32), ((mod, shape, rgb, up, epi), c)
    for n, rec in meta.items():
        assert rec == {"vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (n, rec)
