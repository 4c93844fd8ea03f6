"""tools/isa_gap_budget.py on a hand-written assembly text whose answers can be worked out on paper."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("isa_gap_budget", os.path.join(ROOT, "tools", "isa_gap_budget.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# A kernel with an outer loop (.LBB0_1) around an inner loop (.LBB0_2) of four MFMAs; a second symbol with more MFMAs that must be ignored.
ASM = """
\t.text
other_kernel:
.LBB9_1:
\tv_mfma_f32_32x32x2_f32 a[0:15], v1, v2, a[0:15]
\tv_mfma_f32_32x32x2_f32 a[0:15], v1, v2, a[0:15]
\tv_mfma_f32_32x32x2_f32 a[0:15], v1, v2, a[0:15]
\tv_mfma_f32_32x32x2_f32 a[0:15], v1, v2, a[0:15]
\tv_mfma_f32_32x32x2_f32 a[0:15], v1, v2, a[0:15]
\ts_cbranch_scc0 .LBB9_1
.Lfunc_end9:
toy_kernel:                             ; @toy_kernel
\ts_load_dword s0, s[4:5], 0x0
.LBB0_1:                                ; outer loop
\tv_mov_b32_e32 v9, 0
.LBB0_2:                                ; inner loop
\tds_read_b32 v1, v8
\tds_read_b32 v2, v8 offset:256
\ts_waitcnt lgkmcnt(0)
\tv_mfma_f32_32x32x2_f32 a[0:15], v1, v2, a[0:15]
\ts_add_u32 s2, s2, 0x400
\ts_addc_u32 s3, s3, 0
\t;;#ASMSTART
\ts_mov_b32 m0, s6
\ts_nop 0
\tglobal_load_lds_dwordx4 v47, s[2:3]
\t;;#ASMEND
\t; sched_barrier mask(0x00000000)
\tv_mfma_f32_32x32x2_f32 a[16:31], v1, v2, a[16:31]
\tbuffer_load_dword v10, s[40:43], s81 offen lds
\tv_add_f32 v3, v4, v5
\tv_sub_f32 v4, v4, v5
\tv_mfma_f32_32x32x2_f32 a[32:47], v1, v2, a[32:47]
\tglobal_load_lds_dwordx4 v47, s[2:3] offset:1024
\tglobal_load_lds_dwordx4 v47, s[2:3] offset:2048
\tv_mfma_f32_32x32x2_f32 a[48:63], v1, v2, a[48:63]
\tbuffer_load_dword v11, s[40:43], 0 offen
\ts_barrier
\ts_cbranch_scc0 .LBB0_2
\tglobal_store_dword v[0:1], v3, off
\ts_cbranch_vccz .LBB0_1
\ts_endpgm
.Lfunc_end0:
"""


def test_picks_the_innermost_loop_of_the_symbol():
    t = _tool()
    loop = t.hottest_loop(t.kernel_body(ASM, "toy_kernel"))
    assert loop[0].startswith(".LBB0_2:") and "s_cbranch_scc0 .LBB0_2" in loop[-1]
    assert sum(1 for _, i in t.instructions(loop) if t.classify(i) == "mfma") == 4


def test_classes():
    t = _tool()
    assert t.classify("buffer_load_dword v10, s[40:43], s81 offen lds") == "dma_x1"
    assert t.classify("buffer_load_dword v11, s[40:43], 0 offen") == "vmem"
    assert t.classify("global_load_lds_dwordx4 v47, s[2:3] offset:1024") == "dma_x4"
    assert t.classify("s_nop 0") == "nop" and t.classify("s_waitcnt vmcnt(0)") == "wait" and t.classify("s_barrier") == "ctrl"
    assert t.classify("v_accvgpr_read_b32 v1, a3") == "valu" and t.classify("ds_write_b32 v1, v2") == "lds"
    with pytest.raises(ValueError):
        t.classify("frobnicate v1")


def test_gaps_and_overflow_default_table():
    t = _tool()
    r = t.analyse(ASM, "toy_kernel", chunk=4)
    # gap 0: mfma 8 + 3 salu 12 + nop 4 + x4 piece 60                                   = 84 -> +20
    # gap 1: mfma 8 + gather 60 + 2 valu 8                                              = 76 -> +12
    # gap 2: mfma 8 + two x4 pieces 120                                                 = 128 -> +64
    # gap 3: mfma 8 + vmem 4 + barrier 0 + branch 0, and the wrapped head: 2 lds 8 + wait 4 = 24
    assert r["costs"] == [84, 76, 128, 24]
    assert r["n_chunks"] == 1 and r["overflow"] == 96 and r["over"] == 3
    assert r["dma_gaps"] == 3 and r["multi_dma_gaps"] == 1
    pc = r["per_chunk"]
    assert (pc["mfma"], pc["valu"], pc["salu"], pc["nop"], pc["lds"], pc["dma_x4"], pc["dma_x1"], pc["vmem"], pc["wait"], pc["ctrl"]) == \
        (4, 2, 3, 1, 2, 3, 1, 1, 1, 2)


def test_cost_overrides_and_chunking(capsys):
    t = _tool()
    r = t.analyse(ASM, "toy_kernel", {"dma_x4": 30, "dma_x1": 20}, budget=40, chunk=2)
    assert r["costs"] == [54, 36, 68, 24] and r["n_chunks"] == 2
    assert r["overflow"] == (14 + 28) / 2 and r["over"] == 1
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".s") as f:
        f.write(ASM)
        f.flush()
        t.main([f.name, "toy_kernel", "--dma-x4", "30", "--dma-x1", "20", "--budget", "40", "--chunk", "2", "--gaps"])
    out = capsys.readouterr().out
    assert "summed overflow 21 cycles" in out and out.count("\ngap") + out.startswith("gap") == 4
