"""CPU-side checks of the aligned I420 edge (csrc/frame_sim_i420.hip, csrc/frame_table_i420.hip): the shapes and refusals of
``ops.i420_planes``; ``spk_planar_table_check`` through ctypes on host tables packed with numpy -- the tables that must pass, each
refusal and the entry (or pair of planes) it names, overlap refused only where the surfaces are written, extents that leave 64 bits
-- the 56-byte layout of ``spk_planar_ref`` against include/spk.h; the ``ValueError``s of ``ops.PlanarTable`` (raised before a
device is touched, nothing copied); the argument refusals of the eight launching entry points (which return before a launch, so no
GPU is needed); the host refusals of ``IRFD.live(pixel_format="i420")``; and the cases of tests/i420_cases.py against the NV12 cases
they came from.  These are the checks of tests/test_surface_table_cpu.py, for three planes."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import i420_cases as IC
import nv12_sim_cases as NS
import surface_table_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = np.dtype([("y", "<u8"), ("u", "<u8"), ("v", "<u8"), ("y_row_stride", "<i8"), ("u_row_stride", "<i8"), ("v_row_stride", "<i8"),
                ("H", "<i4"), ("W", "<i4")])
BASE = 0x7000_0000_0000                                                     # addresses are numbers here: the check never follows them
ZERO = (0,) * 8
u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")


def packed(entries):
    t = np.zeros(len(entries), dtype=REF)
    for n, e in enumerate(entries):
        t[n] = e
    return t


def check(pkg, table, written, N=None):
    """-> (code, message)"""
    lib = pkg._lib.lib()
    rc = lib.spk_planar_table_check(table.ctypes.data if table is not None else None, len(table) if N is None else N, written)
    return rc, lib.spk_last_error().decode()


# entry 0: 4 x 6 at pitch 16, Y [0, 54); U two rows of 3 bytes at the ODD pitch 3, [54, 60); V at pitch 5 from the ODD address 61,
# [61, 69).  entry 1: 2 x 2 packed, V FIRST: V at 69, U at 70, Y [71, 75).  entry 2: absent.  entry 3: 6 x 4, Y [4096, 4120), U and
# V (three rows of 2 bytes) in separate allocations far apart
GOOD = [(BASE, BASE + 54, BASE + 61, 16, 3, 5, 4, 6), (BASE + 71, BASE + 70, BASE + 69, 2, 1, 1, 2, 2), ZERO,
        (BASE + 4096, BASE + 2 ** 32, BASE + 2 ** 33, 4, 2, 2, 6, 4)]


def edited(n, **fields):
    e = [list(g) for g in GOOD]
    for k, v in fields.items():
        e[n][REF.names.index(k)] = v
    return packed([tuple(g) for g in e])


# ---- ops.i420_planes ----------------------------------------------------------------------------------------------------------------
def test_i420_planes_shapes_and_refusals(pkg):
    f = pkg.ops.i420_planes
    buf = torch.arange(2 * 6 * 4, dtype=torch.uint8).view(2, 6, 4)          # two packed 4 x 4 surfaces
    y, u, v = f(buf)
    assert tuple(y.shape) == (2, 4, 4) and tuple(u.shape) == tuple(v.shape) == (2, 2, 2)
    assert torch.equal(y, buf[:, :4]) and torch.equal(u.flatten(1), buf.view(2, -1)[:, 16:20]) and torch.equal(v.flatten(1), buf.view(2, -1)[:, 20:24])
    assert y.data_ptr() == buf.data_ptr() and u.data_ptr() == buf.data_ptr() + 16 and v.data_ptr() == buf.data_ptr() + 20        # views
    assert u.stride() == (24, 2, 1)                                         # a packed chroma plane: pitch W / 2
    one = f(buf[1])
    assert [tuple(t.shape) for t in one] == [(1, 4, 4), (1, 2, 2), (1, 2, 2)] and one[2].data_ptr() == buf.data_ptr() + 24 + 20
    assert f(u8(2, 9, 6))[1].stride(1) == 3                                 # W / 2 odd: an odd packed pitch
    triple = (u8(3, 4, 6), u8(3, 2, 3), u8(3, 2, 3))
    assert all(a is b for a, b in zip(f(triple), triple)) and all(a is b for a, b in zip(f(list(triple)), triple))
    assert [tuple(t.shape) for t in f((u8(4, 6), u8(2, 3), u8(2, 3)))] == [(1, 4, 6), (1, 2, 3), (1, 2, 3)]
    wide = u8(3, 8, 16)
    views = (wide[:, 2:6, 4:10], u8(3, 2, 7)[:, :, 1:4], u8(3, 4, 3)[:, ::2])      # any pitch, any offset
    assert all(a is b for a, b in zip(f(views), views))
    bad = {"a number": 7, "a pair": (u8(2, 4, 6), u8(2, 2, 3)), "a string among them": (u8(2, 4, 6), u8(2, 2, 3), "v"),
           "a 4-d tensor": u8(1, 2, 6, 4), "no frames": u8(0, 6, 4), "rows not 3H/2": u8(2, 7, 4), "an odd W": u8(2, 6, 5), "an odd H": u8(2, 9, 4)[:, :3],
           "float": u8(2, 6, 4).float(), "a pitched packed tensor": u8(2, 6, 8)[:, :, :4], "a sliced packed tensor": u8(4, 6, 4)[::2],
           "a transposed one": u8(2, 4, 6).transpose(1, 2), "a float plane": (u8(2, 4, 6), u8(2, 2, 3).float(), u8(2, 2, 3)),
           "a small U": (u8(2, 4, 6), u8(2, 2, 2), u8(2, 2, 3)), "a full-size V": (u8(2, 4, 6), u8(2, 2, 3), u8(2, 4, 6)),
           "an odd Y": (u8(2, 3, 6), u8(2, 1, 3), u8(2, 1, 3)), "counts that differ": (u8(2, 4, 6), u8(3, 2, 3), u8(2, 2, 3)),
           "ranks that differ": (u8(2, 4, 6), u8(2, 3), u8(2, 2, 3)), "nv12 chroma": (u8(2, 4, 6), u8(2, 2, 3, 2), u8(2, 2, 3))}
    for name, arg in bad.items():
        with pytest.raises(ValueError, match="i420"):
            f(arg)


# ---- spk_planar_ref and spk_planar_table_check --------------------------------------------------------------------------------------
def test_the_layout_is_the_header_s(pkg):
    F = pkg._lib.PlanarRef
    assert ctypes.sizeof(F) == 56 == REF.itemsize and ctypes.alignment(F) == 8
    assert [(n, getattr(F, n).offset, getattr(F, n).size) for n, _ in F._fields_] == \
        [("y", 0, 8), ("u", 8, 8), ("v", 16, 8), ("y_row_stride", 24, 8), ("u_row_stride", 32, 8), ("v_row_stride", 40, 8), ("H", 48, 4), ("W", 52, 4)]
    assert [REF.fields[n][1] for n in REF.names] == [0, 8, 16, 24, 32, 40, 48, 52]
    header = open(os.path.join(ROOT, "include", "spk.h")).read()
    m = re.search(r"typedef struct spk_planar_ref \{([^}]*)\} spk_planar_ref;", header)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == \
        "const uint8_t* y; const uint8_t* u; const uint8_t* v; int64_t y_row_stride; int64_t u_row_stride; int64_t v_row_stride; int32_t H, W;"


def test_tables_that_pass(pkg):
    for written in (0, 1):
        assert check(pkg, packed(GOOD), written)[0] == 0                    # odd chroma pitch and base, V before U, ranges that touch
        assert check(pkg, packed([ZERO] * 3), written)[0] == 0              # every surface absent
        assert check(pkg, packed(GOOD[::-1]), written)[0] == 0              # entries out of address order
        assert check(pkg, edited(0, y_row_stride=6, u_row_stride=3, v_row_stride=3), written)[0] == 0      # the smallest strides
        assert check(pkg, edited(3, y=BASE + 75), written)[0] == 0          # Y of 3 right behind Y of 1
        assert check(pkg, edited(0, u=BASE + 2 ** 40, v=BASE + 2 ** 41 + 1), written)[0] == 0           # planes in separate allocations
        assert check(pkg, edited(0, v=BASE + 54, v_row_stride=6, u=BASE + 63), written)[0] == 0         # V [54, 63) before U [63, 69)
    assert check(pkg, edited(1, y_row_stride=2 ** 62, u_row_stride=2 ** 63 - 2, v_row_stride=2 ** 63 - 1), 0)[0] == 0    # one chroma row: its stride does not count


def test_refusals_name_the_entry(pkg):
    assert check(pkg, None, 0, N=4)[0] < 0 and "null" in pkg._lib.lib().spk_last_error().decode()
    for N in (0, -2):
        rc, msg = check(pkg, packed(GOOD), 0, N=N)
        assert rc < 0 and "N must" in msg
    half = [(0, dict(y=0)), (0, dict(u=0)), (0, dict(v=0)), (1, dict(H=0)), (1, dict(H=3)), (3, dict(H=-2)), (0, dict(W=5)), (0, dict(W=0)),
            (3, dict(W=1)), (0, dict(y_row_stride=5)), (0, dict(y_row_stride=-16)), (0, dict(u_row_stride=2)), (0, dict(v_row_stride=2)),
            (0, dict(v_row_stride=-5)), (2, dict(y=BASE + 512)), (2, dict(v=BASE + 512)), (2, dict(u_row_stride=8)), (2, dict(H=2)), (2, dict(W=2)),
            (0, dict(y_row_stride=0, u_row_stride=0, v_row_stride=0, H=0, W=0))]
    for n, fields in half:
        for written in (0, 1):
            rc, msg = check(pkg, edited(n, **fields), written)
            assert rc < 0 and f"entry {n} is half-formed" in msg and "row strides" in msg, (n, fields, msg)


def test_extents_that_leave_64_bits_are_refused(pkg):
    wraps = [(0, dict(y_row_stride=2 ** 62), "Y"), (0, dict(H=2 ** 31 - 2, y_row_stride=2 ** 33), "Y"), (0, dict(u_row_stride=2 ** 63 - 2), "U"),
             (3, dict(v_row_stride=2 ** 62), "V"), (1, dict(y=2 ** 64 - 3), "Y"), (1, dict(u=2 ** 64 - 1), "U"), (1, dict(v=2 ** 64 - 1), "V"),
             (3, dict(y=2 ** 64 - 16), "Y")]
    for n, fields, plane in wraps:
        rc, msg = check(pkg, edited(n, **fields), 0)
        assert rc < 0 and f"entry {n}: the {plane} extent" in msg and "overflows 64 bits" in msg, (n, fields, msg)


def test_overlap_is_refused_only_where_the_surfaces_are_written(pkg):
    cases = [(edited(1, y=BASE + 53), "entries 0 (Y) and 1 (Y) overlap"),                  # the last byte of Y of entry 0
             (edited(1, y=BASE + 66), "entries 0 (V) and 1 (Y) overlap"),                  # Y of one entry against V of another
             (edited(1, u=BASE + 20), "entries 0 (Y) and 1 (U) overlap"),                  # inside the padding columns of Y 0: its byte RANGE
             (edited(1, v=BASE + 59), "entries 0 (U) and 1 (V) overlap"),
             (edited(0, u=BASE + 52), "entries 0 (Y) and 0 (U) overlap"),                  # an entry's own planes
             (edited(0, v=BASE), "entries 0 (Y) and 0 (V) overlap"),
             (edited(0, v=BASE + 58), "entries 0 (U) and 0 (V) overlap"),
             # chroma halves side by side on one pitch: no byte is shared, the ranges [54, 63) and [57, 66) are
             (edited(0, u=BASE + 54, u_row_stride=6, v=BASE + 57, v_row_stride=6), "entries 0 (U) and 0 (V) overlap"),
             (packed([GOOD[0], GOOD[1], GOOD[1], GOOD[3]]), "entries 1 (V) and 2 (V) overlap"),       # twice: the first plane in memory is named
             (edited(3, v=BASE + 2 ** 32 + 5), "entries 3 (U) and 3 (V) overlap")]
    for table, words in cases:
        assert check(pkg, table, 0)[0] == 0, words
        rc, msg = check(pkg, table, 1)
        assert rc < 0 and words in msg, (words, msg)


# ---- ops.PlanarTable ----------------------------------------------------------------------------------------------------------------
def test_planar_table_value_errors_come_before_a_device(pkg, monkeypatch):
    T = pkg.ops.PlanarTable
    copies = []
    monkeypatch.setattr(torch.Tensor, "copy_", lambda self, *a, **k: copies.append(self) or self)      # a refused call copies nothing
    ok = u8(6, 6)                                                           # 4 x 6, packed
    tri = (u8(4, 6), u8(2, 3), u8(2, 3))
    bad = {"not a sequence": 7, "empty": [], "a 4-d tensor": u8(1, 2, 6, 6), "no frames": u8(0, 6, 6), "a string": [ok, "surface"],
           "a number": [ok, 3], "float": [ok, ok.float()], "int8": [ok.to(torch.int8)], "an odd H": [u8(8, 6)[:7]], "an odd W": [u8(6, 5)],
           "rows not 3H/2": [u8(7, 6)], "wrong rank": [u8(1, 1, 6, 6)], "a 3-d element": [u8(2, 6, 6)], "a pitched packed surface": [u8(6, 8)[:, :6]],
           "a pair": [(u8(4, 6), u8(2, 3))], "a float plane": [(u8(4, 6), u8(2, 3).float(), u8(2, 3))], "a small V": [(u8(4, 6), u8(2, 3), u8(2, 2))],
           "an odd triple": [(u8(3, 6), u8(1, 3), u8(1, 3))], "U pixels apart": [(u8(4, 6), u8(2, 6)[:, ::2], u8(2, 3))],
           "Y pixels apart": [(u8(4, 12)[:, ::2], u8(2, 3), u8(2, 3))], "V rows that overlap": [(u8(4, 6), u8(2, 3), u8(1, 3).expand(2, 3))],
           "a triple of two frames among surfaces": [(u8(2, 4, 6), u8(2, 2, 3), u8(2, 2, 3)), ok], "a bad surface behind a good one": [ok, tri, u8(6, 5)],
           "a tensor of odd surfaces": u8(2, 7, 6)}
    for name, surfaces in bad.items():
        with pytest.raises(ValueError, match="PlanarTable|i420"):
            T(surfaces)
    # what has the right shape and strides gets as far as the device check: a packed surface, a triple, pitched planes at odd
    # offsets, a region of interest at even luma offsets as a triple of views, an absent one, a tensor of surfaces, a triple of planes
    wide, cu, cv = u8(8, 16), u8(4, 9), u8(5, 8)
    roi = (wide[2:6, 4:10], cu[1:3, 2:5], cv[1:3, 2:5])
    odd = (u8(4, 7)[:, :6], u8(2, 5)[:, 1:4], u8(7)[1:].view(2, 3))
    for surfaces in ([ok], [tri], [odd], [roi], [None, ok], u8(2, 6, 6), (u8(2, 4, 6), u8(2, 2, 3), u8(2, 2, 3)), [ok, tri, None]):
        with pytest.raises(pkg._lib.SpkError, match="no CPU path"):
            T(surfaces)
    assert not copies


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
def test_the_strided_entry_points_refuse_bad_arguments(pkg):
    lib = pkg._lib.lib()
    buf = np.zeros(8192, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 64
    x, sim, out, ws = base + 1024, base + 2048, base + 4096, 0x10000000
    ok = dict(y=base, y_img=64, y_row=8, u=base + 129, u_img=17, u_row=5, v=base + 192, v_img=16, v_row=4, N=1, H=8, W=8, sim=sim, std=601, full=0)

    def surface(a):
        return (a["y"], a["y_img"], a["y_row"], a["u"], a["u_img"], a["u_row"], a["v"], a["v_img"], a["v_row"])

    def way_in(dst=out, Hout=4, Wout=4, **kw):
        a = dict(ok, **kw)
        return lib.spk_frames_i420_to_f32_sim(*surface(a), a["N"], a["H"], a["W"], a["sim"], 0, a["std"], a["full"], dst, Hout, Wout, 1, 1, 1, 0, 0, 0, None)

    def head(a, src, Hs):
        return (src, a["N"], Hs, 4, *surface(a), a["H"], a["W"], a["sim"], a["std"], a["full"])

    def paste(src=x, Hs=4, feather=0.0, k=127.5, matte=None, mf=0, **kw):
        return lib.spk_frames_paste_i420_sim(*head(dict(ok, **kw), src, Hs), feather, -1.0, k, matte, mf, None, None)

    def sums(src=x, Hs=4, feather=0.0, k=127.5, matte=None, mf=0, out=out, ws=ws, wsb=2 * 64 * 13 * 8, **kw):
        return lib.spk_paste_colour_sums_i420_sim(*head(dict(ok, **kw), src, Hs), feather, -1.0, k, matte, mf, out, ws, wsb, None)

    def match(src=x, Hs=4, feather=0.0, k=127.5, matte=None, mf=0, out=out, ws=ws, wsb=2 * 64 * 13 * 8, gain=2.0, **kw):
        return lib.spk_paste_colour_match_i420_sim(*head(dict(ok, **kw), src, Hs), feather, -1.0, k, matte, mf, gain, 1.0, 16.0, out, ws, wsb, None)

    calls = [(lambda: way_in(dst=None), "null frame pointer"), (lambda: way_in(Hout=0), "output size"), (lambda: way_in(Wout=-1), "output size"),
             (lambda: way_in(N=2, y_img=-64), "negative image stride"), (lambda: sums(N=2, u_img=-1), "negative image stride"),
             (lambda: match(N=2, v_img=-16), "negative image stride"),
             (lambda: paste(N=2, y_img=63), "overlap"), (lambda: paste(N=2, u_img=4 + 3 * 5 - 1), "overlap"), (lambda: paste(N=2, v_img=15), "overlap"),
             (lambda: paste(N=2, v_img=0), "overlap"), (lambda: paste(N=2, u_img=-17), "overlap"),
             (lambda: paste(matte=x, mf=2), "matte_frames"), (lambda: sums(out=None), "null sums"), (lambda: sums(out=out + 4), "aligned"),
             (lambda: sums(wsb=8), "workspace"), (lambda: sums(ws=None), "workspace"), (lambda: match(out=None), "null colour row"),
             (lambda: match(gain=0.5), "max_gain"), (lambda: match(N=2, wsb=64 * 13 * 8), "workspace")]
    # what the entry points share goes through each of them that shares it
    for f in (way_in, paste, sums, match):
        calls += [(lambda f=f: f(y=None), "null plane pointer"), (lambda f=f: f(u=None), "null plane pointer"), (lambda f=f: f(v=None), "null plane pointer"),
                  (lambda f=f: f(N=0), "N must"), (lambda f=f: f(N=-3), "N must"), (lambda f=f: f(H=0), "H, W >= 2"), (lambda f=f: f(W=0), "H, W >= 2"),
                  (lambda f=f: f(H=7), "even height and width"), (lambda f=f: f(W=6 + 1, u_row=3, v_row=3), "even height and width"),
                  (lambda f=f: f(y_row=7), "Y row stride 7"), (lambda f=f: f(u_row=3), "U row stride 3"), (lambda f=f: f(v_row=3), "V row stride 3"),
                  (lambda f=f: f(v_row=-4), "V row stride"), (lambda f=f: f(W=2 ** 31 - 2), "Y row stride"),
                  (lambda f=f: f(sim=None), "null transform"), (lambda f=f: f(std=2020), "standard"), (lambda f=f: f(std=0), "standard"),
                  (lambda f=f: f(full=2), "full_range"), (lambda f=f: f(full=-1), "full_range")]
    for f in (paste, sums, match):
        calls += [(lambda f=f: f(src=None), "null frame pointer"), (lambda f=f: f(Hs=0), "source size"), (lambda f=f: f(feather=-1.0), "feather"),
                  (lambda f=f: f(feather=float("nan")), "feather"), (lambda f=f: f(k=0.0), "value range"), (lambda f=f: f(mf=1), "matte_frames")]
    for n, (call, words) in enumerate(calls):
        assert call() < 0 and words in lib.spk_last_error().decode(), (n, words, lib.spk_last_error().decode())


def test_the_table_entry_points_refuse_bad_arguments(pkg):
    lib = pkg._lib.lib()
    buf = np.zeros(8192, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 64
    table, x, sim, out, ws = base, base + 1024, base + 2048, base + 4096, 0x10000000              # a table of 3 entries: [0, 168)
    way_in = lambda table=table, N=3, sim=sim, dst=out, Hout=8, Wout=8, std=601, full=0: \
        lib.spk_frames_i420_to_f32_sim_table(table, N, sim, 0, std, full, dst, Hout, Wout, 1, 1, 1, 0, 0, 0, None)
    paste = lambda src=x, N=3, Hs=4, Ws=4, table=table, sim=sim, feather=0.0, k=127.5, matte=None, mf=0, std=709, full=1: \
        lib.spk_frames_paste_i420_sim_table(src, N, Hs, Ws, table, sim, std, full, feather, -1.0, k, matte, mf, None, None)
    sums = lambda src=x, table=table, N=3, sim=sim, Hs=4, feather=0.0, k=127.5, mf=0, out=out, ws=ws, wsb=3 * 64 * 13 * 8, std=601, full=0: \
        lib.spk_paste_colour_sums_i420_sim_table(src, N, Hs, 4, table, sim, std, full, feather, -1.0, k, None, mf, out, ws, wsb, None)
    match = lambda src=x, table=table, N=3, sim=sim, Hs=4, feather=0.0, k=127.5, mf=0, out=out, ws=ws, gain=2.0, std=601, full=0: \
        lib.spk_paste_colour_match_i420_sim_table(src, N, Hs, 4, table, sim, std, full, feather, -1.0, k, None, mf, gain, 1.0, 16.0, out, ws,
                                                  3 * 64 * 13 * 8, None)
    calls = [(lambda: way_in(dst=None), "null frame pointer"), (lambda: way_in(Hout=0), "output size"), (lambda: way_in(Wout=-1), "output size"),
             (lambda: way_in(dst=table + 160), "overlaps dst"), (lambda: way_in(dst=table - 64, Hout=2 ** 31 - 1, Wout=2 ** 31 - 1), "overlaps dst"),
             (lambda: paste(matte=x, mf=2), "matte_frames"), (lambda: sums(out=None), "null sums"), (lambda: sums(out=out + 4), "aligned"),
             (lambda: sums(wsb=8), "workspace"), (lambda: sums(ws=None), "workspace"), (lambda: sums(out=table + 160), "overlaps the sums"),
             (lambda: sums(ws=table + 8), "overlaps the workspace"), (lambda: match(out=None), "null colour row"), (lambda: match(gain=0.5), "max_gain"),
             (lambda: match(out=table + 164), "overlaps the colour rows"), (lambda: match(ws=table + 160), "overlaps the workspace")]
    for f in (way_in, paste, sums, match):
        calls += [(lambda f=f: f(table=None), "null planar table"), (lambda f=f: f(table=table + 4), "aligned"), (lambda f=f: f(N=0), "N must"),
                  (lambda f=f: f(N=-3), "N must"), (lambda f=f: f(sim=None), "null transform"), (lambda f=f: f(std=2020), "standard"),
                  (lambda f=f: f(full=2), "full_range")]
    for f in (paste, sums, match):
        calls += [(lambda f=f: f(src=None), "null frame pointer"), (lambda f=f: f(Hs=0), "source size"), (lambda f=f: f(feather=-1.0), "feather"),
                  (lambda f=f: f(feather=float("nan")), "feather"), (lambda f=f: f(k=0.0), "value range"), (lambda f=f: f(mf=1), "matte_frames")]
    for n, (call, words) in enumerate(calls):
        assert call() < 0 and words in lib.spk_last_error().decode(), (n, words, lib.spk_last_error().decode())


# ---- IRFD.live ------------------------------------------------------------------------------------------------------------------------
def test_live_takes_i420_and_its_colour_on_the_host():
    """``live`` / ``live_room(pixel_format="i420")`` accept ``standard=`` / ``full_range=`` (they get as far as the photo, which a bare
    ``IRFD`` on the CPU cannot encode) and refuse bad ones, and the names that are not the format's, before they touch it"""
    import model
    m = model.IRFD.__new__(model.IRFD)                                      # no weights: nothing of the model is reached
    photo = torch.zeros(8, 8, 3, dtype=torch.uint8)
    template = [(2.0, 2.0), (6.0, 2.0), (4.0, 6.0)]
    for make, who in ((lambda **kw: m.live(photo, size=8, template=template, **kw), "live"),
                      (lambda **kw: m.live_room([photo], size=8, template=template, **kw), "live_room")):
        for name in ("yuv420", "yuv420p", "I420", "yv12"):
            with pytest.raises(ValueError, match=f"{who}: pixel_format must be 'rgb24' or 'nv12' or 'i420'"):
                make(pixel_format=name)
        with pytest.raises(ValueError, match="standard / full_range apply to pixel_format='nv12' only, and to 'i420'"):
            make(standard="bt709")
        with pytest.raises(ValueError, match="standard must be"):
            make(pixel_format="i420", standard="bt2020")
        with pytest.raises(ValueError, match="full_range must be"):
            make(pixel_format="i420", full_range=2)
        for colour in (dict(), dict(standard="bt709"), dict(full_range=True), dict(standard="bt709", full_range=True)):
            with pytest.raises(Exception) as e:                             # past every host check of the format: the photo is next
                make(pixel_format="i420", **colour)
            assert not isinstance(e.value, ValueError), (who, colour, e.value)
    from importlib import import_module
    live = import_module("speak-hack_amd").live
    assert live._EDGES["i420"] is live._I420Edge and live._I420Edge.table is import_module("speak-hack_amd").ops.PlanarTable


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NS.SPECS))
def test_the_interleave_of_a_case_is_the_nv12_case(pkg, name):
    c, theirs = IC.case(name), NS.case(name)
    y, u, v = c["layout"].planes(c["flats"], 0)
    assert torch.equal(y, theirs["y"]) and torch.equal(IC.interleave(u, v), theirs["uv"])
    assert u.stride() == (583, 29, 1) and v.stride(1) == 32 and u.storage_offset() % 2 == 1
    planes = pkg.ops.i420_planes((y, u, v))
    assert all(a is b for a, b in zip(planes, (y, u, v)))
    assert c["layout"].rest_intact(c["flats"], [torch.full_like(f, 0xA5) for f in c["flats"]])       # guards and padding are 0xA5
    assert all(bool((f[:IC.GUARD] == 0xA5).all()) and bool((f[-IC.GUARD:] == 0xA5).all()) for f in c["flats"])


@pytest.mark.parametrize("name", SC.MIXED)
def test_the_interleave_of_a_mixed_case_is_the_surface_table_case(pkg, name):
    c, theirs = IC.mixed(name), SC.case(name)
    for n in range(len(SC.LAYOUT)):
        y, u, v = c["layout"].planes(c["flats"], n)
        ty, tuv = SC.planes_of(theirs["flats"][n], n)
        assert torch.equal(y, ty) and torch.equal(IC.interleave(u, v), tuv), n
        assert tuple(y.shape) == SC.SIZES[n] and tuple(u.shape) == tuple(v.shape) == (SC.SIZES[n][0] // 2, SC.SIZES[n][1] // 2)
    assert c["layout"].rest_intact(c["flats"], [torch.full_like(f, 0xA5) for f in c["flats"]])
    assert all(bool((f[:IC.GUARD] == 0xA5).all()) and bool((f[-IC.GUARD:] == 0xA5).all()) for f in c["flats"])
