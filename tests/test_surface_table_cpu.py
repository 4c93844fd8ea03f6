"""CPU-side checks of the surface table (csrc/frame_table_nv12.hip, ``ops.SurfaceTable``): ``spk_surface_table_check`` through ctypes
on host tables packed with numpy -- the tables that must pass, each refusal and the entry (or pair of planes) it names, overlap
refused only where the surfaces are written, extents that leave 64 bits -- the 40-byte layout of ``spk_surface_ref`` against
include/spk.h, the ``ValueError``s of ``ops.SurfaceTable`` (raised before a device is touched), the argument refusals of the four
``_nv12_sim_table`` entry points (which return before a launch, so no GPU is needed), and the host refusals of
``IRFD.live(pixel_format=)``."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = np.dtype([("y", "<u8"), ("uv", "<u8"), ("y_row_stride", "<i8"), ("uv_row_stride", "<i8"), ("H", "<i4"), ("W", "<i4")])
BASE = 0x7000_0000_0000                                                     # addresses are numbers here: the check never follows them
ZERO = (0, 0, 0, 0, 0, 0)


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
    rc = lib.spk_surface_table_check(table.ctypes.data if table is not None else None, len(table) if N is None else N, written)
    return rc, lib.spk_last_error().decode()


# entry 0: 4 x 6 at pitch 16, Y [0, 54), UV two rows at pitch 8 in [54, 68);  entry 1: 2 x 2 packed, Y [68, 72), UV [72, 74);
# entry 2: absent;  entry 3: 6 x 4, Y and UV in separate allocations far apart, Y [4096, 4120), UV three rows at pitch 6
GOOD = [(BASE, BASE + 54, 16, 8, 4, 6), (BASE + 68, BASE + 72, 2, 2, 2, 2), ZERO, (BASE + 4096, BASE + 2 ** 32, 4, 6, 6, 4)]


def edited(n, **fields):
    e = [list(g) for g in GOOD]
    for k, v in fields.items():
        e[n][REF.names.index(k)] = v
    return packed([tuple(g) for g in e])


def test_the_layout_is_the_header_s(pkg):
    F = pkg._lib.SurfaceRef
    assert ctypes.sizeof(F) == 40 == REF.itemsize and ctypes.alignment(F) == 8
    assert [(n, getattr(F, n).offset, getattr(F, n).size) for n, _ in F._fields_] == \
        [("y", 0, 8), ("uv", 8, 8), ("y_row_stride", 16, 8), ("uv_row_stride", 24, 8), ("H", 32, 4), ("W", 36, 4)]
    assert [REF.fields[n][1] for n in REF.names] == [0, 8, 16, 24, 32, 36]
    header = open(os.path.join(ROOT, "include", "spk.h")).read()
    m = re.search(r"typedef struct spk_surface_ref \{([^}]*)\} spk_surface_ref;", header)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == \
        "const uint8_t* y; const uint8_t* uv; int64_t y_row_stride; int64_t uv_row_stride; int32_t H, W;"


def test_tables_that_pass(pkg):
    for written in (0, 1):
        assert check(pkg, packed(GOOD), written)[0] == 0                    # [0, 54) [54, 68) [68, 72) [72, 74) touch: apart
        assert check(pkg, packed([ZERO] * 3), written)[0] == 0              # every surface absent
        assert check(pkg, packed(GOOD[::-1]), written)[0] == 0              # entries out of address order
        assert check(pkg, edited(0, y_row_stride=6, uv_row_stride=6), written)[0] == 0                # the smallest strides
        assert check(pkg, edited(3, uv=BASE + 74), written)[0] == 0         # UV of 3 right behind UV of 1
        assert check(pkg, edited(0, uv=BASE + 2 ** 40), written)[0] == 0    # Y and UV in separate allocations
    assert check(pkg, edited(1, y_row_stride=2 ** 62, uv_row_stride=2 ** 63 - 1 - 1), 0)[0] == 0     # one UV row: its stride does not count


def test_refusals_name_the_entry(pkg):
    assert check(pkg, None, 0, N=4)[0] < 0 and "null" in pkg._lib.lib().spk_last_error().decode()
    for N in (0, -2):
        rc, msg = check(pkg, packed(GOOD), 0, N=N)
        assert rc < 0 and "N must" in msg
    half = [(0, dict(y=0)), (0, dict(uv=0)), (1, dict(H=0)), (1, dict(H=3)), (3, dict(H=-2)), (0, dict(W=5)), (0, dict(W=0)), (3, dict(W=1)),
            (0, dict(y_row_stride=5)), (0, dict(y_row_stride=-16)), (0, dict(uv_row_stride=4)), (0, dict(uv_row_stride=7)), (0, dict(uv=BASE + 55)),
            (2, dict(y=BASE + 512)), (2, dict(uv_row_stride=8)), (2, dict(H=2)), (2, dict(W=2)),
            (0, dict(y_row_stride=0, uv_row_stride=0, H=0, W=0))]
    for n, fields in half:
        for written in (0, 1):
            rc, msg = check(pkg, edited(n, **fields), written)
            assert rc < 0 and f"entry {n} is half-formed" in msg and "row strides" in msg, (n, fields, msg)


def test_extents_that_leave_64_bits_are_refused(pkg):
    wraps = [(0, dict(y_row_stride=2 ** 62), "Y"), (0, dict(H=2 ** 31 - 2, y_row_stride=2 ** 33), "Y"), (0, dict(uv_row_stride=2 ** 63 - 2), "UV"),
             (3, dict(uv_row_stride=2 ** 62), "UV"), (1, dict(y=2 ** 64 - 3), "Y"), (1, dict(uv=2 ** 64 - 2), "UV"),
             (3, dict(y=2 ** 64 - 16), "Y")]
    for n, fields, plane in wraps:
        rc, msg = check(pkg, edited(n, **fields), 0)
        assert rc < 0 and f"entry {n}: the {plane} extent" in msg and "overflows 64 bits" in msg, (n, fields, msg)


def test_overlap_is_refused_only_where_the_surfaces_are_written(pkg):
    cases = [(edited(1, y=BASE + 53), "entries 0 (Y) and 1 (Y) overlap"),                  # the last byte of Y of entry 0
             (edited(1, y=BASE + 66), "entries 0 (UV) and 1 (Y) overlap"),                 # Y of one entry against UV of another
             (edited(1, uv=BASE + 20), "entries 0 (Y) and 1 (UV) overlap"),                # inside the padding columns of Y 0: its byte RANGE
             (edited(0, uv=BASE + 52), "entries 0 (Y) and 0 (UV) overlap"),                # an entry's own two planes
             (edited(0, uv=BASE), "entries 0 (Y) and 0 (UV) overlap"),
             (edited(3, y=BASE + 72, uv=BASE + 4096), "entries 1 (UV) and 3 (Y) overlap"),
             (edited(2, y=BASE + 68, uv=BASE + 72, y_row_stride=2, uv_row_stride=2, H=2, W=2), "entries 1 (Y) and 2 (Y) overlap"),   # twice
             (packed([GOOD[3], GOOD[1], ZERO, (BASE + 40, BASE + 8192, 16, 8, 4, 6)]), "entries 1 (Y) and 3 (Y) overlap")]
    for table, words in cases:
        assert check(pkg, table, 0)[0] == 0, words
        rc, msg = check(pkg, table, 1)
        assert rc < 0 and words in msg, (words, msg)


def test_surface_table_value_errors_come_before_a_device(pkg):
    T = pkg.ops.SurfaceTable
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)
    ok = u8(6, 6)                                                           # 4 x 6
    bad = {"not a sequence": 7, "empty": [], "a 4-d tensor": u8(1, 2, 6, 6), "no frames": u8(0, 6, 6), "a string": [ok, "surface"],
           "a number": [ok, 3], "float": [ok, ok.float()], "int8": [ok.to(torch.int8)], "an odd H": [u8(8, 6)], "an odd W": [u8(6, 5)],
           "rows not 3H/2": [u8(7, 6)], "wrong rank": [u8(1, 1, 6, 6)], "a 3-d element": [u8(2, 6, 6)], "a pixel stride": [u8(6, 12)[:, ::2]],
           "an odd pitch": [u8(6, 7)[:, :6]], "a float pair": [(u8(4, 6), torch.zeros(2, 3, 2))], "a pair of the wrong size": [(u8(4, 6), u8(2, 2, 2))],
           "an odd pair": [(u8(3, 6), u8(1, 3, 2))], "a UV pair not packed": [(u8(4, 6), u8(2, 3, 4)[:, :, ::2])],
           "UV pairs apart": [(u8(4, 6), u8(2, 6, 2)[:, ::2])], "Y pixels apart": [(u8(4, 12)[:, ::2], u8(2, 3, 2))],
           "a bad surface behind a good one": [ok, u8(6, 12)[:, ::2]], "a tensor of odd surfaces": u8(2, 7, 6)}
    for name, surfaces in bad.items():
        with pytest.raises(ValueError, match="SurfaceTable|nv12"):
            T(surfaces)
    # what has the right shape and strides gets as far as the device check: a surface, a pitched one, a region of interest at even
    # offsets as a pair of views, an absent one, a tensor of surfaces and a pair of planes
    wide = u8(12, 16)                                                       # 8 x 16
    roi = (wide[2:6, 4:10], wide[8:][1:3, 4:10].unflatten(1, (3, 2)))
    for surfaces in ([ok], [u8(6, 8)[:, :6]], [roi], [None, ok], u8(2, 6, 6), (u8(2, 4, 6), u8(2, 2, 3, 2)), [(u8(4, 6), u8(2, 3, 2))]):
        with pytest.raises(pkg._lib.SpkError, match="no CPU path"):
            T(surfaces)


def test_the_table_entry_points_refuse_bad_arguments(pkg):
    lib = pkg._lib.lib()
    buf = np.zeros(8192, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 64
    table, x, sim, out, ws = base, base + 1024, base + 2048, base + 4096, 0x10000000
    way_in = lambda table=table, N=3, sim=sim, dst=out, Hout=8, Wout=8, std=601, full=0: \
        lib.spk_frames_nv12_to_f32_sim_table(table, N, sim, 0, std, full, dst, Hout, Wout, 1, 1, 1, 0, 0, 0, None)
    paste = lambda src=x, N=3, Hs=4, Ws=4, table=table, sim=sim, feather=0.0, k=127.5, matte=None, mf=0, std=709, full=1: \
        lib.spk_frames_paste_nv12_sim_table(src, N, Hs, Ws, table, sim, std, full, feather, -1.0, k, matte, mf, None, None)
    sums = lambda src=x, table=table, N=3, sim=sim, Hs=4, feather=0.0, k=127.5, mf=0, out=out, ws=ws, wsb=3 * 64 * 13 * 8, std=601, full=0: \
        lib.spk_paste_colour_sums_nv12_sim_table(src, N, Hs, 4, table, sim, std, full, feather, -1.0, k, None, mf, out, ws, wsb, None)
    match = lambda src=x, table=table, N=3, sim=sim, Hs=4, feather=0.0, k=127.5, mf=0, out=out, ws=ws, gain=2.0, std=601, full=0: \
        lib.spk_paste_colour_match_nv12_sim_table(src, N, Hs, 4, table, sim, std, full, feather, -1.0, k, None, mf, gain, 1.0, 16.0, out, ws,
                                                  3 * 64 * 13 * 8, None)
    calls = [(lambda: way_in(dst=None), "null frame pointer"), (lambda: way_in(Hout=0), "output size"), (lambda: way_in(Wout=-1), "output size"),
             (lambda: way_in(dst=table + 64), "overlaps dst"), (lambda: way_in(dst=table - 64, Hout=2 ** 31 - 1, Wout=2 ** 31 - 1), "overlaps dst"),
             (lambda: paste(matte=x, mf=2), "matte_frames"), (lambda: sums(out=None), "null sums"), (lambda: sums(out=out + 4), "aligned"),
             (lambda: sums(wsb=8), "workspace"), (lambda: sums(ws=None), "workspace"), (lambda: sums(out=table + 64), "overlaps the sums"),
             (lambda: sums(ws=table + 8), "overlaps the workspace"), (lambda: match(out=None), "null colour row"), (lambda: match(gain=0.5), "max_gain"),
             (lambda: match(out=table + 68), "overlaps the colour rows"), (lambda: match(ws=table + 64), "overlaps the workspace")]
    # what the entry points share goes through each of them that shares it
    for f in (way_in, paste, sums, match):
        calls += [(lambda f=f: f(table=None), "null surface table"), (lambda f=f: f(table=table + 4), "aligned"), (lambda f=f: f(N=0), "N must"),
                  (lambda f=f: f(N=-3), "N must"), (lambda f=f: f(sim=None), "null transform"), (lambda f=f: f(std=2020), "standard"),
                  (lambda f=f: f(full=2), "full_range")]
    for f in (paste, sums, match):
        calls += [(lambda f=f: f(src=None), "null frame pointer"), (lambda f=f: f(Hs=0), "source size"), (lambda f=f: f(feather=-1.0), "feather"),
                  (lambda f=f: f(feather=float("nan")), "feather"), (lambda f=f: f(k=0.0), "value range"), (lambda f=f: f(mf=1), "matte_frames")]
    for n, (call, words) in enumerate(calls):
        assert call() < 0 and words in lib.spk_last_error().decode(), (n, words, lib.spk_last_error().decode())


def test_live_refuses_a_pixel_format_on_the_host():
    """``live`` / ``live_room`` check ``pixel_format``, ``standard`` and ``full_range`` before they touch the photo or the networks: a
    bare ``IRFD`` on the CPU and a CPU photo get as far as the refusal"""
    import model
    m = model.IRFD.__new__(model.IRFD)                                      # no weights: nothing of the model is reached
    photo = torch.zeros(8, 8, 3, dtype=torch.uint8)
    template = [(2.0, 2.0), (6.0, 2.0), (4.0, 6.0)]
    for make, who in ((lambda **kw: m.live(photo, size=8, template=template, **kw), "live"),
                      (lambda **kw: m.live_room([photo], size=8, template=template, **kw), "live_room")):
        with pytest.raises(ValueError, match=f"{who}: pixel_format must be 'rgb24' or 'nv12'"):
            make(pixel_format="yuv420")
        with pytest.raises(ValueError, match="standard / full_range apply to pixel_format='nv12' only"):
            make(standard="bt709")
        with pytest.raises(ValueError, match="standard / full_range apply to pixel_format='nv12' only"):
            make(full_range=True)
        with pytest.raises(ValueError, match="standard must be"):
            make(pixel_format="nv12", standard="bt2020")
        with pytest.raises(ValueError, match="full_range must be"):
            make(pixel_format="nv12", full_range=2)
