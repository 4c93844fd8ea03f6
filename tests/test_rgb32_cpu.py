"""CPU-side checks of the aligned RGB32 edge (csrc/frame_sim_rgb32.hip, csrc/frame_table_rgb32.hip): the argument refusals of the
ten entry points through ctypes (they return before a launch and before anything is dereferenced, so no GPU is needed) -- null
pointers, a row stride below 4 W or not a multiple of 4, a misaligned base, ``alpha_first`` outside {0, 1} -- and
``spk_frame_table_check_rgb32`` on host tables packed with numpy: the tables that must pass (touching ranges, every entry absent, a
view at a pixel offset, separate allocations), half-formed entries (a misaligned one included), extents that leave 64 bits, overlap
refused only where the frames are written; the ``ValueError``s of ``ops.Rgb32Table`` and of the launchers (raised before a device is
touched); the host refusals of ``IRFD.live(pixel_format="rgb32")``; the three refusals of the rgb24 edge that must stay; and the
cases of tests/rgb32_cases.py against the packed cases they came from."""
import importlib

import numpy as np
import pytest
import torch

import blend_cases as BC
import frame_table_cases as FC
import rgb32_cases as RC

REF = np.dtype([("data", "<u8"), ("row_stride", "<i8"), ("H", "<i4"), ("W", "<i4")])
BASE = 0x7000_0000_0000                                                     # addresses are numbers here: the check never follows them
ZERO = (0, 0, 0, 0)
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
    rc = lib.spk_frame_table_check_rgb32(table.ctypes.data if table is not None else None, len(table) if N is None else N, written)
    return rc, lib.spk_last_error().decode()


# entry 0: 4 x 6 at pitch 32: [0, 120).  entry 1: 2 x 2 packed, [120, 136): it TOUCHES entry 0.  entry 2: absent.  entry 3: a 3 x 5
# view at pixel offset (1, 2) of a 6 x 8 surface at pitch 48 that begins at 4096: [4152, 4268), 4-aligned and not 16-aligned.
# entry 4: 1 x 1 in an allocation far away
GOOD = [(BASE, 32, 4, 6), (BASE + 120, 8, 2, 2), ZERO, (BASE + 4096 + 48 + 8, 48, 3, 5), (BASE + 2 ** 33, 4, 1, 1)]


def edited(n, **fields):
    e = [list(g) for g in GOOD]
    for k, v in fields.items():
        e[n][REF.names.index(k)] = v
    return packed([tuple(g) for g in e])


# ---- spk_frame_table_check_rgb32 ----------------------------------------------------------------------------------------------------
def test_the_entries_are_the_frame_table_s(pkg):
    assert REF.itemsize == 24 == importlib.import_module("ctypes").sizeof(pkg._lib.FrameRef)


def test_tables_that_pass(pkg):
    assert (GOOD[3][0] - BASE) % 16 == 8 and GOOD[0][0] + 3 * 32 + 24 == GOOD[1][0]
    for written in (0, 1):
        assert check(pkg, packed(GOOD), written)[0] == 0                    # ranges that touch, a view at a pixel offset, separate allocations
        assert check(pkg, packed([ZERO] * 3), written)[0] == 0              # every entry absent
        assert check(pkg, packed(GOOD[::-1]), written)[0] == 0              # entries out of address order
        assert check(pkg, edited(0, row_stride=24), written)[0] == 0        # the smallest stride
        assert check(pkg, edited(4, data=BASE + 136), written)[0] == 0      # right behind entry 1
    assert check(pkg, edited(4, row_stride=2 ** 62), 1)[0] == 0             # one row: its stride does not count
    assert check(pkg, edited(1, data=BASE + 60), 0)[0] == 0                 # overlap is tolerated where the frames are only read


def test_refusals_name_the_entry(pkg):
    assert check(pkg, None, 0, N=4)[0] < 0 and "null" in pkg._lib.lib().spk_last_error().decode()
    for N in (0, -2):
        rc, msg = check(pkg, packed(GOOD), 0, N=N)
        assert rc < 0 and "N must" in msg
    half = [(0, dict(data=0)), (1, dict(H=0)), (3, dict(H=-2)), (0, dict(W=0)), (0, dict(W=-1)), (0, dict(row_stride=23)),       # < 4 W
            (0, dict(row_stride=20)), (0, dict(row_stride=-32)), (0, dict(row_stride=26)), (0, dict(row_stride=33)),             # % 4
            (0, dict(data=BASE + 1)), (1, dict(data=BASE + 122)), (3, dict(data=BASE + 4096 + 3)),                                # data % 4
            (2, dict(data=BASE + 512)), (2, dict(row_stride=8)), (2, dict(H=2)), (2, dict(W=2)), (0, dict(row_stride=0, H=0, W=0))]
    for n, fields in half:
        for written in (0, 1):
            rc, msg = check(pkg, edited(n, **fields), written)
            assert rc < 0 and f"entry {n} is half-formed" in msg and "multiple of 4" in msg, (n, fields, msg)


def test_extents_that_leave_64_bits_are_refused(pkg):
    wraps = [(0, dict(row_stride=2 ** 62)), (0, dict(H=2 ** 31 - 2, row_stride=2 ** 33)), (1, dict(data=2 ** 64 - 8)), (4, dict(data=2 ** 64 - 4))]
    for n, fields in wraps:
        rc, msg = check(pkg, edited(n, **fields), 0)
        assert rc < 0 and f"entry {n}: the extent" in msg and "overflows 64 bits" in msg, (n, fields, msg)


def test_overlap_is_refused_only_where_the_frames_are_written(pkg):
    cases = [(edited(1, data=BASE + 116), "entries 0 (RGB32) and 1 (RGB32) overlap"),      # the last pixel of entry 0
             (edited(1, data=BASE + 28), "entries 0 (RGB32) and 1 (RGB32) overlap"),       # inside the pitch padding of entry 0: its byte RANGE
             (edited(4, data=BASE + 4096 + 48 * 3 + 24), "entries 3 (RGB32) and 4 (RGB32) overlap"),
             (packed([GOOD[0], GOOD[1], GOOD[1]]), "entries 1 (RGB32) and 2 (RGB32) overlap")]       # twice
    for table, words in cases:
        assert check(pkg, table, 0)[0] == 0, words
        rc, msg = check(pkg, table, 1)
        assert rc < 0 and words in msg, (words, msg)


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
def test_the_strided_entry_points_refuse_bad_arguments(pkg):
    lib = pkg._lib.lib()
    buf = np.zeros(8192, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 64
    x, sim, out, ws = base + 1024, base + 2048, base + 4096, 0x10000000
    ok = dict(p=base, img=256, row=32, N=1, H=8, W=8, sim=sim, swap=0, af=0)

    def way_in(dst=out, Hout=4, Wout=4, **kw):
        a = dict(ok, **kw)
        return lib.spk_frames_rgb32_to_f32_sim(a["p"], a["img"], a["row"], a["N"], a["H"], a["W"], a["sim"], a["swap"], a["af"], dst, Hout, Wout,
                                               1, 1, 1, 0, 0, 0, None)

    def head(a, src, Hs):
        return (src, a["N"], Hs, 4, a["p"], a["img"], a["row"], a["H"], a["W"], a["sim"], a["swap"], a["af"])

    def paste(src=x, Hs=4, feather=0.0, k=127.5, **kw):
        return lib.spk_frames_paste_rgb32_sim(*head(dict(ok, **kw), src, Hs), feather, -1.0, k, None)

    def blend(src=x, Hs=4, feather=0.0, k=127.5, matte=None, mf=0, **kw):
        return lib.spk_frames_paste_rgb32_sim_blend(*head(dict(ok, **kw), src, Hs), feather, -1.0, k, matte, mf, None, None)

    def sums(src=x, Hs=4, feather=0.0, k=127.5, matte=None, mf=0, out=out, ws=ws, wsb=2 * 64 * 13 * 8, **kw):
        return lib.spk_paste_colour_sums_rgb32_sim(*head(dict(ok, **kw), src, Hs), feather, -1.0, k, matte, mf, out, ws, wsb, None)

    def match(src=x, Hs=4, feather=0.0, k=127.5, matte=None, mf=0, out=out, ws=ws, wsb=2 * 64 * 13 * 8, gain=2.0, **kw):
        return lib.spk_paste_colour_match_rgb32_sim(*head(dict(ok, **kw), src, Hs), feather, -1.0, k, matte, mf, gain, 1.0, 16.0, out, ws, wsb, None)

    calls = [(lambda: way_in(dst=None), "null frame pointer"), (lambda: way_in(Hout=0), "N / H / W"), (lambda: way_in(Wout=-1), "N / H / W"),
             (lambda: way_in(N=2, img=-256), "negative image stride"), (lambda: paste(N=2, img=7 * 32 + 28), "overlap"),
             (lambda: blend(N=2, img=0), "overlap"), (lambda: sums(N=2, img=-256), "overlap"),
             (lambda: blend(matte=x, mf=2), "matte_frames"), (lambda: sums(out=None), "null sums"), (lambda: sums(out=out + 4), "aligned"),
             (lambda: sums(wsb=8), "workspace"), (lambda: sums(ws=None), "workspace"), (lambda: match(out=None), "null colour row"),
             (lambda: match(gain=0.5), "max_gain"), (lambda: match(N=2, wsb=64 * 13 * 8), "workspace")]
    # what the entry points share goes through each of them
    for f in (way_in, paste, blend, sums, match):
        calls += [(lambda f=f: f(p=None), "null frame pointer"), (lambda f=f: f(sim=None), "null transform"), (lambda f=f: f(N=0), "N / H / W"),
                  (lambda f=f: f(H=0), "N / H / W"), (lambda f=f: f(W=-1), "N / H / W"),
                  (lambda f=f: f(row=31), "smaller than 4 * W"), (lambda f=f: f(row=24), "smaller than 4 * W"), (lambda f=f: f(row=-32), "smaller than 4 * W"),
                  (lambda f=f: f(W=2 ** 31 - 1), "smaller than 4 * W"),
                  (lambda f=f: f(row=34), "row stride 34 is not a multiple of 4"), (lambda f=f: f(row=33), "row stride 33 is not a multiple of 4"),
                  (lambda f=f: f(N=2, img=258), "image stride 258 is not a multiple of 4"),
                  (lambda f=f: f(p=base + 1), "aligned to 4 bytes"), (lambda f=f: f(p=base + 2), "aligned to 4 bytes"), (lambda f=f: f(p=base + 7), "aligned to 4 bytes"),
                  (lambda f=f: f(af=2), "alpha_first"), (lambda f=f: f(af=-1), "alpha_first")]
    for f in (paste, blend, sums, match):
        calls += [(lambda f=f: f(src=None), "null frame pointer"), (lambda f=f: f(Hs=0), "N / H / W"), (lambda f=f: f(feather=-1.0), "feather"),
                  (lambda f=f: f(feather=float("nan")), "feather"), (lambda f=f: f(k=0.0), "value range")]
    for f in (blend, sums, match):
        calls += [(lambda f=f: f(mf=1), "matte_frames")]
    for n, (call, words) in enumerate(calls):
        assert call() < 0 and words in lib.spk_last_error().decode(), (n, words, lib.spk_last_error().decode())


def test_the_table_entry_points_refuse_bad_arguments(pkg):
    lib = pkg._lib.lib()
    buf = np.zeros(8192, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 64
    table, x, sim, out, ws = base, base + 1024, base + 2048, base + 4096, 0x10000000              # a table of 3 entries: [0, 72)
    way_in = lambda table=table, N=3, sim=sim, dst=out, Hout=8, Wout=8, af=0: \
        lib.spk_frames_rgb32_to_f32_sim_table(table, N, sim, 0, af, dst, Hout, Wout, 1, 1, 1, 0, 0, 0, None)
    paste = lambda src=x, N=3, Hs=4, Ws=4, table=table, sim=sim, feather=0.0, k=127.5, matte=None, mf=0, af=1: \
        lib.spk_frames_paste_rgb32_sim_table(src, N, Hs, Ws, table, sim, 1, af, feather, -1.0, k, matte, mf, None, None)
    sums = lambda src=x, table=table, N=3, sim=sim, Hs=4, feather=0.0, k=127.5, mf=0, out=out, ws=ws, wsb=3 * 64 * 13 * 8, af=0: \
        lib.spk_paste_colour_sums_rgb32_sim_table(src, N, Hs, 4, table, sim, 0, af, feather, -1.0, k, None, mf, out, ws, wsb, None)
    match = lambda src=x, table=table, N=3, sim=sim, Hs=4, feather=0.0, k=127.5, mf=0, out=out, ws=ws, gain=2.0, af=0: \
        lib.spk_paste_colour_match_rgb32_sim_table(src, N, Hs, 4, table, sim, 0, af, feather, -1.0, k, None, mf, gain, 1.0, 16.0, out, ws,
                                                   3 * 64 * 13 * 8, None)
    calls = [(lambda: way_in(dst=None), "null frame pointer"), (lambda: way_in(Hout=0), "output size"), (lambda: way_in(Wout=-1), "output size"),
             (lambda: way_in(dst=table + 64), "overlaps dst"), (lambda: way_in(dst=table - 64, Hout=2 ** 31 - 1, Wout=2 ** 31 - 1), "overlaps dst"),
             (lambda: paste(matte=x, mf=2), "matte_frames"), (lambda: sums(out=None), "null sums"), (lambda: sums(out=out + 4), "aligned"),
             (lambda: sums(wsb=8), "workspace"), (lambda: sums(ws=None), "workspace"), (lambda: sums(out=table + 64), "overlaps the sums"),
             (lambda: sums(ws=table + 8), "overlaps the workspace"), (lambda: match(out=None), "null colour row"), (lambda: match(gain=0.5), "max_gain"),
             (lambda: match(out=table + 68), "overlaps the colour rows"), (lambda: match(ws=table + 64), "overlaps the workspace")]
    for f in (way_in, paste, sums, match):
        calls += [(lambda f=f: f(table=None), "null frame table"), (lambda f=f: f(table=table + 4), "aligned"), (lambda f=f: f(N=0), "N must"),
                  (lambda f=f: f(N=-3), "N must"), (lambda f=f: f(sim=None), "null transform"), (lambda f=f: f(af=2), "alpha_first"),
                  (lambda f=f: f(af=-1), "alpha_first")]
    for f in (paste, sums, match):
        calls += [(lambda f=f: f(src=None), "null frame pointer"), (lambda f=f: f(Hs=0), "source size"), (lambda f=f: f(feather=-1.0), "feather"),
                  (lambda f=f: f(feather=float("nan")), "feather"), (lambda f=f: f(k=0.0), "value range"), (lambda f=f: f(mf=1), "matte_frames")]
    for n, (call, words) in enumerate(calls):
        assert call() < 0 and words in lib.spk_last_error().decode(), (n, words, lib.spk_last_error().decode())


# ---- ops.Rgb32Table and the launchers -----------------------------------------------------------------------------------------------
def test_rgb32_table_value_errors_come_before_a_device(pkg, monkeypatch):
    T = pkg.ops.Rgb32Table
    copies = []
    monkeypatch.setattr(torch.Tensor, "copy_", lambda self, *a, **k: copies.append(self) or self)      # a refused call copies nothing
    ok = u8(4, 6, 4)
    bad = {"not a sequence": 7, "empty": [], "a 3-d tensor": u8(2, 6, 4), "no frames": u8(0, 4, 6, 4), "a string": [ok, "frame"], "a number": [ok, 3],
           "float": [ok, ok.float()], "int8": [ok.to(torch.int8)], "three channels": [u8(4, 6, 3)], "a packed tensor": u8(2, 4, 6, 3), "wrong rank": [u8(1, 4, 6, 4)],
           "no rows": [u8(0, 6, 4)], "pixels apart": [u8(4, 12, 4)[:, ::2]], "bytes apart": [u8(4, 6, 8)[:, :, ::2]], "rows that overlap": [u8(1, 6, 4).expand(4, 6, 4)],
           "a pitch that is no multiple of 4": [u8(4, 26)[:, :24].unflatten(1, (6, 4))], "a misaligned base": [u8(4 * 6 * 4 + 1)[1:].view(4, 6, 4)],
           "a colour slice of five channels": [u8(4, 6, 5)[..., :4]], "a bad frame behind a good one": [ok, None, u8(4, 6, 3)]}
    for name, frames in bad.items():
        with pytest.raises(ValueError, match="Rgb32Table"):
            T(frames)
    # what has the right shape and strides gets as far as the device check: a frame, a view at a pixel offset, an absent one, a tensor
    wide = u8(8, 16, 4)
    for frames in ([ok], [wide[2:6, 5:12]], [None, ok], u8(2, 4, 6, 4), [ok, wide[1:, 3:], None]):
        with pytest.raises(pkg._lib.SpkError, match="no CPU path"):
            T(frames)
    assert not copies


def test_launcher_value_errors(pkg):
    ops = pkg.ops
    x, rows, frames = torch.zeros(2, 3, 8, 8), [[1.0, 0.0, 0.0, 0.0]] * 2, u8(2, 16, 16, 4)
    for order in ("rgb", "bgr", "RGBA", "rgbx", "bgr0", "", None, 3):
        for call in (lambda: ops.frames_from_rgb32_aligned(frames, 8, rows, channel_order=order),
                     lambda: ops.frames_paste_rgb32_aligned(x, frames, rows, channel_order=order),
                     lambda: ops.paste_colour_sums_rgb32(x, frames, rows, channel_order=order),
                     lambda: ops.paste_colour_match_rgb32(x, frames, rows, channel_order=order)):
            with pytest.raises(ValueError, match="channel_order must be one of 'rgba', 'bgra', 'argb', 'abgr'"):
                call()
    assert [pkg.frames.rgb32_order(o) for o in RC.ORDERS] == [("rgb", 0), ("bgr", 0), ("rgb", 1), ("bgr", 1)]
    for bad in (u8(2, 16, 16, 3), u8(16, 16), u8(3, 16, 16, 4), "frames", pkg.ops.FrameTable):
        with pytest.raises(ValueError, match="frames must be"):
            ops.frames_paste_rgb32_aligned(x, bad, rows)
    with pytest.raises(ValueError, match="frames must be"):
        ops.frames_from_rgb32_aligned(u8(2, 16, 16, 3), 8, rows)
    with pytest.raises(ValueError, match="not a valid transform"):
        ops.frames_from_rgb32_aligned(frames, 8, [[0.0, 0.0, 0.0, 0.0]] * 2)
    with pytest.raises(pkg._lib.SpkError, match="no CPU path"):             # past every host check: the device is next
        ops.frames_from_rgb32_aligned(frames, 8, rows)
    # what rgb32_pixels asks of frames that are written
    P = pkg.frames.rgb32_pixels
    assert P(frames) and P(u8(2, 16, 20, 4)[:, 2:, 3:19]) and P(u8(1, 4, 6, 4)[:, :, 1:])
    assert not P(u8(2, 16, 32, 4)[:, :, ::2]) and not P(u8(2, 16, 66)[:, :, :64].unflatten(2, (16, 4))) and not P(u8(1, 16, 16, 4).expand(2, 16, 16, 4))
    assert not P(u8(2 * 16 * 16 * 4 + 2)[2:].view(2, 16, 16, 4)) and not P(u8(2, 16 * 16 * 4 + 2)[:, :-2].view(2, 16, 16, 4))


def test_the_rgb24_edge_refuses_what_it_refused(pkg):
    ops = pkg.ops
    x, rows = torch.zeros(2, 3, 8, 8), [[1.0, 0.0, 0.0, 0.0]] * 2
    with pytest.raises(ValueError, match="channel_order must be 'rgb' or 'bgr'"):
        ops.frames_to_u8(x, channel_order="bgra")
    with pytest.raises(ValueError, match="pixels must be packed"):
        ops.FrameTable([u8(4, 6, 4)[:, :, :3]])
    for call in (lambda: ops.frames_from_u8_aligned(u8(2, 16, 16, 4), 8, rows), lambda: ops.frames_paste_u8_aligned(x, u8(2, 16, 16, 4), rows),
                 lambda: ops.paste_colour_sums(x, u8(2, 16, 16, 4), rows), lambda: ops.paste_colour_match(x, u8(2, 16, 16, 4), rows)):
        with pytest.raises(ValueError, match=r"frames must be \[(N|2),H,W,3\]"):
            call()
    assert not pkg.frames.packed_pixels(u8(2, 16, 16, 4)[..., :3])


# ---- IRFD.live ----------------------------------------------------------------------------------------------------------------------
def test_live_takes_rgb32_and_its_orders_on_the_host():
    """``live`` / ``live_room(pixel_format="rgb32")`` accept the four orders (they get as far as the photo, which a bare ``IRFD`` on the
    CPU cannot encode) and refuse every other order, ``standard`` / ``full_range``, and names that are not the format's"""
    import model
    m = model.IRFD.__new__(model.IRFD)                                      # no weights: nothing of the model is reached
    photo = torch.zeros(8, 8, 3, dtype=torch.uint8)
    template = [(2.0, 2.0), (6.0, 2.0), (4.0, 6.0)]
    for make, who in ((lambda **kw: m.live(photo, size=8, template=template, **kw), "live"),
                      (lambda **kw: m.live_room([photo], size=8, template=template, **kw), "live_room")):
        for name in ("rgba", "bgra", "rgb32 ", "RGB32", "argb32"):
            with pytest.raises(ValueError, match=f"{who}: pixel_format must be 'rgb24' or 'nv12' or 'i420' or 'rgb32'"):
                make(pixel_format=name)
        for order in ("rgb", "bgr", "rgbx", "BGRA"):
            with pytest.raises(ValueError, match="channel_order must be one of 'rgba'"):
                make(pixel_format="rgb32", channel_order=order)
        with pytest.raises(ValueError, match="channel_order must be 'rgb' or 'bgr'"):
            make(channel_order="bgra")                                     # the order of another format
        for colour in (dict(standard="bt709"), dict(full_range=True)):
            with pytest.raises(ValueError, match="standard / full_range apply to pixel_format='nv12' only, and to 'i420'"):
                make(pixel_format="rgb32", channel_order="bgra", **colour)
        for order in RC.ORDERS:
            with pytest.raises(Exception) as e:                             # past every host check of the format: the photo is next
                make(pixel_format="rgb32", channel_order=order)
            assert not isinstance(e.value, ValueError), (who, order, e.value)
        with pytest.raises(ValueError, match=r"must be \[H,W,3\]"):         # the identity photo stays a packed photo
            (m.live if who == "live" else lambda p, **kw: m.live_room([p], **kw))(torch.zeros(8, 8, 4, dtype=torch.uint8), size=8, template=template,
                                                                                  pixel_format="rgb32", channel_order="bgra")
    live, ops = importlib.import_module("speak-hack_amd").live, importlib.import_module("speak-hack_amd").ops
    assert live._EDGES["rgb32"] is live._Rgb32Edge and live._Rgb32Edge.table is ops.Rgb32Table and live._Rgb32Edge.channels == 4
    assert live._Rgb24Edge.table is ops.FrameTable and live._Rgb24Edge.channels == 3
    edge = live._Rgb32Edge("abgr", "bt601", False)
    assert edge.args == dict(channel_order="abgr") and not edge.surfaces
    with pytest.raises(pkg_error(), match="aligned 32-bit words"):
        edge.writable("live.step", u8(2 * 8 * 8 * 4 + 1)[1:].view(2, 8, 8, 4))
    edge.writable("live.step", u8(2, 8, 12, 4)[:, :, 3:11])


def pkg_error():
    return importlib.import_module("speak-hack_amd")._lib.SpkError


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", RC.ORDERS)
def test_a_case_stripped_of_its_fourth_byte_is_the_packed_case(order):
    rgb, first, fourth = RC.colour_of(order)
    assert rgb == ("rgb" if "rgb" in order else "bgr") and (first, fourth) == ((1, 0) if order[0] == "a" else (0, 3))
    for name in RC.NAMES:
        c, theirs = RC.case(name, order), BC.case(name)
        s, flat = c["surface"], c["flat"]
        frames = s.view(flat)
        assert torch.equal(frames[..., first:first + 3], theirs["bg"]) and frames.stride() == (BC.H * (4 * BC.W + 16), 4 * BC.W + 16, 4, 1)
        assert int(frames[..., fourth].max()) < 255 and int(frames[..., fourth].min()) == 0 and len(frames[..., fourth].unique()) > 200
        assert s.rest_intact(flat, torch.full_like(flat, RC.PAD)) and bool((flat[:RC.GUARD] == RC.PAD).all()) and bool((flat[-RC.GUARD:] == RC.PAD).all())
        assert flat.numel() == 2 * RC.GUARD + theirs["bg"].size(0) * BC.H * (4 * BC.W + 16)
    r = RC.roi_case(order)
    v = r["surface"].view(r["flat"])
    assert tuple(v.shape) == (1, 33, 47, 4) and v.storage_offset() % 4 == 0 and v.storage_offset() % 16 == 4 and v.stride(1) == 256
    assert torch.equal(v[..., first:first + 3], r["bg"])


@pytest.mark.parametrize("order", RC.ORDERS)
def test_a_mixed_case_stripped_is_the_frame_table_case(order):
    for name in RC.NAMES:
        c = RC.mixed(name, order)                                           # (frame_table_cases.case asserts the overhang of the clipped frame)
        theirs = FC.buffers(900 + sorted(BC.SPECS).index(name))
        for n, (s, flat) in enumerate(zip(c["surfaces"], c["flats"])):
            frame = s.view(flat)[0]
            assert tuple(frame.shape[:2]) == FC.SIZES[n] and torch.equal(RC.packed(frame, order), FC.frame_of(theirs[n], n)), (name, n)
            assert int(RC.fourth(frame, order).max()) < 255 and frame.stride(0) == 4 * FC.LAYOUT[n][1] + 16
            assert s.rest_intact(flat, torch.full_like(flat, RC.PAD))
        assert c["surfaces"][1].offset % 16 == 4
        x_lo, x_hi, y_lo, y_hi = FC.region_corners(c["rows"][FC.CLIPPED].double().numpy(), c["net"])
        h, w = FC.SIZES[FC.CLIPPED]
        assert x_lo < 0 and x_hi > w and y_lo < 0 and y_hi > h, name
