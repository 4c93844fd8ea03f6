"""CPU-side checks of the full-frame way out of the video edge (``spk_frames_paste_u8``, ``spk_frames_u8_to_f32_boxes``,
``spk_feather_table``): the feather table against its formula, the new entry points on both sides of the C boundary, their
refusals (all before a launch, so without a device), and the argument errors of the launchers and of
``IRFD.reenact_video(paste=...)``."""
import importlib
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")


def feather_ref(n, feather):
    i = torch.arange(n, dtype=torch.float64)
    return torch.minimum(torch.ones(n, dtype=torch.float64), (torch.minimum(i, n - 1 - i) + 1) / (feather + 1.0)).float()


@pytest.mark.parametrize("n", [1, 2, 9, 11, 32, 37, 53, 400])
@pytest.mark.parametrize("feather", [0, 0.5, 3, 40, 1000])
def test_feather_tables_equal_the_formula(pkg, n, feather):
    a = pkg.ops.feather_tables(n, feather)
    assert a.dtype == torch.float32 and a.shape == (n,) and not a.is_cuda
    assert torch.equal(a, feather_ref(n, feather))
    assert torch.equal(a, a.flip(0)) and float(a.max()) <= 1.0 and float(a.min()) > 0.0
    if feather == 0:
        assert torch.all(a == 1)
    if feather >= n:                                  # wider than the box: no pixel reaches weight 1
        assert float(a.max()) < 1.0 and float(a.max()) == float(torch.tensor(((n - 1) // 2 + 1) / (feather + 1.0)).float())
    else:
        assert float(a[0]) == float(torch.tensor(1.0 / (feather + 1.0)).float())


def test_feather_table_argument_errors(pkg):
    lib = pkg._lib.lib()
    a = torch.empty(4, dtype=torch.float32)
    assert lib.spk_feather_table(0, 1.0, a.data_ptr()) == -1 and lib.spk_last_error()
    assert lib.spk_feather_table(4, -0.5, a.data_ptr()) == -1 and b"feather" in lib.spk_last_error()
    assert lib.spk_feather_table(4, float("nan"), a.data_ptr()) == -1
    assert lib.spk_feather_table(4, float("inf"), a.data_ptr()) == -1
    assert lib.spk_feather_table(4, 1.0, None) == -1 and b"null" in lib.spk_last_error()
    assert lib.spk_feather_table(4, 1.0, a.data_ptr()) == 0 and a.tolist() == [0.5, 1.0, 1.0, 0.5]
    for bad in ((0, 1), (4, -1), (4, float("nan")), (4, float("inf"))):
        with pytest.raises(ValueError):
            pkg.ops.feather_tables(*bad)


def test_header_and_ctypes_agree_on_the_new_entries(pkg):
    L = pkg._lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spk.h")).read(), flags=re.S)
    lib = L.lib()
    for name in ("spk_frames_paste_u8", "spk_frames_u8_to_f32_boxes", "spk_feather_table"):
        decl = re.search(name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert decl, f"{name} is not declared in include/spk.h"
        params = [p.strip() for p in decl.group(1).split(",")]
        assert name in L.exported_symbols() and len(getattr(lib, name).argtypes) == len(params), name
        for p, t in zip(params, getattr(lib, name).argtypes):         # pointers travel as void*, scalars by their C type
            want = "c_void_p" if "*" in p else {"int": "c_int", "int64_t": "c_long", "float": "c_float", "double": "c_double"}[p.split()[0]]
            assert t.__name__ == want, (name, p, t)
    # the launch-list enum and the quantiser's descriptor are as they were: the paste is an ordinary launcher call
    full = open(os.path.join(ROOT, "include", "spk.h")).read()
    kinds = re.findall(r"^\s*(SPK_OP_[A-Z0-9_]+)\s*=", full, flags=re.M)
    assert len(kinds) == len(set(kinds)) == 12 and not any("PASTE" in k for k in kinds)
    assert [f[0] for f in L.FramesToU8Args._fields_] == ["x", "y", "N", "H", "W", "swap_rb", "lo", "k"]


def test_entry_refusals_need_no_device(pkg):
    """Every refusal of the two new entry points happens before a launch: -1 and a message, on a machine without a GPU."""
    lib = pkg._lib.lib()
    p = 4096                     # any non-null address: the arguments are refused before anything is read or launched

    def paste(src=p, dst=p, tab=p, ay=None, ax=None, N=1, Hs=4, Ws=4, H=8, W=8, h=4, w=4, row=24, img=None, taps=2, lo=-1.0, k=127.5,
              boxes=None):
        return lib.spk_frames_paste_u8(src, N, Hs, Ws, dst, H * row if img is None else img, row, H, W, h, w, 0, 0, boxes, 0,
                                       tab, tab, tab, taps, tab, tab, tab, taps, ay, ax, lo, k, None)

    for bad in (dict(src=None), dict(dst=None), dict(tab=None), dict(ay=p), dict(ax=p), dict(N=0), dict(Hs=0), dict(Ws=0), dict(H=0),
                dict(W=0), dict(h=0), dict(w=0), dict(taps=0), dict(row=23), dict(N=2, img=7 * 24 + 23), dict(N=2, img=0), dict(k=0.0),
                dict(lo=float("nan")), dict(k=float("inf"))):
        assert paste(**bad) == -1, bad
        assert lib.spk_last_error(), bad
    assert paste(row=23) == -1 and b"row stride" in lib.spk_last_error()
    assert paste(ay=p) == -1 and b"feather" in lib.spk_last_error()
    assert paste(N=2, img=0) == -1 and b"overlap" in lib.spk_last_error()

    def boxes(src=p, dst=p, tab=p, box=p, N=1, H=8, W=8, Hin=4, Win=4, row=24, taps=2, Hout=2, Wout=2, img=192):
        return lib.spk_frames_u8_to_f32_boxes(src, img, row, N, H, W, box, Hin, Win, 0, tab, tab, tab, taps, tab, tab, tab, taps, dst,
                                              Hout, Wout, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, None)

    for bad in (dict(src=None), dict(dst=None), dict(tab=None), dict(box=None), dict(N=0), dict(Hin=0), dict(Win=0), dict(Hout=0),
                dict(Wout=0), dict(taps=0), dict(row=23), dict(Hin=9), dict(Win=9), dict(img=-1)):
        assert boxes(**bad) == -1, bad
        assert lib.spk_last_error(), bad
    assert boxes(Hin=9) == -1 and b"does not fit" in lib.spk_last_error()
    assert boxes(box=None) == -1 and b"box" in lib.spk_last_error()


def test_parse_boxes_forms(pkg):
    pb = pkg.ops.parse_boxes
    assert pb((1, 2, 3, 4), 5, 8, 8) == ((1, 2), 3, 4)
    rows = [(0, 0, 3, 4), (5, 4, 3, 4), (2, 1, 3, 4)]
    for form in (rows, [list(r) for r in rows], torch.tensor(rows), torch.tensor(rows, dtype=torch.int32)):
        o, h, w = pb(form, 3, 8, 8)
        assert (h, w) == (3, 4) and o.dtype == torch.int32 and o.tolist() == [[0, 0], [5, 4], [2, 1]]
    with pytest.raises(ValueError, match="one filter table"):
        pb([(0, 0, 3, 4), (0, 0, 4, 3), (0, 0, 3, 4)], 3, 8, 8)
    with pytest.raises(ValueError, match="leaves"):
        pb([(0, 0, 3, 4), (6, 0, 3, 4), (0, 0, 3, 4)], 3, 8, 8)
    with pytest.raises(ValueError, match="leaves"):
        pb((0, 5, 3, 4), 3, 8, 8)
    with pytest.raises(ValueError):
        pb(rows[:2], 3, 8, 8)                                             # a row per frame
    with pytest.raises(ValueError):
        pb(torch.tensor(rows).float(), 3, 8, 8)
    yx = torch.zeros(3, 2, dtype=torch.int32)
    assert pb((yx, 3, 4), 3, 8, 8)[0] is yx                               # origins as given: the kernels clamp / skip
    with pytest.raises(ValueError):
        pb((yx.long(), 3, 4), 3, 8, 8)
    with pytest.raises(ValueError):
        pb((yx[:2], 3, 4), 3, 8, 8)
    with pytest.raises(ValueError, match="fit"):
        pb((yx, 9, 4), 3, 8, 8)
    assert pb((yx, 9, 4), 3, 8, 8, inside=False)[1:] == (9, 4)            # the paste skips what leaves the frame


def test_launchers_refuse_cpu_tensors_and_bad_arguments(pkg):
    ops, SpkError = pkg.ops, pkg._lib.SpkError
    x, u8 = torch.zeros(2, 3, 4, 4), torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_paste_u8(x, u8, (0, 0, 4, 4))
    with pytest.raises(ValueError, match="one filter table"):
        ops.frames_paste_u8(x, u8, [(0, 0, 4, 4), (0, 0, 4, 5)])
    with pytest.raises(ValueError, match="leaves"):
        ops.frames_paste_u8(x, u8, (5, 0, 4, 4))
    with pytest.raises(ValueError, match="leaves"):
        ops.frames_paste_u8(x, u8, [(0, 0, 4, 4), (0, 5, 4, 4)])
    with pytest.raises(ValueError, match="feather"):
        ops.frames_paste_u8(x, u8, (0, 0, 4, 4), feather=-1)
    with pytest.raises(ValueError):
        ops.frames_paste_u8(x, u8, (0, 0, 4, 4), channel_order="gbr")
    with pytest.raises(ValueError):
        ops.frames_paste_u8(x, u8, (0, 0, 4, 4), value_range=(1, 1))
    with pytest.raises(ValueError):
        ops.frames_paste_u8(x, u8[:1], (0, 0, 4, 4))                      # a frame per generated frame
    with pytest.raises(ValueError):
        ops.frames_paste_u8(torch.zeros(2, 4, 4, 3), u8, (0, 0, 4, 4))
    # the input side: the same three box forms
    with pytest.raises(ValueError, match="one filter table"):
        ops.frames_from_u8(u8, 4, crop=[(0, 0, 4, 4), (0, 0, 5, 4)])
    with pytest.raises(ValueError, match="leaves"):
        ops.frames_from_u8(u8, 4, crop=[(0, 0, 4, 4), (5, 0, 4, 4)])
    with pytest.raises(ValueError, match="fit"):
        ops.frames_from_u8(u8, 4, crop=(torch.zeros(2, 2, dtype=torch.int32), 9, 4))
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_from_u8(u8, 4, crop=[(0, 0, 4, 4), (1, 2, 4, 4)])
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_from_u8(u8, 4, crop=(torch.zeros(2, 2, dtype=torch.int32), 4, 4))


def test_reenact_video_paste_argument_errors(pkg):
    import model
    m = model.IRFD()
    ident, video = torch.zeros(48, 64, 3, dtype=torch.uint8), torch.zeros(3, 48, 64, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="inplace"):
        m.reenact_video(ident, video, inplace=True)
    with pytest.raises(ValueError, match="feather"):
        m.reenact_video(ident, video, paste=True, feather=-2)
    with pytest.raises(ValueError, match="feather"):
        m.reenact_video(ident, video, feather=3)                          # a feather without a paste
    with pytest.raises(ValueError, match="one filter table"):
        m.reenact_video(ident, video, paste=True, crop=[(0, 0, 40, 44), (0, 0, 40, 44), (0, 0, 44, 40)])
    with pytest.raises(ValueError, match="leaves"):
        m.reenact_video(ident, video, paste=True, crop=[(0, 0, 40, 44), (9, 0, 40, 44), (0, 0, 40, 44)])
    with pytest.raises(ValueError, match="leaves"):
        m.reenact_video(ident, video, paste=True, crop=(0, 21, 40, 44))
    with pytest.raises(ValueError):
        m.reenact_video(ident, video, paste=True, crop=[(0, 0, 40, 44)] * 2)        # a box per frame
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        m.reenact_video(ident, video, paste=True, crop=(3, 5, 40, 44), feather=4)
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        m.reenact_video(ident, video, paste=True, inplace=True)
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        m.reenact_video(ident, video, crop=[(3, 5, 40, 44), (4, 6, 40, 44), (5, 7, 40, 44)])
