"""CPU-side checks of the aligned video edge (``spk_frames_u8_to_f32_sim``, ``spk_frames_paste_u8_sim``): the fp64 model
tests/sim_ref.py against what it must reduce to for an axis-aligned crop -- torch's ``interpolate(antialias=True)`` on the way in,
the ``resize_tables`` / ``feather_tables`` composition on the way out --, ``similarity_rows`` against closed-form corners, the
entry points on both sides of the C boundary with their refusals (all before a launch, so without a device), and every
``ValueError`` of the launchers and of ``IRFD.reenact_video(align=...)`` that is raised before a device is touched."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")


def frames(seed, *shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


# ---- the model against what it reduces to without a rotation ---------------------------------------------------------------------
@pytest.mark.parametrize("scale", [2, 4])
def test_model_way_in_is_interpolate_antialias_for_whole_frames(scale):
    """c = 0, the whole 40 x 56 frame, a scale that is exact in fp32: the triangle filter along the crop's axes is torch's
    separable one.  In byte units (scale 1, shift 0): <= 1e-12."""
    H, W = 40, 56
    Ho, Wo = H // scale, W // scale
    u8 = frames(scale, 2, H, W, 3)
    got, hit = R.warp_in(u8.numpy(), [[scale, 0, 0, 0]] * 2, Ho, Wo, scale=(1.0,) * 3, shift=(0.0,) * 3)
    want = F.interpolate(u8.permute(0, 3, 1, 2).double(), size=(Ho, Wo), mode="bilinear", align_corners=False, antialias=True).numpy()
    err = float(np.abs(got - want).max())
    print(f"model way in, scale {scale}: largest |model - interpolate| = {err:.3e} byte units")
    assert hit.all() and err <= 1e-12


@pytest.mark.parametrize("S,h,origin,feather", [(16, 24, (5, 7), 0), (16, 24, (5, 7), 2.5), (16, 40, (0, 3), 3), (16, 8, (20, 33), 1),
                                                (16, 16, (9, 2), 2.5)])
def test_model_way_out_is_the_table_composition_for_integer_boxes(pkg, S, h, origin, feather):
    """c = 0 and a box at an integer origin (scales 1.5, 2.5, 0.5, 1): region, weights and feather are those of
    ``resize_tables`` / ``feather_tables``.  Before the final rounding: <= 1e-4 byte units (the feather table is fp32)."""
    ops = pkg.ops
    N, H, W = 2, 48, 64
    g = torch.Generator().manual_seed(S + h)
    x = torch.randn(N, 3, S, S, generator=g) * 0.7
    bg = frames(h, N, H, W, 3)
    y0, x0 = origin
    z, region, margin = R.paste_out(x.numpy(), bg.numpy(), [[h / S, 0, x0, y0]] * N, feather=feather)
    first, count, w = ops.resize_tables(S, h)
    A = torch.zeros(h, S, dtype=torch.float64)
    for o in range(h):
        A[o, int(first[o]):int(first[o]) + int(count[o])] = w[o, :int(count[o])]
    val = torch.einsum("yj,ncji,xi->nyxc", A, x.double(), A)
    q = ((val + 1) * 127.5).clamp(0, 255)
    a = ops.feather_tables(h, feather).double()
    m = (a.view(h, 1) * a.view(1, h)).view(1, h, h, 1)
    b = bg[:, y0:y0 + h, x0:x0 + h].double()
    want = bg.double().clone()
    want[:, y0:y0 + h, x0:x0 + h] = b + m * (q - b)
    box = torch.zeros(N, H, W, dtype=torch.bool)
    box[:, y0:y0 + h, x0:x0 + h] = True
    assert np.array_equal(region, box.numpy()) and margin > 0.1
    err = float(np.abs(z - want.numpy()).max())
    print(f"model way out, {S} -> {h} at {origin}, feather {feather}: largest |model - tables| = {err:.3e} byte units")
    assert err <= 1e-4


def test_model_invalid_rows_and_empty_footprints():
    u8 = frames(3, 3, 12, 16, 3).numpy()
    sim = [[1, 0, 0, 0], [float("nan"), 0, 0, 0], [1, 0, 1000, 0]]                    # valid, invalid, valid but far away
    dst, hit = R.warp_in(u8, sim, 4, 4, shift=(-1.0, -0.5, 0.25))
    assert hit[0].all() and not hit[1].any() and not hit[2].any()
    for c, sh in enumerate((-1.0, -0.5, 0.25)):
        assert (dst[1:, c] == sh).all()
    x = np.zeros((3, 3, 4, 4), dtype=np.float32)
    z, region, _ = R.paste_out(x, u8, sim)
    assert region[0, :4, :4].all() and int(region[0].sum()) == 16 and not region[1:].any() and np.array_equal(z[1:], u8[1:])


# ---- similarity_rows -------------------------------------------------------------------------------------------------------------
def test_similarity_rows_against_closed_form_corners(pkg):
    ops = pkg.ops
    centres, sides, angles, size = [(20.5, 30.25), (11.0, 40.0), (35.1, 50.3)], [20.8, 9.6, 16.0], [0.3, -1.1, 2.0], 16
    rows = ops.similarity_rows(centres, sides, angles, size)
    assert rows.dtype == torch.float32 and rows.shape == (3, 4) and not rows.is_cuda
    for (cy, cx), side, th, row in zip(centres, sides, angles, rows.double().tolist()):
        a, c, tx, ty = row
        assert abs(math.hypot(a, c) - side / size) < 1e-6 and abs(math.atan2(c, a) - th) < 1e-6
        for su, sv in ((-1, -1), (1, -1), (-1, 1), (1, 1)):          # the corners of the network image and of the rotated square
            u, v = size / 2 * (1 + su), size / 2 * (1 + sv)
            ex, ey = side / 2 * su, side / 2 * sv
            want_x, want_y = cx + math.cos(th) * ex - math.sin(th) * ey, cy + math.sin(th) * ex + math.cos(th) * ey
            assert abs(a * u - c * v + tx - want_x) < 1e-4 and abs(c * u + a * v + ty - want_y) < 1e-4
    model_rows = torch.tensor([R.rows(c, s, t, (size, size)) for c, s, t in zip(centres, sides, angles)], dtype=torch.float64).float()
    assert torch.allclose(rows, model_rows, rtol=1e-6, atol=1e-6)
    # no rotation, the centre of a box: that box
    assert ops.similarity_rows((3 + 12, 5 + 12), 24, 0.0, 16).tolist() == [[1.5, 0.0, 5.0, 3.0]]
    # one centre, many sides; a rectangular network image: side spans the width
    many = ops.similarity_rows((10, 12), [8, 16, 32], 0.0, (12, 20))
    assert many.shape == (3, 4) and many[:, 0].tolist() == [0.4000000059604645, 0.800000011920929, 1.600000023841858]
    assert torch.allclose(many[1], torch.tensor(R.rows((10, 12), 16, 0.0, (12, 20)), dtype=torch.float32))
    with pytest.raises(ValueError):
        ops.similarity_rows([(1, 2), (3, 4)], [1, 2, 3], 0.0, 16)
    with pytest.raises(ValueError):
        ops.similarity_rows((1, 2), 8, 0.0, 0)


# ---- the C boundary --------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_new_entries(pkg):
    L = pkg._lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spk.h")).read(), flags=re.S)
    lib = L.lib()
    for name in ("spk_frames_u8_to_f32_sim", "spk_frames_paste_u8_sim"):
        decl = re.search(name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert decl, f"{name} is not declared in include/spk.h"
        params = [p.strip() for p in decl.group(1).split(",")]
        assert name in L.exported_symbols() and len(getattr(lib, name).argtypes) == len(params), name
        for p, t in zip(params, getattr(lib, name).argtypes):         # pointers travel as void*, scalars by their C type
            want = "c_void_p" if "*" in p else {"int": "c_int", "int64_t": "c_long", "float": "c_float", "double": "c_double"}[p.split()[0]]
            assert t.__name__ == want, (name, p, t)


def test_entry_refusals_need_no_device(pkg):
    """Every refusal of the two entry points happens before a launch: -1 and a message, on a machine without a GPU."""
    lib = pkg._lib.lib()
    p = 4096                     # any non-null address: the arguments are refused before anything is read or launched

    def way_in(src=p, dst=p, sim=p, N=1, H=8, W=8, row=24, img=192, Hout=2, Wout=2):
        return lib.spk_frames_u8_to_f32_sim(src, img, row, N, H, W, sim, 0, dst, Hout, Wout, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, None)

    for bad in (dict(src=None), dict(dst=None), dict(sim=None), dict(N=0), dict(H=0), dict(W=-1), dict(Hout=0), dict(Wout=0), dict(row=23),
                dict(img=-1), dict(W=0x7fffffff)):
        assert way_in(**bad) == -1, bad
        assert lib.spk_last_error(), bad
    assert way_in(sim=None) == -1 and b"transform" in lib.spk_last_error()
    assert way_in(row=23) == -1 and b"row stride" in lib.spk_last_error()

    def way_out(src=p, dst=p, sim=p, N=1, Hs=4, Ws=4, H=8, W=8, row=24, img=192, feather=0.0, lo=-1.0, k=127.5):
        return lib.spk_frames_paste_u8_sim(src, N, Hs, Ws, dst, img, row, H, W, sim, 0, feather, lo, k, None)

    for bad in (dict(src=None), dict(dst=None), dict(sim=None), dict(N=0), dict(Hs=0), dict(Ws=0), dict(H=0), dict(W=0), dict(row=23),
                dict(N=2, img=7 * 24 + 23), dict(N=2, img=0), dict(N=2, img=-192), dict(feather=-0.5), dict(feather=float("nan")),
                dict(feather=float("inf")), dict(k=0.0), dict(lo=float("nan")), dict(k=float("inf")), dict(W=0x7fffffff)):
        assert way_out(**bad) == -1, bad
        assert lib.spk_last_error(), bad
    assert way_out(N=2, img=0) == -1 and b"overlap" in lib.spk_last_error()
    assert way_out(feather=-1.0) == -1 and b"feather" in lib.spk_last_error()
    assert way_out(sim=None) == -1 and b"transform" in lib.spk_last_error()


# ---- the launchers and reenact_video: what is refused before a device is touched ---------------------------------------------------
BAD_ROWS = [
    [[1, 0, 0, 0], [float("nan"), 0, 0, 0]],                     # NaN
    [[1, 0, 0, float("inf")], [1, 0, 0, 0]],
    [[0, 0, 3, 4], [1, 0, 0, 0]],                                # s = 0
    [[1, 0, 0, 0], [1 / 32, 0, 0, 0]],                           # s = 1/32
    [[0, 32, 0, 0], [1, 0, 0, 0]],                               # s = 32
    [[1, 0, 0], [1, 0, 0]],                                      # [N,3]
    [[1, 0, 0, 0]],                                              # a row per frame
]


@pytest.mark.parametrize("rows", BAD_ROWS)
def test_launchers_refuse_bad_host_rows_before_any_device_use(pkg, rows):
    ops = pkg.ops
    x, u8 = torch.zeros(2, 3, 4, 4), torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for form in (rows, torch.tensor(rows, dtype=torch.float64)):
        with pytest.raises(ValueError, match="sim"):
            ops.frames_from_u8_aligned(u8, 4, form)
        with pytest.raises(ValueError, match="sim"):
            ops.frames_paste_u8_aligned(x, u8, form)
        with pytest.raises(ValueError):
            ops.parse_sim(form, 2)


def test_launchers_check_the_rest_and_have_no_cpu_path(pkg):
    ops, SpkError = pkg.ops, pkg._lib.SpkError
    x, u8 = torch.zeros(2, 3, 4, 4), torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    good = [[1, 0, 0, 0], [0.5, 0.5, 1, 2]]
    rows = ops.parse_sim(good, 2)
    assert rows.dtype == torch.float32 and rows.tolist() == [[1, 0, 0, 0], [0.5, 0.5, 1, 2]]
    assert ops.parse_sim([[1 / 16, 0, 0, 0], [0, -16, 0, 0]], 2).shape == (2, 4)          # the ends of the scale range are valid
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_from_u8_aligned(u8, 4, good)
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_paste_u8_aligned(x, u8, good)
    with pytest.raises(ValueError):
        ops.frames_from_u8_aligned(u8, 0, good)
    with pytest.raises(ValueError):
        ops.frames_from_u8_aligned(u8, 4, good, channel_order="gbr")
    with pytest.raises(ValueError):
        ops.frames_from_u8_aligned(u8, 4, good, std=0)
    with pytest.raises(ValueError):
        ops.frames_from_u8_aligned(u8.permute(0, 3, 1, 2), 4, good)
    with pytest.raises(ValueError, match="feather"):
        ops.frames_paste_u8_aligned(x, u8, good, feather=-1)
    with pytest.raises(ValueError):
        ops.frames_paste_u8_aligned(x, u8, good, value_range=(1, 1))
    with pytest.raises(ValueError):
        ops.frames_paste_u8_aligned(x, u8[:1], good)                                    # a frame per generated frame
    with pytest.raises(ValueError):
        ops.frames_paste_u8_aligned(torch.zeros(2, 4, 4, 3), u8, good)


def test_reenact_video_align_argument_errors(pkg):
    import model
    m = model.IRFD()
    ident, video = torch.zeros(48, 64, 3, dtype=torch.uint8), torch.zeros(3, 48, 64, 3, dtype=torch.uint8)
    surf = torch.zeros(3, 72, 64, dtype=torch.uint8)
    good = [[0.25, 0, 3, 4]] * 3
    with pytest.raises(ValueError, match="crop and align"):
        m.reenact_video(ident, video, crop=(3, 5, 40, 44), align=good)
    with pytest.raises(ValueError, match="crop and align"):
        m.reenact_video(ident, video, crop=(3, 5, 40, 44), align=good, paste=True)
    with pytest.raises(ValueError, match="align"):
        m.reenact_video(ident, surf, align=good, pixel_format="nv12")
    with pytest.raises(ValueError, match="align"):
        m.reenact_video(ident, surf, align=good, pixel_format="nv12", paste=True)
    for rows in BAD_ROWS[:6]:
        bad = rows + [[1, 0, 0, 0][:len(rows[0])]]
        with pytest.raises(ValueError, match="align"):
            m.reenact_video(ident, video, align=bad)
        with pytest.raises(ValueError, match="align"):
            m.reenact_video(ident, video, align=torch.tensor(bad), paste=True, feather=2)
    with pytest.raises(ValueError, match="align"):
        m.reenact_video(ident, video, align=good[:2])                                    # a row per frame
    with pytest.raises(ValueError, match="inplace"):
        m.reenact_video(ident, video, align=good, inplace=True)                          # the rules of paste= hold as they were
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        m.reenact_video(ident, video, align=good, paste=True)
