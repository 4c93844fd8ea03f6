"""CPU-side checks of the NV12 video edge (csrc/frame_nv12.hip): the colour matrices of ``spk_yuv_coeffs`` against their known
answers and their inverse property, the plane views of ``ops.nv12_planes``, the new entries on both sides of the C boundary, the
argument errors of the launchers and of ``IRFD.reenact_video(pixel_format=...)`` (all before any device use), and the fp64
reference helper tests/nv12_ref.py against a brute-force loop per pixel written from the definitions in include/spk.h."""
import ctypes
import importlib
import math
import os
import re

import pytest
import torch

import nv12_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")


def test_yuv_coeffs_known_answers(pkg):
    t601, _ = pkg.ops.yuv_coeffs()                                       # the default: BT.601, limited range
    assert torch.equal(t601, pkg.ops.yuv_coeffs("bt601", False)[0])
    assert t601[0, 0] == t601[1, 0] == t601[2, 0] and abs(float(t601[0, 0]) - 255 / 219) < 1e-15
    for got, want in ((t601[0, 2], 1.596027), (t601[1, 1], -0.391762), (t601[1, 2], -0.812968), (t601[2, 1], 2.017232)):
        assert abs(float(got) - want) < 5e-7, (float(got), want)
    assert float(t601[0, 1]) == 0.0 and float(t601[2, 2]) == 0.0
    t709, _ = pkg.ops.yuv_coeffs("bt709")
    for got, want in ((t709[0, 2], 1.792741), (t709[1, 1], -0.213249), (t709[1, 2], -0.532909), (t709[2, 1], 2.112402)):
        assert abs(float(got) - want) < 5e-7, (float(got), want)
    # black and white of the limited range: (16, 128, 128) -> 0, (235, 128, 128) -> 255
    for t in (t601, t709):
        assert float((t @ torch.tensor([16.0, 128, 128, 1], dtype=torch.float64)).abs().max()) < 1e-12
        assert float((t @ torch.tensor([235.0, 128, 128, 1], dtype=torch.float64) - 255).abs().max()) < 1e-12
    full, _ = pkg.ops.yuv_coeffs("bt601", True)
    assert abs(float(full[0, 0]) - 1.0) < 1e-15 and abs(float(full[0, 2]) - 1.402) < 1e-12 and abs(float(full[2, 1]) - 1.772) < 1e-12


@pytest.mark.parametrize("standard,full", PAIRS)
def test_yuv_coeffs_inverse_and_grey(pkg, standard, full):
    to_rgb, from_rgb = pkg.ops.yuv_coeffs(standard, full)
    assert to_rgb.shape == from_rgb.shape == (3, 4) and to_rgb.dtype == torch.float64
    eye = torch.eye(4, dtype=torch.float64)
    A, B = torch.cat([to_rgb, eye[3:]]), torch.cat([from_rgb, eye[3:]])
    assert float((A @ B - eye).abs().max()) <= 1e-12 and float((B @ A - eye).abs().max()) <= 1e-12
    kr, kb = (0.299, 0.114) if standard == "bt601" else (0.2126, 0.0722)
    sy, oy = (1.0, 0.0) if full else (219 / 255, 16.0)
    want_y = torch.tensor([sy * kr, sy * (1 - kr - kb), sy * kb, oy], dtype=torch.float64)
    assert float((from_rgb[0] - want_y).abs().max()) < 1e-15
    # the chroma rows have no grey response: every grey triple maps to U = V = 128 exactly after rint
    for g in range(256):
        yuv = from_rgb @ torch.tensor([g, g, g, 1], dtype=torch.float64)
        assert torch.equal(torch.round(yuv[1:]), torch.tensor([128.0, 128.0], dtype=torch.float64)), (g, yuv)
    assert float(from_rgb[1:, :3].sum(1).abs().max()) < 1e-15
    assert float(from_rgb[:, :3].abs().sum(1).max()) <= 1.0 + 1e-15        # no row of from_rgb has a gain


def test_yuv_coeffs_argument_errors(pkg):
    lib = pkg._lib.lib()
    m = (ctypes.c_double * 12)()
    assert lib.spk_yuv_coeffs(2020, 0, m, m) == -1 and b"601" in lib.spk_last_error()
    assert lib.spk_yuv_coeffs(601, 2, m, m) == -1 and lib.spk_yuv_coeffs(601, 0, None, None) == -1
    assert lib.spk_yuv_coeffs(709, 1, None, m) == 0 and m[3] == 0.0 and m[7] == 128.0
    for bad in (("bt2020", False), ("601", False), ("bt601", 2), ("bt601", None)):
        with pytest.raises(ValueError):
            pkg.ops.yuv_coeffs(*bad)


def test_nv12_planes_views_and_strides(pkg):
    N, H, W, pitch = 2, 6, 8, 16
    raw = torch.arange(N * (3 * H // 2) * pitch, dtype=torch.int32).remainder(251).to(torch.uint8).view(N, 3 * H // 2, pitch)
    surf = raw[:, :, :W]                                                 # a pitched decoder surface
    y, uv = pkg.ops.nv12_planes(surf)
    assert y.shape == (N, H, W) and uv.shape == (N, H // 2, W // 2, 2)
    assert y.stride() == (3 * H // 2 * pitch, pitch, 1) and uv.stride() == (3 * H // 2 * pitch, pitch, 2, 1)
    assert y.data_ptr() == surf.data_ptr() and uv.data_ptr() == surf.data_ptr() + H * pitch
    assert torch.equal(y, raw[:, :H, :W]) and torch.equal(uv[1, 2, 3], raw[1, H + 2, 6:8])
    y1, uv1 = pkg.ops.nv12_planes(surf[0])                               # one frame
    assert y1.shape == (1, H, W) and uv1.shape == (1, H // 2, W // 2, 2) and y1.data_ptr() == surf.data_ptr()
    # a pair of planes is passed through
    py, puv = torch.zeros(N, H, W, dtype=torch.uint8), torch.zeros(N, H // 2, W // 2, 2, dtype=torch.uint8)
    a, b = pkg.ops.nv12_planes((py, puv))
    assert a is py and b is puv
    for bad in (torch.zeros(N, 3 * H // 2, W), torch.zeros(N, 10, W, dtype=torch.uint8), torch.zeros(N, 9, 7, dtype=torch.uint8),
                torch.zeros(N, 9, 8, dtype=torch.uint8).transpose(1, 2), (py, puv[:, :, :2]), (py, puv.float()), (py,), "nv12",
                torch.zeros(N, H, W, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            pkg.ops.nv12_planes(bad)


def test_header_and_ctypes_agree_on_the_nv12_entries(pkg):
    L = pkg._lib
    raw = open(os.path.join(ROOT, "include", "spk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = L.lib()
    counts = {}
    for name in ("spk_yuv_coeffs", "spk_frames_nv12_to_f32", "spk_frames_f32_to_nv12", "spk_frames_paste_nv12"):
        params = re.search(name + r"\s*\(([^)]*)\)\s*;", src).group(1).split(",")
        assert len(params) == len(getattr(lib, name).argtypes), name
        counts[name] = len(params)
    assert counts == {"spk_yuv_coeffs": 4, "spk_frames_nv12_to_f32": 35, "spk_frames_f32_to_nv12": 15, "spk_frames_paste_nv12": 32}
    # the op kind: 13, spelled relative to the kind before it, and dispatched by the launch list
    m = re.search(r"enum \{\s*SPK_OP_FRAMES_TO_NV12\s*=\s*SPK_OP_NOISE_FILL \+ 1\s*\};", src)
    assert m and L.OP_FRAMES_TO_NV12 == L.OP_NOISE_FILL + 1 == 13
    body = re.search(r"typedef struct spk_frames_to_nv12_args \{(.*?)\} spk_frames_to_nv12_args;", src, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*(?:,|;)", body)
    assert names == [f[0] for f in L.FramesToNv12Args._fields_]
    assert L.FramesToNv12Args.y_image_stride.offset == 24 and L.FramesToNv12Args.N.offset == 56 and ctypes.sizeof(L.FramesToNv12Args) == 88
    launch = open(os.path.join(ROOT, "speak-hack_amd", "csrc", "launch_list.hip")).read()
    assert "case SPK_OP_FRAMES_TO_NV12" in launch
    for word in ("REPLICATION", "AFTER the resize", "2-byte aligned"):      # the definitions are part of the header
        assert word in raw, word


def test_c_launchers_refuse_bad_arguments_before_a_launch(pkg):
    """Every refusal happens on the host: made-up, never dereferenced addresses stand for the device pointers."""
    lib = pkg._lib.lib()
    P, T = 0x10000, 0x20000

    def to_f32(**kw):
        a = dict(y=P, yi=96, yr=8, uv=P + 64, ui=96, ur=8, N=1, H=8, W=8, boxes=None, y0=0, x0=0, Hin=4, Win=4, std=601, full=0, tab=T, w=T,
                 taps=2, dst=P, Hout=2, Wout=2)
        a.update(kw)
        return lib.spk_frames_nv12_to_f32(a["y"], a["yi"], a["yr"], a["uv"], a["ui"], a["ur"], a["N"], a["H"], a["W"], a["boxes"], a["y0"], a["x0"],
                                          a["Hin"], a["Win"], 0, a["std"], a["full"], a["tab"], a["tab"], a["w"], a["taps"], a["tab"], a["tab"],
                                          a["w"], a["taps"], a["dst"], a["Hout"], a["Wout"], 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, None)

    def paste(**kw):
        a = dict(src=P, N=1, Hs=4, Ws=4, y=P, yi=96, yr=8, uv=P + 64, ui=96, ur=8, H=8, W=8, h=4, w_=4, std=601, full=0, tab=T, w=T, taps=2,
                 ay=None, ax=None, lo=-1.0, k=127.5)
        a.update(kw)
        return lib.spk_frames_paste_nv12(a["src"], a["N"], a["Hs"], a["Ws"], a["y"], a["yi"], a["yr"], a["uv"], a["ui"], a["ur"], a["H"], a["W"],
                                         a["h"], a["w_"], 0, 0, None, a["std"], a["full"], a["tab"], a["tab"], a["w"], a["taps"], a["tab"], a["tab"],
                                         a["w"], a["taps"], a["ay"], a["ax"], a["lo"], a["k"], None)

    def to_nv12(**kw):
        a = dict(src=P, N=1, H=8, W=8, y=P, yi=96, yr=8, uv=P + 64, ui=96, ur=8, std=601, full=0, lo=-1.0, k=127.5)
        a.update(kw)
        return lib.spk_frames_f32_to_nv12(a["src"], a["N"], a["H"], a["W"], a["y"], a["yi"], a["yr"], a["uv"], a["ui"], a["ur"], a["std"], a["full"],
                                          a["lo"], a["k"], None)

    surface = (dict(y=None), dict(uv=None), dict(N=0), dict(H=7), dict(W=6 + 1), dict(H=0), dict(uv=P + 65), dict(ur=9), dict(ui=97), dict(yr=7),
               dict(ur=6), dict(std=2020), dict(full=2))
    for bad in surface + (dict(dst=None), dict(tab=None), dict(w=None), dict(Hin=0), dict(Win=0), dict(Hin=10), dict(Win=10), dict(taps=0),
                          dict(Hout=0), dict(Wout=-1), dict(yi=-1)):
        assert to_f32(**bad) == -1 and lib.spk_last_error(), bad
    assert to_f32(Hin=10) == -1 and b"does not fit" in lib.spk_last_error()
    assert to_f32(H=7) == -1 and b"even" in lib.spk_last_error()
    assert to_f32(uv=P + 65) == -1 and b"aligned" in lib.spk_last_error()
    for bad in surface + (dict(src=None), dict(tab=None), dict(w=None), dict(ay=T), dict(ax=T), dict(Hs=0), dict(Ws=0), dict(h=0), dict(w_=0),
                          dict(taps=0), dict(lo=math.nan), dict(k=0.0), dict(k=math.inf), dict(N=2, yi=63), dict(N=2, ui=30), dict(N=2, yi=0)):
        assert paste(**bad) == -1 and lib.spk_last_error(), bad
    assert paste(N=2, yi=63) == -1 and b"overlap" in lib.spk_last_error()
    assert paste(ay=T) == -1 and b"feather" in lib.spk_last_error()
    for bad in surface + (dict(src=None), dict(lo=math.inf), dict(k=-1.0), dict(N=2, ui=30)):
        assert to_nv12(**bad) == -1 and lib.spk_last_error(), bad
    assert to_nv12(yr=7) == -1 and b"row stride" in lib.spk_last_error()


def test_launchers_refuse_cpu_tensors_and_bad_arguments(pkg):
    ops, SpkError = pkg.ops, pkg._lib.SpkError
    surf = torch.zeros(2, 12, 8, dtype=torch.uint8)
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_from_nv12(surf, 4)
    for bad in (dict(channel_order="gbr"), dict(crop=(4, 4, 8, 2)), dict(std=(0.5, 0.0, 0.5)), dict(standard="bt2020"), dict(full_range=3)):
        with pytest.raises(ValueError):
            ops.frames_from_nv12(surf, 4, **bad)
    with pytest.raises(ValueError):
        ops.frames_from_nv12(surf, 0)
    with pytest.raises(ValueError):
        ops.frames_from_nv12(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), 4)             # packed RGB is not a surface
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_to_nv12(x)
    for bad in (dict(value_range=(1, 1)), dict(standard="rec709"), dict(full_range="yes")):
        with pytest.raises(ValueError):
            ops.frames_to_nv12(x, **bad)
    with pytest.raises(ValueError):
        ops.frames_to_nv12(torch.zeros(2, 3, 7, 8))                                     # odd height
    with pytest.raises(ValueError):
        ops.frames_to_nv12(torch.zeros(2, 8, 8, 3))
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_paste_nv12(x, surf, (0, 0, 4, 4))
    for bad in (dict(feather=-1), dict(feather=float("nan")), dict(value_range=(1, 0)), dict(standard="bt2020")):
        with pytest.raises(ValueError):
            ops.frames_paste_nv12(x, surf, (0, 0, 4, 4), **bad)
    with pytest.raises(ValueError):
        ops.frames_paste_nv12(x, surf, (0, 0, 0, 4))
    with pytest.raises(ValueError):
        ops.frames_paste_nv12(x, surf[:1], (0, 0, 4, 4))                                # one surface for two frames
    with pytest.raises(ValueError):
        ops.frames_paste_nv12(x, torch.zeros(2, 8, 8, 3, dtype=torch.uint8), (0, 0, 4, 4))


def test_reenact_video_pixel_format_argument_errors(pkg):
    import model
    m = model.IRFD()
    ident, surf = torch.zeros(16, 16, 3, dtype=torch.uint8), torch.zeros(3, 24, 16, dtype=torch.uint8)
    rgb = torch.zeros(3, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="pixel_format"):
        m.reenact_video(ident, surf, pixel_format="yuv420p")
    with pytest.raises(ValueError, match="pixel_format"):
        m.reenact_video(ident, rgb, standard="bt709")                                   # colour arguments need nv12
    with pytest.raises(ValueError, match="pixel_format"):
        m.reenact_video(ident, rgb, full_range=True)
    with pytest.raises(ValueError, match="standard"):
        m.reenact_video(ident, surf, pixel_format="nv12", standard="bt2020")
    with pytest.raises(ValueError):
        m.reenact_video(ident, rgb, pixel_format="nv12")                                # packed RGB frames are not NV12
    with pytest.raises(ValueError):
        m.reenact_video(ident, surf, pixel_format="nv12", crop=(0, 0, 17, 4))           # the box leaves the 16 x 16 frame
    with pytest.raises(ValueError):
        m.reenact_video(ident, surf, pixel_format="nv12", inplace=True)                 # inplace applies to paste=True only
    with pytest.raises(ValueError):
        m.reenact_video(ident, surf, pixel_format="nv12", feather=2)
    img, frames = torch.zeros(1, 3, 64, 64), torch.zeros(3, 3, 64, 64)
    with pytest.raises(ValueError):
        m.reenact(img, frames, output="nv21")
    with pytest.raises(ValueError):
        m.reenact(img, frames, output="nv12", channel_order="bgr")
    with pytest.raises(ValueError):
        m.reenact(img, frames, output="nv12", standard="bt2020")
    with pytest.raises(ValueError):
        m.reenact(img, frames, output="uint8", standard="bt709")


# ---- the reference helper against a loop per pixel ------------------------------------------------------------------------
def rand_u8(seed, *shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def tap_list(ops, n_in, n_out):
    first, count, w = ops.resize_tables(n_in, n_out)
    return [[(int(first[o]) + j, float(w[o, j])) for j in range(int(count[o]))] for o in range(n_out)]


def row_dot(M, c, p):
    return M[c][0] * p[0] + M[c][1] * p[1] + M[c][2] * p[2] + M[c][3]


def test_reference_helper_vs_brute_force(pkg):
    """A 6 x 8 frame, a 3 x 5 box at the odd origin (1, 3) (so the box starts and ends inside chroma blocks), and a second frame
    whose box hangs over the bottom right corner."""
    ops = pkg.ops
    H, W, h, w = 6, 8, 3, 5
    y, uv = rand_u8(1, 2, H, W), rand_u8(2, 2, H // 2, W // 2, 2)
    to_rgb, from_rgb = (m.tolist() for m in ops.yuv_coeffs())
    # in: both frames at in-frame origins, to 4 x 3
    boxes, (Ho, Wo) = [(1, 3), (3, 0)], (4, 3)
    ty, tx = tap_list(ops, h, Ho), tap_list(ops, w, Wo)
    want = torch.zeros(2, 3, Ho, Wo, dtype=torch.float64)
    for n, (y0, x0) in enumerate(boxes):
        for oy in range(Ho):
            for ox in range(Wo):
                f = [0.0, 0.0, 0.0]
                for iy, wy in ty[oy]:
                    for ix, wx in tx[ox]:
                        Y, X = y0 + iy, x0 + ix
                        px = (int(y[n, Y, X]), int(uv[n, Y >> 1, X >> 1, 0]), int(uv[n, Y >> 1, X >> 1, 1]))
                        for c in range(3):
                            f[c] += wy * wx * px[c]
                for c in range(3):
                    want[n, c, oy, ox] = min(max(row_dot(to_rgb, c, f), 0.0), 255.0) / 255 * 2 - 1
    got = R.from_nv12_ref(ops, y, uv, boxes, h, w, (Ho, Wo), torch.tensor(to_rgb, dtype=torch.float64))
    assert float((got - want).abs().max()) < 1e-12
    bgr = R.from_nv12_ref(ops, y, uv, boxes, h, w, (Ho, Wo), torch.tensor(to_rgb, dtype=torch.float64), bgr=True)
    assert torch.equal(bgr, got.flip(1))
    # out: a 4 x 4 source enlarged into the 3 x 5 box, feather 1, frame 1's box over the corner
    x = torch.randn(2, 3, 4, 4, generator=torch.Generator().manual_seed(3), dtype=torch.float64).float() * 0.7
    boxes = [(1, 3), (4, 5)]
    sy, sx = tap_list(ops, 4, h), tap_list(ops, 4, w)
    ay, ax = ops.feather_tables(h, 1).tolist(), ops.feather_tables(w, 1).tolist()
    want_y, want_uv = y.double().clone(), uv.double().clone()
    for n, (y0, x0) in enumerate(boxes):
        acc, S = {}, {}
        for by in range(h):
            for bx in range(w):
                Y, X = y0 + by, x0 + bx
                if not (0 <= Y < H and 0 <= X < W):
                    continue
                q = []
                for c in range(3):
                    v = sum(wy * wx * float(x[n, c, iy, ix]) for iy, wy in sy[by] for ix, wx in sx[bx])
                    q.append(min(max((v + 1) * 127.5, 0.0), 255.0))
                m = ay[by] * ax[bx]
                want_y[n, Y, X] = (1 - m) * float(y[n, Y, X]) + m * row_dot(from_rgb, 0, q)
                s = (Y >> 1, X >> 1)
                a = acc.setdefault(s, [0.0, 0.0])
                a[0] += 0.25 * m * row_dot(from_rgb, 1, q)
                a[1] += 0.25 * m * row_dot(from_rgb, 2, q)
                S[s] = S.get(s, 0.0) + 0.25 * m
        for s, a in acc.items():
            for c in range(2):
                want_uv[n, s[0], s[1], c] = (1 - S[s]) * float(uv[n, s[0], s[1], c]) + a[c]
    val_y, val_uv = R.paste_nv12_ref(ops, x, y, uv, boxes, h, w, torch.tensor(from_rgb, dtype=torch.float64), feather=1)
    assert float((val_y - want_y).abs().max()) < 1e-11 and float((val_uv - want_uv).abs().max()) < 1e-11
    # the box's part of the frame moved, nothing else did: frame 1 keeps all but its last 2 x 3 pixels and 1 x 2 samples
    assert torch.equal(val_y[1, :4], y[1, :4].double()) and torch.equal(val_y[1, :, :5], y[1, :, :5].double())
    assert not torch.equal(val_y[1, 4:, 5:], y[1, 4:, 5:].double())
    assert torch.equal(val_uv[1, :2], uv[1, :2].double()) and torch.equal(val_uv[1, :, :2], uv[1, :, :2].double())
    # a sample with ONE in-box pixel (frame 0, sample (0, 1): pixel (1, 3) alone) moved by that pixel's quarter weight only
    m00 = ay[0] * ax[0]
    moved = float((val_uv[0, 0, 1] - uv[0, 0, 1].double()).abs().max())
    assert 0 < moved <= 0.25 * m00 * 255
    # whole-frame, no feather: the plain conversion
    full = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(4), dtype=torch.float64).float() * 0.7
    py, puv = R.to_nv12_ref(ops, full, torch.tensor(from_rgb, dtype=torch.float64))
    q = ((full.double() + 1) * 127.5).clamp(0, 255)
    e = R.affine(torch.tensor(from_rgb, dtype=torch.float64), q)
    assert float((py - e[:, 0]).abs().max()) < 1e-12
    mean = e[:, 1:].view(1, 2, H // 2, 2, W // 2, 2).mean((3, 5)).permute(0, 2, 3, 1)
    assert float((puv - mean).abs().max()) < 1e-12
