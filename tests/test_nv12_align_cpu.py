"""CPU checks around the aligned NV12 edge (csrc/frame_sim_nv12.hip): the numpy model tests/nv12_sim_ref.py against a loop per pixel
written from include/spk.h, against ``nv12_ref.paste_nv12_ref`` where an integer box makes the two forms one, and against
``sim_ref.warp_in`` on a grey surface; what the GPU cases of tests/nv12_sim_cases.py rely on; the launchers' argument errors; and
the C boundary (header against prototypes, every refusal without a device)."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import blend_ref as B
import nv12_ref as NR
import nv12_sim_cases as NC
import nv12_sim_ref as M
import sim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


def tri(t):
    return max(0.0, 1.0 - abs(t))


# ---- the model against a loop per pixel --------------------------------------------------------------------------------------------
def loop_in(y, uv, row, Hout, Wout, to_rgb, scale, shift, swap):
    H, W = y.shape
    a, c, tx, ty = (float(v) for v in R.rows64(row)[0])
    s = math.hypot(a, c)
    S = max(s, 1.0)
    out = np.empty((3, Hout, Wout))
    for oy in range(Hout):
        for ox in range(Wout):
            px, py = a * (ox + 0.5) - c * (oy + 0.5) + tx, c * (ox + 0.5) + a * (oy + 0.5) + ty
            acc, wt = [0.0, 0.0, 0.0], 0.0
            for iy in range(H):
                for ix in range(W):
                    dx, dy = ix + 0.5 - px, iy + 0.5 - py
                    w = tri((a * dx + c * dy) / s / S) * tri((-c * dx + a * dy) / s / S)
                    wt += w
                    for f, v in enumerate((y[iy, ix], uv[iy >> 1, ix >> 1, 0], uv[iy >> 1, ix >> 1, 1])):
                        acc[f] += w * float(v)
            for ch in range(3):
                rgb = 0.0 if wt <= 0 else min(max(sum(to_rgb[ch, f] * acc[f] / wt for f in range(3)) + to_rgb[ch, 3], 0.0), 255.0)
                cd = 2 - ch if swap else ch
                out[cd, oy, ox] = scale[cd] * rgb + shift[cd]
    return out


def loop_out(x, y, uv, row, from_rgb, feather, matte, colour):
    Hs, Ws = x.shape[1:]
    H, W = y.shape
    a, c, tx, ty = (float(v) for v in R.rows64(row)[0])
    s = math.hypot(a, c)
    r = max(1.0, 1.0 / s)
    z_y, z_uv = y.astype(np.float64), uv.astype(np.float64)
    count = np.zeros((H // 2, W // 2), dtype=int)
    for CY in range(H // 2):
        for CX in range(W // 2):
            acc, Ssum = [0.0, 0.0], 0.0
            for Y, X in ((2 * CY, 2 * CX), (2 * CY, 2 * CX + 1), (2 * CY + 1, 2 * CX), (2 * CY + 1, 2 * CX + 1)):
                dx, dy = X + 0.5 - tx, Y + 0.5 - ty
                u, v = (a * dx + c * dy) / (s * s), (-c * dx + a * dy) / (s * s)
                if not (0 <= u < Ws and 0 <= v < Hs):
                    continue
                wu, wv = [tri((i + 0.5 - u) / r) for i in range(Ws)], [tri((j + 0.5 - v) / r) for j in range(Hs)]
                norm = sum(wu) * sum(wv)
                q = []
                for ch in range(3):
                    val = sum(wv[j] * wu[i] * float(x[ch, j, i]) for j in range(Hs) for i in range(Ws)) / norm
                    qc = min(max((val + 1.0) * 127.5, 0.0), 255.0)
                    if colour is not None:
                        qc = min(max(float(colour[ch, 0]) * qc + float(colour[ch, 1]), 0.0), 255.0)
                    q.append(qc)
                m = min(1.0, (s * min(u, Ws - u) + 0.5) / (feather + 1)) * min(1.0, (s * min(v, Hs - v) + 0.5) / (feather + 1))
                if matte is not None:
                    mt = sum(wv[j] * wu[i] * (0.0 if math.isnan(matte[j, i]) else float(matte[j, i])) for j in range(Hs) for i in range(Ws)) / norm
                    m *= min(max(mt, 0.0), 1.0)
                e = [sum(from_rgb[f, ch] * q[ch] for ch in range(3)) + from_rgb[f, 3] for f in range(3)]
                z_y[Y, X] = min(max((1 - m) * float(y[Y, X]) + m * e[0], 0.0), 255.0)
                acc[0] += 0.25 * m * e[1]
                acc[1] += 0.25 * m * e[2]
                Ssum += 0.25 * m
                count[CY, CX] += 1
            if count[CY, CX]:
                for f in range(2):
                    z_uv[CY, CX, f] = min(max((1 - Ssum) * float(uv[CY, CX, f]) + acc[f], 0.0), 255.0)
    return z_y, z_uv, count


@pytest.mark.parametrize("standard,full", [("bt601", False), ("bt709", True)])
def test_model_against_a_loop_per_pixel(standard, full):
    """One small case: a 10 x 12 surface, a 4 x 5 image, rotation with s > 1 and a region over the frame's corner."""
    Hh, Ww, net = 10, 12, (4, 5)
    to_rgb, from_rgb = NC.coeffs(standard, full)
    y, uv = NC.surface_from_rgb(5, 1, Hh, Ww, standard, full)
    y, uv = y.numpy(), uv.numpy()
    x = NC.BC.source(6, 1, *net).numpy()
    matte = NC.BC.matte_for(7, 1, 8, 10)[0, :4, :5].numpy()
    colour = np.array([[[1.2, -9.0], [0.8, 14.0], [float("nan"), 3.0]]], dtype=np.float32)
    for row in ([R.rows((4.7, 6.2), 1.7 * net[1], 0.4, net)], [R.rows((1.3, 9.9), 0.8 * net[1], -0.9, net)]):
        got = M.paste_out(x, y, uv, row, from_rgb, to_rgb, feather=1.5, matte=matte, colour=colour)
        fixed = np.where(np.isfinite(colour[0]).all(1, keepdims=True), colour[0], np.array([1.0, 0.0]))
        z_y, z_uv, count = loop_out(x[0], y[0], uv[0], row, from_rgb, 1.5, matte, fixed)
        assert np.array_equal(count, got["count"][0]) and got["touched_uv"][0].sum() == (count > 0).sum() >= 4
        assert np.abs(z_y - got["z_y"][0]).max() <= 1e-10 and np.abs(z_uv - got["z_uv"][0]).max() <= 1e-10
        assert (got["m"][0][~got["region"][0]] == 0).all() and (got["m"][0] >= 0).all() and (got["m"][0] <= 1).all()
        scale, shift = (0.01, 0.02, 0.03), (-1.0, -0.5, 0.25)
        for swap in (False, True):
            dst, hit = M.warp_in(y, uv, row, 4, 5, to_rgb, scale, shift, swap)
            want = loop_in(y[0], uv[0], row, 4, 5, to_rgb, scale, shift, swap)
            assert np.abs(dst[0] - want).max() <= 1e-12


def test_model_outputs_by_rule():
    """An invalid row and a footprint outside the frame: shift exactly on the way in; nothing touched on the way out."""
    to_rgb, from_rgb = NC.coeffs()
    y, uv = (t.numpy() for t in NC.surface_from_rgb(8, 2, 8, 8))
    rows = [[float("nan"), 0, 0, 0], [1.0, 0.0, 40.0, 40.0]]
    dst, hit = M.warp_in(y, uv, rows, 4, 4, to_rgb, shift=(-1.0, 0.5, 2.0))
    assert not hit.any() and (dst == np.array([-1.0, 0.5, 2.0]).reshape(1, 3, 1, 1)).all()
    out = M.paste_out(np.zeros((2, 3, 4, 4), dtype=np.float32), y, uv, rows, from_rgb, to_rgb)
    assert not out["region"].any() and not out["touched_uv"].any() and np.array_equal(out["z_y"], y) and np.array_equal(out["z_uv"], uv)
    assert out["valid"].tolist() == [False, True] and (out["sums"] == 0).all()


@pytest.mark.parametrize("feather", [0, 2.5])
@pytest.mark.parametrize("origin", [(4, 6), (5, 7), (-3, 41)])
def test_model_integer_box_is_the_table_model(pkg, feather, origin):
    """c = 0, s = 1.5: ``nv12_ref.paste_nv12_ref`` (even and odd origins, a box over the frame's edge).  1e-4 byte units: the table
    model sums with ``ops.resize_tables``' weights and the fp32 ramps of ``ops.feather_tables``."""
    S, h = 16, 24
    to_rgb, from_rgb = NC.coeffs()
    x = NC.BC.source(18, 2, S, S)
    y, uv = NC.surface_from_rgb(19, 2, NC.H, NC.W)
    rows = [[h / S, 0, origin[1], origin[0]]] * 2
    got = M.paste_out(x.numpy(), y.numpy(), uv.numpy(), rows, from_rgb, to_rgb, feather=feather)
    val_y, val_uv = NR.paste_nv12_ref(pkg.ops, x, y, uv, [origin] * 2, h, h, torch.from_numpy(from_rgb), feather=feather)
    ey, euv = np.abs(got["z_y"] - val_y.numpy()).max(), np.abs(got["z_uv"] - val_uv.numpy()).max()
    print(f"integer box at {origin}, feather {feather}: |z_y - val_y| <= {ey:.2e}, |z_uv - val_uv| <= {euv:.2e}")
    assert ey <= 1e-4 and euv <= 1e-4
    box = np.zeros((2, NC.H, NC.W), dtype=bool)
    box[:, max(origin[0], 0):origin[0] + h, max(origin[1], 0):origin[1] + h] = True
    assert np.array_equal(got["region"], box)


def test_model_grey_surface_is_sim_ref():
    """U = V = 128 gives R = G = B = clamp(ay (Y - oy)): ``sim_ref.warp_in`` of the Y plane through that map."""
    to_rgb, _ = NC.coeffs()
    y = NC.BC.frames(21, 3, NC.H, NC.W).clamp(16, 235)                     # in gamut: the clamp is idle, the matrix commutes with the sum
    uv = torch.full((3, NC.H // 2, NC.W // 2, 2), 128, dtype=torch.uint8)
    rows = NC.BC.rows_for((0, 1, 2), (16, 16)).numpy()
    dst, hit = M.warp_in(y.numpy(), uv.numpy(), rows, 16, 16, to_rgb)
    grey = y.numpy()[..., None].repeat(3, -1)
    ay, off = to_rgb[0, 0], to_rgb[0, 3] + 128.0 * (to_rgb[0, 1] + to_rgb[0, 2])
    want, hit_rgb = R.warp_in(grey, rows, 16, 16, scale=(ay,) * 3, shift=(off,) * 3)          # ay V + off in byte units where hit
    want = np.where(hit_rgb[:, None], want * 2 / 255 - 1, -1.0)
    assert np.array_equal(hit, hit_rgb) and hit.any() and not hit.all()
    assert np.abs(dst - want).max() <= 1e-12 and np.abs(dst[:, 0] - dst[:, 1]).max() <= 1e-12 and np.abs(dst[:, 0] - dst[:, 2]).max() <= 1e-12


# ---- what the GPU cases rely on ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NC.SPECS))
def test_gpu_cases_keep_their_margins_blocks_and_variances(name):
    c, ref = NC.case(name), NC.reference(name)
    assert ref["margin"] >= NC.MARGIN, f"{name}: a pixel centre lies {ref['margin']:.2e} from a region edge"
    N = c["x"].size(0)
    assert 3 <= N <= 4 and tuple(c["y"].shape) == (N, NC.H, NC.W) and tuple(c["uv"].shape) == (N, NC.H // 2, NC.W // 2, 2)
    if name in NC.ROTATED:                                                # partial chroma blocks of every size
        assert set(np.unique(ref["count"])) == {0, 1, 2, 3, 4}, (name, np.unique(ref["count"]))
    for n in range(N):
        S0 = ref["sums"][n, 0]
        if n in c["by_rule"]:
            assert ref["rows"][n].tolist() == [[1.0, 0.0]] * 3 and (S0 == 0.0 or not ref["valid"][n])
            continue
        assert ref["valid"][n] and abs(S0 - NC.MIN_WEIGHT) >= 1.0 and S0 > NC.MIN_WEIGHT, f"{name}: frame {n} has S0 = {S0:.2f}"
        assert (ref["var_b"][n] >= 100.0).all(), (name, n, ref["var_b"][n])
        if c["kind"] == "constant":                                       # the rule var_q <= min_sigma^2 decides: g = 1 exactly
            assert (ref["var_q"][n] <= 1e-6).all() and (ref["rows"][n, :, 0] == 1.0).all()
            continue
        assert (ref["var_q"][n] >= 100.0).all(), (name, n, ref["var_q"][n])
        ratio = np.sqrt(ref["var_b"][n] / ref["var_q"][n])
        if c["kind"] == "small":                                          # the cap decides, and from far away
            assert (ratio >= 1.25 * NC.MAX_GAIN).all() and (ref["rows"][n, :, 0] == NC.MAX_GAIN).all()
        assert (np.abs(ratio / NC.MAX_GAIN - 1.0) > 0.01).all() and (np.abs(ratio * NC.MAX_GAIN - 1.0) > 0.01).all(), (name, n, ratio)
        assert (np.abs(ref["rows"][n, :, 1]) < 256.0).all()
    if c["matte"] is not None:
        zero = (ref["m"] == 0) & ref["region"]
        assert zero.any() and ((ref["m"] > 0) & (ref["m"] < 1)).any()
    to_rgb, _ = NC.coeffs(**c["colour"])
    raw = M.fields(c["y"].numpy(), c["uv"].numpy()) @ to_rgb[:, :3].T + to_rgb[:, 3]
    out_of_gamut = float(((raw < -0.5) | (raw > 255.5)).any(-1).mean())
    assert out_of_gamut > 0.3 if name == "raw bytes" else out_of_gamut < 0.3, (name, out_of_gamut)


# ---- the C boundary ----------------------------------------------------------------------------------------------------------------
NEW = ("spk_frames_nv12_to_f32_sim", "spk_frames_paste_nv12_sim", "spk_paste_colour_match_nv12_sim")


def test_header_and_ctypes_agree_on_the_new_entries(pkg):
    L = pkg._lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spk.h")).read(), flags=re.S)
    lib = L.lib()
    ctype = {"int": "c_int", "int64_t": "c_long", "float": "c_float", "double": "c_double", "size_t": "c_ulong"}
    for name in NEW:
        decl = re.search(name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert decl, f"{name} is not declared in include/spk.h"
        params = [p.strip() for p in decl.group(1).split(",")]
        assert name in L.exported_symbols() and len(getattr(lib, name).argtypes) == len(params), name
        for p, t in zip(params, getattr(lib, name).argtypes):             # pointers travel as void*, scalars by their C type
            assert t.__name__ == ("c_void_p" if "*" in p else ctype[p.split()[0]]), (name, p, t)
    # the statistics take the paste's arguments up to the matte, then their own in the order of the RGB form
    paste, match, rgb = (getattr(lib, n).argtypes for n in ("spk_frames_paste_nv12_sim", "spk_paste_colour_match_nv12_sim", "spk_paste_colour_match_sim"))
    assert list(match[:len(paste) - 2]) == list(paste[:-2]) and list(match[len(paste) - 2:]) == list(rgb[-7:])


def test_entry_refusals_need_no_device(pkg):
    """Every refusal of the three entry points happens before a launch: -1 and a message, on a machine without a GPU."""
    lib = pkg._lib.lib()
    p = 4096                     # any non-null, aligned address: the arguments are refused before anything is read or launched
    nan, inf = float("nan"), float("inf")
    per = lib.spk_paste_colour_match_workspace_bytes(1)

    def way_in(src=p, y=p, uv=p, sim=p, N=1, Hs=4, Ws=4, H=8, W=8, yi=64, yr=8, ui=32, ur=8, std=601, full=0, **_):
        return lib.spk_frames_nv12_to_f32_sim(y, yi, yr, uv, ui, ur, N, H, W, sim, 0, std, full, src, Hs, Ws, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, None)

    def paste(src=p, y=p, uv=p, sim=p, N=1, Hs=4, Ws=4, H=8, W=8, yi=64, yr=8, ui=32, ur=8, std=601, full=0, feather=0.0, lo=-1.0, k=127.5,
              matte=None, mf=0):
        return lib.spk_frames_paste_nv12_sim(src, N, Hs, Ws, y, yi, yr, uv, ui, ur, H, W, sim, std, full, feather, lo, k, matte, mf, None, None)

    def match(src=p, y=p, uv=p, sim=p, N=1, Hs=4, Ws=4, H=8, W=8, yi=64, yr=8, ui=32, ur=8, std=601, full=0, feather=0.0, lo=-1.0, k=127.5,
              matte=None, mf=0, gain=2.0, sigma=1.0, weight=16.0, out=p, ws=p, wsb=None):
        wsb = per * max(N, 1) if wsb is None else wsb
        return lib.spk_paste_colour_match_nv12_sim(src, N, Hs, Ws, y, yi, yr, uv, ui, ur, H, W, sim, std, full, feather, lo, k, matte, mf, gain,
                                                   sigma, weight, out, ws, wsb, None)

    surface = (dict(src=None), dict(y=None), dict(uv=None), dict(sim=None), dict(N=0), dict(Hs=0), dict(Ws=0), dict(H=0), dict(W=0), dict(H=7),
               dict(W=9), dict(uv=p + 1), dict(ur=9), dict(N=2, ui=33), dict(yr=7), dict(ur=6), dict(W=0x7ffffffe), dict(std=2020), dict(std=0),
               dict(full=2), dict(full=-1))
    blend = (dict(feather=-0.5), dict(feather=nan), dict(feather=inf), dict(k=0.0), dict(lo=nan), dict(k=inf), dict(matte=p, mf=0),
             dict(matte=p, mf=2), dict(matte=p, mf=-1), dict(N=3, matte=p, mf=2), dict(mf=1), dict(N=2, mf=2))
    for f, bads in ((way_in, surface), (paste, surface + blend), (match, surface + blend)):
        for bad in bads:
            assert f(**bad) == -1, (f.__name__, bad)
            assert lib.spk_last_error(), bad
        assert f(std=2020) == -1 and b"standard" in lib.spk_last_error()
        assert f(H=6, W=9) == -1 and b"even" in lib.spk_last_error()
        assert f(sim=None) == -1 and b"transform" in lib.spk_last_error()
    for bad in (dict(N=2, yi=63), dict(N=2, ui=30), dict(N=2, yi=0), dict(N=2, ui=-32), dict(N=2, H=0x7ffffffe)):      # a written surface
        assert paste(**bad) == -1 and b"overlap" in lib.spk_last_error(), bad
    for f in (way_in, match):                                             # a read one
        assert f(N=2, yi=-64) == -1 and b"negative" in lib.spk_last_error()
    for bad in (dict(gain=0.99), dict(gain=nan), dict(gain=inf), dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf), dict(weight=-1.0),
                dict(weight=nan), dict(weight=inf), dict(out=None), dict(ws=None), dict(wsb=per - 1), dict(wsb=0), dict(N=2, wsb=per),
                dict(ws=p + 4)):
        assert match(**bad) == -1, bad
        assert lib.spk_last_error(), bad
    assert match(gain=0.5) == -1 and b"max_gain" in lib.spk_last_error()
    assert match(wsb=8) == -1 and b"workspace" in lib.spk_last_error()


# ---- the launchers: what is refused before a device is touched ------------------------------------------------------------------------
def test_launchers_refuse_bad_arguments_before_any_device_use(pkg):
    ops, SpkError = pkg.ops, pkg._lib.SpkError
    x, surf = torch.zeros(2, 3, 4, 6), torch.zeros(2, 12, 8, dtype=torch.uint8)
    pair = (torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 4, 4, 2, dtype=torch.uint8))
    good = [[1, 0, 0, 0], [0.5, 0.5, 1, 2]]
    outs = (lambda **kw: ops.frames_paste_nv12_aligned(x, surf, good, **kw), lambda **kw: ops.paste_colour_match_nv12(x, pair, good, **kw))
    every = outs + (lambda **kw: ops.frames_from_nv12_aligned(surf, 4, good, **kw),)
    for f in every:
        with pytest.raises(ValueError, match="standard"):
            f(standard="bt2020")
        with pytest.raises(ValueError, match="full_range"):
            f(full_range=2)
    for f in outs:
        with pytest.raises(ValueError, match="feather"):
            f(feather=-1)
        with pytest.raises(ValueError):
            f(value_range=(1, 1))
        for bad in (torch.zeros(4), torch.zeros(6, 4), torch.zeros(3, 4, 6), torch.zeros(4, 6, dtype=torch.float64), [[0.0] * 6] * 4):
            with pytest.raises(ValueError, match="matte"):
                f(matte=bad)
    for bad in (torch.zeros(2, 3), torch.zeros(3, 3, 2), torch.zeros(2, 3, 2, dtype=torch.float64), [[1.0, 0.0]] * 3):
        with pytest.raises(ValueError, match="colour"):
            ops.frames_paste_nv12_aligned(x, surf, good, colour=bad)
    for kw in (dict(max_gain=0.5), dict(max_gain=float("nan")), dict(min_sigma=-1), dict(min_weight=float("inf"))):
        with pytest.raises(ValueError, match="max_gain|min_sigma"):
            ops.paste_colour_match_nv12(x, surf, good, **kw)
    bad_rows = [[1, 0, 0, 0], [float("nan"), 0, 0, 0]]
    for f in (lambda: ops.frames_from_nv12_aligned(surf, 4, bad_rows), lambda: ops.frames_paste_nv12_aligned(x, surf, bad_rows),
              lambda: ops.paste_colour_match_nv12(x, surf, [[1, 0, 0, 0]] * 3), lambda: ops.frames_from_nv12_aligned(surf, 4, [[0.01, 0, 0, 0]] * 2)):
        with pytest.raises(ValueError, match="sim"):
            f()
    for f in (lambda: ops.frames_from_nv12_aligned(torch.zeros(2, 11, 8, dtype=torch.uint8), 4, good),          # 11 rows are no 3H/2
              lambda: ops.frames_from_nv12_aligned(surf.float(), 4, good), lambda: ops.frames_from_nv12_aligned(surf, 0, good),
              lambda: ops.frames_from_nv12_aligned(surf, 4, good, channel_order="gbr"), lambda: ops.frames_from_nv12_aligned(surf, 4, good, std=0),
              lambda: ops.frames_paste_nv12_aligned(x, surf[:1], good), lambda: ops.frames_paste_nv12_aligned(x[:, :2], surf, good),
              lambda: ops.paste_colour_match_nv12(x, (pair[0], pair[1][:, :2]), good)):
        with pytest.raises(ValueError):
            f()
    # well-formed arguments: there is no CPU path
    for f in (lambda: ops.frames_from_nv12_aligned(surf, 4, good), lambda: ops.frames_from_nv12_aligned(pair, (4, 6), good, channel_order="bgr"),
              lambda: ops.frames_paste_nv12_aligned(x, surf, good, matte=torch.zeros(4, 6), colour=torch.zeros(2, 3, 2)),
              lambda: ops.paste_colour_match_nv12(x, pair, good, matte=torch.zeros(2, 4, 6))):
        with pytest.raises(SpkError, match="HIP|device|CPU"):
            f()
