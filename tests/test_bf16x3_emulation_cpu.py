"""The split-precision reference (tests/bf16x3_emulation.py) checks itself, without a GPU: it really truncates to 16 bits, it
notices a missing term, its x2 images are the bilinear / upfirdn2d ones, its bound separates a wrong ``lo`` half on a few
positions from fp32 summation noise, and the case tables of tests/test_bf16x3_branches_gpu.py still reach every branch of
csrc/conv3x3_bf16x3.hip they are named for (a retune of the kernel's tile choice fails HERE, not silently un-covers a branch)."""
import pytest
import torch
import torch.nn.functional as F

import bf16x3_emulation as E
from oracle.weights_recipe import recipe_input, recipe_tensor

ALL_PLAIN = [(c, False) for c in E.PLAIN_CASES] + [(c, True) for c in E.PLAIN_MODULATED]
ALL_X2 = [(c, f, False) for c in E.X2_CASES for f in (False, True)] + [(c, f, True) for c, f in E.X2_MODULATED]


@pytest.mark.parametrize("Cin", [16, 40, 128])
def test_emulation_truncates_to_16_bits_and_needs_every_term(Cin):
    x = recipe_input(f"bfe.x.{Cin}", (2, Cin, 12, 12))
    w = recipe_tensor(f"bfe.w.{Cin}", (24, Cin, 3, 3), (9 * Cin) ** -0.5)
    ref = F.conv2d(x.double(), w.double(), padding=1)
    err = E.rel_l2(E.conv_emu(x, w), ref)
    assert 1e-6 < err < 1e-5, err                    # the 2^-16 operand truncation: there, and no more than that
    assert E.rel_l2(E.conv_emu(x, w, terms=("hh", "hl")), ref) > 5e-4           # c(xl, wh) left out
    assert E.rel_l2(E.conv_emu(x, w, terms=("hh", "lh")), ref) > 5e-4           # c(xh, wl) left out
    f32 = E.rel_l2(F.conv2d(x, w, padding=1), ref)
    assert f32 < 1e-6 and E.rel_l2(E.conv_emu(x, w, dtype=torch.float32), E.conv_emu(x, w)) < 1e-6      # summation noise is far below it


def test_split_is_two_round_to_nearest_even_conversions():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.14159274, 0.0, 1e-30])
    hi, lo = E.split(t)
    assert hi.tolist()[:4] == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]      # ties go to the even mantissa
    assert torch.equal(hi, hi.to(torch.bfloat16).float()) and torch.equal(lo, lo.to(torch.bfloat16).float())
    assert ((hi.double() + lo.double() - t.double()).abs() <= t.double().abs() * 2.0 ** -16).all()


@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (1, 2, 1, 2), (2, 5, 4, 8), (1, 3, 9, 5)])
def test_upsample_emu_equals_bilinear_and_upfirdn2d(shape):
    x = recipe_input(f"bfe.up.{shape}", shape)
    tol = 2e-6 * max(1.0, float(x.abs().max()))
    ref = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False)
    for exact in (False, True):
        assert float((E.upsample_emu(x, False, exact).double() - ref).abs().max()) <= tol
    # upfirdn2d(up = 2, [1,3,3,1] * 4 / 64, pad (2,1)), as tests/test_wino_gpu.py::test_upsample2x_zero_border_equals_upfirdn2d builds it
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64)
    k = (k1[:, None] * k1[None, :]) / 64.0 * 4.0
    C = shape[1]
    up = torch.zeros(shape[0], C, 2 * shape[2], 2 * shape[3], dtype=torch.float64)
    up[:, :, ::2, ::2] = x.double()
    ref = F.conv2d(F.pad(up, (2, 1, 2, 1)), k.flip(0, 1).view(1, 1, 4, 4).repeat(C, 1, 1, 1), groups=C)
    for exact in (False, True):
        assert float((E.upsample_emu(x, True, exact).double() - ref).abs().max()) <= tol
    # the two orders of arithmetic differ by fp32 rounding, and somewhere they do differ (else the x2 term of the bound is idle)
    if shape[2] * shape[3] >= 32:
        assert not torch.equal(E.upsample_emu(x, False), E.upsample_emu(x, False, True))


def test_pack_image_layout():
    """One element, by hand: channel co = 70 (tile 1, row 6), ci = 27 (chunk 1, k-group 1, slot 3), tap 5."""
    w = recipe_tensor("bfe.pack", (72, 40, 3, 3), 1.0)
    img = E.pack_image(w).view(torch.bfloat16).view(2, 3, 2, 9, 2, 64, 8)
    hi, lo = E.split(w)
    assert float(img[1, 1, 0, 5, 1, 6, 3]) == float(hi[70, 27, 1, 2]) and float(img[1, 1, 1, 5, 1, 6, 3]) == float(lo[70, 27, 1, 2])
    assert float(img[1, 2, :, :, 1].abs().max()) == 0 and float(img[1, :, :, :, :, 8:].abs().max()) == 0      # ci >= 40, co >= 72
    # the data-gradient operator: rows are the forward conv's input channels, taps turned by 180 degrees
    imt = E.pack_image(w, True).view(torch.bfloat16).view(1, 5, 2, 9, 2, 64, 8)
    assert float(imt[0, 4, 0, 5, 0, 27, 6]) == float(hi[70, 27, 1, 0])          # co' = 27, ci' = 70 = 4*16 + 6, tap 5 <- tap 3
    assert E.pack_image(w).numel() == 2 * 3 * 2 * 9 * 2 * 64 * 8 * 2


def test_case_tables_cover_every_branch():
    plain = [E.geometry(B, H, W, Cin) for B, Cin, _, H, W in E.PLAIN_CASES]
    x2 = [E.geometry(B, 2 * Hs, 2 * Ws, Cin, x2=True) for B, Cin, _, Hs, Ws in E.X2_CASES]
    assert all(g["ok"] for g in plain + x2)

    def has(gs, **want):
        return any(all((v(g[k]) if callable(v) else g[k] == v) for k, v in want.items()) for g in gs)

    for gs in (plain, x2):                               # on BOTH paths
        assert has(gs, rounds=2) and has(gs, rounds=3)
        for n in (1, 2, 3):
            assert has(gs, n_chunks=n), n
        assert has(gs, n_chunks=lambda n: n >= 4)
        assert has(gs, n_chunks=lambda n: n > 1, ci_last=lambda c: c < 8)        # the second k-group of the last chunk dead
        assert has(gs, n_chunks=lambda n: n > 1, ci_last=8)
        assert has(gs, n_chunks=lambda n: n > 1, ci_last=lambda c: 8 < c < 16)   # the last chunk reaches into the second k-group
        assert has(gs, TB=1) and has(gs, TB=lambda t: t > 1, ragged_b=True)
        assert has(gs, staged=True) and has(gs, staged=False)
    assert has(x2, s_rounds=1) and has(x2, s_rounds=2)
    assert has(x2, rounds=2, TB=lambda t: t > 1)                                 # tb * SPLANE source addressing, 8x8-class planes
    assert has(x2, s_rounds=2, ragged_b=True, tiles_b=lambda t: t > 1)           # the tbc clamp of a ragged LAST image group
    assert any(g["TB"] < g["TB_full"] for g in plain) and any(g["TB"] < g["TB_full"] for g in x2)      # TB halved by the 768-item limit
    assert any(g["staged"] and (g["partial_x"] or g["partial_y"]) for g in plain)
    assert any(not g["staged"] and g["partial_x"] and g["partial_y"] for g in plain)
    assert any(g["staged"] and g["partial_x"] for g in x2) and any(not g["staged"] and g["partial_x"] and g["partial_y"] for g in x2)
    assert has(plain, TW=2, staged=False) and has(plain, TW=4, staged=True) and has(plain, TW=1, TH=1)
    # the cases named for a branch still hit it
    g = E.geometry(3, 8, 8, 32)
    assert (g["TB"], g["TB_full"], g["rounds"], g["n_chunks"], g["staged"], g["ragged_b"]) == (2, 4, 2, 2, True, True)
    g = E.geometry(5, 4, 4, 24)
    assert (g["TB"], g["TB_full"], g["ci_last"]) == (8, 16, 8)
    g = E.geometry(9, 2, 2, 64)
    assert (g["TW"], g["TB"], g["n_chunks"], g["staged"]) == (2, 16, 4, False)
    g = E.geometry(18, 2, 4, 16, x2=True)
    assert (g["TB"], g["s_rounds"], g["tiles_b"], g["ragged_b"], g["n_chunks"]) == (16, 2, 2, True, 1)
    g = E.geometry(5, 2, 2, 21, x2=True)
    assert (g["s_rounds"], g["staged"], g["n_chunks"], g["ci_last"]) == (2, False, 2, 5)
    g = E.geometry(3, 8, 8, 48, x2=True)
    assert (g["TB"], g["rounds"], g["s_rounds"], g["n_chunks"]) == (2, 2, 1, 3)
    assert E.geometry(2, 6, 10, 29, x2=True)["ci_last"] == 13 and E.geometry(1, 18, 18, 72, x2=True)["ci_last"] == 8
    # a misaligned y / y_pre / noise takes the dword epilogue at W % 4 == 0 (the forced-dword case)
    assert E.geometry(3, 8, 8, 32)["staged"] and not E.geometry(3, 8, 8, 32, aligned=False)["staged"]
    # every modulated subset: one TB > 1 case with ragged B on each path, one x2 + FIR case
    assert all(c in E.PLAIN_CASES for c in E.PLAIN_MODULATED) and all(c in E.X2_CASES for c, _ in E.X2_MODULATED)
    assert any(E.geometry(c[0], c[3], c[4])["ragged_b"] for c in E.PLAIN_MODULATED)
    assert any(E.geometry(c[0], 2 * c[3], 2 * c[4], x2=True)["ragged_b"] for c, _ in E.X2_MODULATED) and any(f for _, f in E.X2_MODULATED)


def _check_bound(ref, Cin):
    """The bound comes from the reference alone: it is at fp32-summation level -- below the truncation error at small Cin, which
    is what makes the test sharper than an fp64 check -- and the fp32 emulation itself stays inside the single-pixel factor."""
    assert E.chain_floor(Cin) <= ref["bound"] < 1e-5, ref["bound"]
    worst = float((ref["y32"] - ref["y"]).abs().max())
    assert worst <= E.MAX_FACTOR * ref["bound"] * E.rms(ref["y"]), (worst, ref["bound"], E.rms(ref["y"]))


@pytest.mark.parametrize("case,modulated", ALL_PLAIN)
def test_plain_bounds_and_sensitivity(case, modulated):
    ref = E.plain_reference(case, modulated)
    B, Cin, Cout, H, W = case
    _check_bound(ref, Cin)
    t = ref["inputs"]
    x = E.modulate(t["x"], t["s"]) if modulated else t["x"]
    epi = dict(out_scale=E.OUT_SCALE, bias=t["bias"], slope=E.SLOPE)
    if modulated:
        epi.update(demod=t["demod"], act_gain=E.ACT_GAIN)
    # a wrong lo half at the halo ring of ONE image (the last: the ragged image group where there is one) is above the bound
    lo = E.split(x)[1]
    ring = torch.ones(H, W, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    bad = lo.clone()
    bad[B - 1][:, ring] = 0
    err = E.rel_l2(E.epilogue_emu(E.conv_emu(x, t["w"], x_lo=bad), **epi)[1], ref["y"])
    assert err > 2 * ref["bound"], (err, ref["bound"])
    print(f"{case} modulated={modulated}: bound {ref['bound']:.2e}; lo = 0 on the ring of one image {err:.2e}", end="")
    # ... and so is one in the second k-group of the ragged last chunk
    g = E.geometry(B, H, W, Cin)
    if g["ci_last"] > 8:
        bad = lo.clone()
        bad[:, (g["n_chunks"] - 1) * 16 + 8:] = 0
        err = E.rel_l2(E.epilogue_emu(E.conv_emu(x, t["w"], x_lo=bad), **epi)[1], ref["y"])
        assert err > 2 * ref["bound"], (err, ref["bound"])
        print(f"; in the second k-group of the last chunk {err:.2e}", end="")
    print()


@pytest.mark.parametrize("case,fir,modulated", ALL_X2)
def test_x2_bounds_and_sensitivity(case, fir, modulated):
    ref = E.x2_reference(case, fir, modulated)
    B, Cin, Cout, Hs, Ws = case
    _check_bound(ref, Cin)
    t = ref["inputs"]
    epi = dict(bias=t["bias"], noise_w=t["noise_w"], noise=t["noise"], slope=E.SLOPE, style=t["style"])
    x = t["x"]
    if modulated:
        x = E.modulate(x, t["s"])
        epi.update(out_scale=E.OUT_SCALE, demod=t["demod"], act_gain=E.ACT_GAIN)
    img = E.upsample_emu(x, fir)
    lo = E.split(img)[1]
    ring = torch.ones(2 * Hs, 2 * Ws, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    bad = lo.clone()
    bad[B - 1][:, ring] = 0
    err = E.rel_l2(E.epilogue_emu(E.conv_emu(img, t["w"], x_lo=bad), **epi)[1], ref["y"])
    assert err > 2 * ref["bound"], (err, ref["bound"])
    print(f"{case} fir={fir} modulated={modulated}: bound {ref['bound']:.2e}; lo = 0 on the ring of one image {err:.2e}", end="")
    g = E.geometry(B, 2 * Hs, 2 * Ws, Cin, x2=True)
    if g["ci_last"] > 8:
        bad = lo.clone()
        bad[:, (g["n_chunks"] - 1) * 16 + 8:] = 0
        err = E.rel_l2(E.epilogue_emu(E.conv_emu(img, t["w"], x_lo=bad), **epi)[1], ref["y"])
        assert err > 2 * ref["bound"], (err, ref["bound"])
        print(f"; in the second k-group of the last chunk {err:.2e}", end="")
    print()
    # the FIR form differs from the bilinear one at the border only, and there it does
    if fir:
        other = E.upsample_emu(x, False)
        assert torch.equal(img[..., 1:-1, 1:-1], other[..., 1:-1, 1:-1]) and not torch.equal(img, other)


@pytest.mark.parametrize("case", E.DGRAD_CASES)
def test_dgrad_reference(case):
    ref = E.dgrad_reference(case)
    _check_bound(ref, case[2])
    assert 1e-6 < E.rel_l2(ref["y"], ref["autograd"]) < 1e-5      # the transposed, flipped operator IS the data gradient
