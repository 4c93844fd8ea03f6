"""The case table of tests/wgrad_cases.py held to the branches it is named for, without a GPU: ``spk_conv2d_wgrad_launch_form`` (the
launch path's own statements, nothing launched) answers which kernel, geometry and reducer every case takes; the union must equal
the branch list below; ``spk_conv2d_wgrad_workspace_bytes`` must cover what each launcher asks for; no bound is looser than the
2e-5 of the older tests; the checks of tests/test_wgrad_branches_gpu.py are shown to see the faults they exist for, by seeding each
into the fp64 reference; the reducers' float32 emulation (tests/wgrad_reduce_ref.py) is held to the fp64 sum; and the shapes of
tests/test_backward_gpu.py are asked which form they take."""
import importlib

import numpy as np
import pytest
import torch

import wgrad_cases as Wc
import wgrad_reduce_ref as Rr


@pytest.fixture(scope="module")
def L():
    Wc.require_default_dispatch()
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")._lib


@pytest.fixture(scope="module")
def forms(L):
    return {c["name"]: Wc.query(c, L) for c in Wc.CASES}


# (kernel [. k x k s stride for the tap kernel and the GEMM], input stage, reducer)
REQUIRED = {
    ("tap.3x3s1", "plain", "dword"), ("tap.3x3s1", "plain", "vec"), ("tap.3x3s1", "affine", "vec"),
    ("tap_fixed", "affine", "vec"), ("tap_fixed", "affine", "dword"),
    ("pipe", "plain", "vec"), ("pipe", "plain", "dword"),
    ("wide16", "plain", "vec"), ("wide16", "plain", "dword"), ("wide16", "affine", "vec"), ("wide16", "bscale", "vec"),
    ("wide8", "plain", "vec"), ("wide8", "plain", "dword"), ("wide8", "plain", "deep"), ("wide8", "affine", "vec"), ("wide8", "affine", "deep"),
    ("wide8", "bscale", "vec"),
    ("s2_16", "plain", "vec"), ("s2_16", "affine", "vec"), ("s2_8", "plain", "vec"), ("s2_8", "affine", "vec"),
    ("tap.3x3s2", "plain", "vec"), ("tap.3x3s2", "affine", "vec"),
    ("up", "bilinear", "vec"), ("up", "fir+bscale", "vec"),
    ("gemm1x1.1x1s1", "plain", "dword"), ("gemm1x1.1x1s1", "plain", "vec"), ("gemm1x1.1x1s1", "plain", "deep"),
    ("gemm1x1.1x1s1", "affine", "vec"), ("gemm1x1.1x1s1", "affine", "dword"),
    ("gemm1x1.1x1s2", "plain", "vec"), ("gemm1x1.1x1s2", "affine", "vec"), ("gemm1x1.1x1s2", "affine", "dword"),
    ("gemm1x1_dma", "plain", "vec"), ("gemm1x1_dma", "affine", "vec"),
    ("tap.1x1s1", "plain", "vec"), ("tap.1x1s1", "affine", "dword"), ("tap.1x1s2", "plain", "vec"), ("tap.1x1s2", "affine", "vec"),
    ("tap.4x4s2", "plain", "vec"),
    ("stem", "plain", "dword"),                    # (147 input-side columns: never a multiple of four)
    ("tap.7x7s2", "plain", "dword"), ("tap.7x7s2", "plain", "vec"), ("tap.7x7s2", "affine", "dword"),
    ("wino", "plain", "vec"),
}


@pytest.mark.parametrize("c", Wc.CASES, ids=lambda c: c["name"])
def test_case_reaches_the_form_it_declares(forms, c):
    form = forms[c["name"]]
    got = {k: form[k] for k in c["declares"]}
    assert got == c["declares"], (c["name"], form)
    assert form["mode"] == c["mode"] and form["fold"] == c["fold"]
    assert form["taps"] == (1 if form["kernel"] == "stem" else c["k"] * c["k"])
    assert form["grid_x"] > 0 and form["grid_y"] > 0 and form["grid_z"] > 0 and 0 < form["lds_bytes"] <= 160 * 1024
    assert 1 <= form["splits"] <= form["n_tiles"] <= form["splits"] * form["tiles_per_split"]
    if c["splits"] and form["kernel"] not in ("stem", "wino"):
        assert form["splits"] <= c["splits"]


def test_required_branches_are_covered(forms):
    have = {Wc.coverage_key(c, forms[c["name"]]) for c in Wc.CASES}
    assert REQUIRED <= have, sorted(REQUIRED - have)
    assert have <= REQUIRED, f"new branches reached: list them in REQUIRED so that dropping their case fails here: {sorted(have - REQUIRED)}"


def test_every_case_is_needed(forms):
    """Every case is the only one behind some required key or some named edge: ``EDGES`` names one case per edge, each case at most
    once there, and together with the first case of every REQUIRED key they make up the whole table."""
    named = [n for names in EDGES.values() for n in names]
    assert len(named) == len(set(named)) and set(named) <= set(Wc.BY_NAME), sorted(set(named) - set(Wc.BY_NAME))
    keys = {}
    for c in Wc.CASES:
        keys.setdefault(Wc.coverage_key(c, forms[c["name"]]), []).append(c["name"])
    sole = {names[0] for names in keys.values() if len(names) == 1}
    assert sole | set(named) == set(Wc.BY_NAME), sorted(set(Wc.BY_NAME) - sole - set(named))


# the items of the branch list that the (kernel, input stage, reducer) key does not spell out: edge -> the cases that are there for it
EDGES = {
    "tap 3x3 s1: TB > 1 with a ragged image group, at a 2x2 and a 5x3 plane": ["tap.s1.2x2", "tap.s1.5x3"],
    "tap 3x3 s1 affine at a 4x4 plane": ["tap.s1.affine.4x4"],
    "fixed geometry: W % 4 != 0, a misaligned g, a misaligned x": ["fixed.w13", "fixed.misg", "fixed.misx"],
    "pipe: one workgroup walks every tile, misaligned at W % 4 == 0, ragged channel blocks": ["pipe.w13.split1", "pipe.misg", "pipe.misx.ragged"],
    "wide: partial tiles, W = 8 and 12, groups with own and shared input, fold, Cout % 64 == 0 grouped, ragged ungrouped": [
        "wide16.plain.partial", "wide16.affine.g2.fold", "wide16.affine.shared", "wide16.bscale", "wide8.plain.w8", "wide8.plain.w12",
        "wide8.affine.ragged", "wide8.affine.g3", "wide8.plain.g4.fold.shared", "wide8.bscale", "wide8.affine.g2.fold.deep", "wide16.plain.misdw"],
    "s2: Cout 96 / 128 / 160, grouped, and the four fallbacks to the tap kernel": [
        "s2_16.plain.c96", "s2_16.affine.c160", "s2_8.plain.c128", "s2_8.affine.g2.fold", "s2_16.plain.g2", "taps2.cout80", "taps2.w4", "taps2.odd",
        "taps2.misx"],
    "up: the smallest plane, a partial x tile, ragged channels": ["up.bilinear.16x4", "up.bilinear.w24", "up.fir.16x4", "up.fir.w24"],
    "gemm1x1: S x mode, four block shapes, ragged channels, a short last split, n_tiles < 4, misaligned": [
        "g1.s1.plain.m2n2", "g1.s1.affine.m1n1", "g1.s1.plain.m2n1.short", "g1.s1.affine.m1n2", "g1.s1.mis", "g1.s2.plain.m1n1", "g1.s2.affine.m2n2",
        "g1.s2.plain.m1n2.g2", "g1.s2.affine.m2n1", "g1.s1.slabs32.dword"],
    "gemm1x1_dma: four block shapes, one k-tile, k-tiles across images, grouped with fold": [
        "dma.m1n1.onetile", "dma.m1n2.affine", "dma.m2n1", "dma.m2n2.affine", "dma.g2.fold"],
    "tap 1x1: 5x5 planes, 1x1 planes with TB = 64, an odd input at stride 2": ["tap1.s1.5x5", "tap1.s1.1x1", "tap1.s2.odd.affine"],
    "4x4 s2 row passes, ragged channels": ["k4.rowpass", "k4.rowpass.ragged"],
    "stem: own and shared groups, fold, a partial tile, more slabs asked for than tiles": ["stem.g1", "stem.g2.own", "stem.g2.shared.fold",
                                                                                          "stem.slabs.over"],
    "7x7 packed: Cout 40, W % 4 != 0, Cin 4, a misaligned g, affine": ["k7.cout40", "k7.w11", "k7.cin4", "k7.misg", "k7.affine"],
}


def test_edges_are_what_their_names_say(L, forms):
    C, Fm, hw = Wc.BY_NAME, forms, lambda n: Wc.out_hw(Wc.BY_NAME[n])
    for n in ("tap.s1.2x2", "tap.s1.5x3", "tap.s1.affine.4x4"):
        assert Fm[n]["TB"] > 1 and C[n]["B"] % Fm[n]["TB"] != 0 and hw(n)[1] < 8
    assert hw("tap.s1.2x2") == (2, 2) and hw("tap.s1.5x3") == (5, 3) and C["tap.s1.5x3"]["Cin"] % 64 and C["tap.s1.5x3"]["Cout"] % 64
    assert hw("fixed.w13") == (9, 13) and hw("fixed.misg")[1] % 4 == 0 and C["fixed.misg"]["misalign"] == {"g"} and C["fixed.misx"]["misalign"] == {"x"}
    assert hw("pipe.w13.split1") == (9, 13) and Fm["pipe.w13.split1"]["grid_z"] == 1 and Fm["pipe.w13.split1"]["tiles_per_split"] == Fm["pipe.w13.split1"]["n_tiles"] > 1
    assert hw("pipe.misg")[1] % 4 == 0 and C["pipe.misg"]["misalign"] and C["pipe.misx.ragged"]["Cin"] % 64 and C["pipe.misx.ragged"]["Cout"] % 64
    wide = [n for n in C if Fm[n]["kernel"] in ("wide16", "wide8")]
    for kern in ("wide16", "wide8"):
        assert {C[n]["mode"] for n in wide if Fm[n]["kernel"] == kern} == {"plain", "affine", "bscale"}
        tw = 16 if kern == "wide16" else 8
        assert any(hw(n)[1] % tw and hw(n)[0] % (64 // tw) for n in wide if Fm[n]["kernel"] == kern), kern
        assert any(C[n]["G"] > 1 and C[n]["Cout"] % 64 == 0 for n in wide if Fm[n]["kernel"] == kern)
        assert any(C[n]["G"] == 1 and C[n]["Cout"] % 64 and C[n]["Cin"] % 64 for n in wide if Fm[n]["kernel"] == kern)
        assert any(C[n]["fold"] == 2 for n in wide if Fm[n]["kernel"] == kern)
    assert {hw(n)[1] for n in wide} >= {8, 12} and any(C[n]["shared"] for n in wide) and any(C[n]["G"] > 1 and not C[n]["shared"] for n in wide)
    s2 = [n for n in C if Fm[n]["kernel"] in ("s2_16", "s2_8")]
    assert {C[n]["Cout"] for n in s2} >= {96, 128, 160} and any(C[n]["G"] > 1 and C[n]["Cout"] % 128 == 0 for n in s2)
    assert {(Fm[n]["kernel"], C[n]["mode"]) for n in s2} == {(k, m) for k in ("s2_16", "s2_8") for m in ("plain", "affine")}
    assert C["taps2.cout80"]["Cout"] < 96 and hw("taps2.w4")[1] < 8 and C["taps2.odd"]["Hs"] == 9 and hw("taps2.odd") == (5, 5) and C["taps2.misx"]["misalign"]
    for n in ("taps2.cout80", "taps2.w4", "taps2.odd", "taps2.misx"):
        assert Fm[n]["kernel"] == "tap" and C[n]["stride"] == 2 and C[n]["k"] == 3
    assert hw("up.bilinear.16x4") == hw("up.fir.16x4") == (4, 16) and hw("up.bilinear.w24")[1] == hw("up.fir.w24")[1] == 24
    assert C["up.bilinear.w24"]["Cin"] % 64 and C["up.bilinear.w24"]["Cout"] % 64
    g1 = [n for n in C if Fm[n]["kernel"] == "gemm1x1"]
    assert {(C[n]["stride"], C[n]["mode"]) for n in g1} == {(1, "plain"), (1, "affine"), (2, "plain"), (2, "affine")}
    for s in (1, 2):
        assert {(Fm[n]["MT"], Fm[n]["NT"]) for n in g1 if C[n]["stride"] == s} == {(1, 1), (1, 2), (2, 1), (2, 2)}, s
    assert any(C[n]["Cin"] % 64 and C[n]["Cout"] % 64 for n in g1) and any(Fm[n]["n_tiles"] < 4 for n in g1)
    assert any(Fm[n]["n_tiles"] % Fm[n]["tiles_per_split"] and Fm[n]["splits"] > 1 for n in g1)
    assert C["g1.s1.mis"]["misalign"] and Wc.query(dict(C["g1.s1.mis"], misalign=frozenset()), L)["kernel"] == "gemm1x1_dma"
    dma = [n for n in C if Fm[n]["kernel"] == "gemm1x1_dma"]
    assert {(Fm[n]["MT"], Fm[n]["NT"]) for n in dma} == {(1, 1), (1, 2), (2, 1), (2, 2)} and any(Fm[n]["n_tiles"] == 1 for n in dma)
    assert any((hw(n)[0] * hw(n)[1] // 32) % 2 == 1 and C[n]["B"] > 1 and Fm[n]["splits"] > 1 for n in dma) and any(C[n]["G"] > 1 and C[n]["fold"] > 1 for n in dma)
    assert hw("tap1.s1.5x5") == (5, 5) and (Fm["tap1.s1.1x1"]["TB"], hw("tap1.s1.1x1")) == (64, (1, 1)) and C["tap1.s1.1x1"]["B"] % 64
    assert C["tap1.s2.odd.affine"]["Hs"] % 2 == 1 and {(C[n]["stride"], C[n]["mode"]) for n in C if Fm[n]["kernel"] == "tap" and C[n]["k"] == 1} == {
        (1, "plain"), (1, "affine"), (2, "plain"), (2, "affine")}
    assert Fm["k4.rowpass"]["grid_y"] == 4 * 1 and Fm["k4.rowpass.ragged"]["grid_y"] == 4 * 2 and C["k4.rowpass.ragged"]["Cout"] % 64
    stem = [n for n in C if Fm[n]["kernel"] == "stem"]
    assert any(C[n]["G"] > 1 and C[n]["shared"] and C[n]["fold"] == 2 for n in stem) and any(C[n]["G"] > 1 and not C[n]["shared"] for n in stem)
    assert all(hw(n)[1] % 32 for n in stem) and any(hw(n)[1] > 32 for n in stem) and any(hw(n)[0] % 4 for n in stem)
    assert C["stem.slabs.over"]["splits"] > Fm["stem.slabs.over"]["n_tiles"] == Fm["stem.slabs.over"]["n_slabs"]
    assert Fm["stem.slabs.over"]["workspace_bytes"] == C["stem.slabs.over"]["splits"] * Fm["stem.slabs.over"]["slab_floats"] * 4
    assert C["k7.cout40"]["Cout"] == 40 and hw("k7.w11")[1] % 4 and C["k7.cin4"]["Cin"] == 4 and C["k7.misg"]["misalign"] == {"g"} and C["k7.affine"]["mode"] == "affine"
    for n in ("k7.misg", "k7.affine"):     # the stem form's shape, declined for the one reason the case names
        assert Wc.query(dict(C[n], misalign=frozenset(), mode="plain"), L)["kernel"] == "stem"
    # scale + accumulate meets every reducer and every kernel family; a misaligned dw sends an aligned, Cin % 4 == 0 problem to dword
    acc = [n for n in C if C[n]["accumulate"] and C[n]["scale"] != 1.0]
    assert {Fm[n]["reducer"] for n in acc} == {"dword", "vec", "deep"}
    assert {Fm[n]["kernel"] for n in acc} >= {"tap", "tap_fixed", "pipe", "wide16", "wide8", "s2_16", "up", "gemm1x1", "gemm1x1_dma", "stem"}
    assert C["wide16.plain.misdw"]["Cin"] % 4 == 0 and Fm["wide16.plain.misdw"]["reducer"] == "dword"
    assert any(Fm[n]["reducer"] == "deep" and Fm[n]["fold"] > 1 for n in C) and any(Fm[n]["reducer"] == "deep" and Fm[n]["taps"] == 1 for n in C)


@pytest.mark.parametrize("c", Wc.CASES, ids=lambda c: c["name"])
def test_workspace_query_covers_what_the_launcher_asks_for(L, forms, c):
    """spk_conv2d_wgrad_workspace_bytes is a second statement of the geometry rules: it must never answer less."""
    need = forms[c["name"]]["workspace_bytes"]
    assert need == forms[c["name"]]["n_slabs"] * forms[c["name"]]["slab_floats"] * 4 or c["name"] == "stem.slabs.over"
    assert Wc.workspace_bytes(c, L) >= need > 0
    d = Wc.dummy_desc(c, L)                # and the launcher refuses one byte less
    d.workspace_bytes = need - 1
    with pytest.raises(L.SpkError, match="workspace"):
        Wc.query(c, L, d)


@pytest.mark.parametrize("c,msg", Wc.REFUSALS, ids=[c["name"] for c, _ in Wc.REFUSALS])
def test_refusals_stay_refusals(L, c, msg):
    with pytest.raises(L.SpkError, match=msg):
        Wc.query(c, L)


def test_query_refuses_bad_arguments(L):
    assert L.lib().spk_conv2d_wgrad_launch_form(None, None) < 0
    d = Wc.dummy_desc(Wc.BY_NAME["wide8.plain.w8"], L)
    d.workspace = None
    with pytest.raises(L.SpkError, match="workspace"):
        Wc.query(None, L, d)


def test_a_set_switch_fails_with_its_name(monkeypatch):
    for name in Wc.ENV_SWITCHES:
        monkeypatch.setenv(name, "0")
        with pytest.raises(AssertionError, match=name + " is set"):
            Wc.require_default_dispatch()
        monkeypatch.delenv(name)
    Wc.require_default_dispatch()


@pytest.mark.parametrize("c", Wc.CASES, ids=lambda c: c["name"])
def test_bound_is_no_looser_than_the_older_tests(c):
    ref = Wc.reference(c)
    assert 0 < ref["bound"] <= Wc.TOL_OP, ref["bound"]
    for what, (v, lim) in Wc.figures(c, ref["dw32"]).items():      # the reference's own fp32 evaluation sits inside every limit
        assert v <= lim, (what, v, lim)


# ---- sensitivity: each fault seeded into the fp64 reference must exceed a limit by 10 x ---------------------------------------------
FAULTS = [("border_row", "wide16.plain.partial"), ("border_row", "s2_8.plain.c128"), ("taps_transposed", "pipe.w13.split1"),
          ("taps_transposed", "k4.rowpass"), ("halo_relu_shift", "fixed.w13"), ("halo_relu_shift", "taps2.misx"), ("halo_relu_shift", "k7.affine"),
          ("last_tile_lost", "pipe.w13.split1"), ("last_tile_lost", "g1.s1.plain.m2n1.short"), ("last_tile_lost", "stem.g2.shared.fold"),
          ("ragged_rows", "wide8.affine.ragged"), ("ragged_rows", "g1.s1.plain.m2n2"), ("fold_neighbour", "wide8.plain.g4.fold.shared"),
          ("bilinear_border", "up.bilinear.16x4"), ("no_g_scale", "wide8.bscale"), ("no_g_scale", "up.fir.w24")]


@pytest.mark.parametrize("fault,name", FAULTS, ids=[f"{f}-{n}" for f, n in FAULTS])
def test_checks_see_the_seeded_fault(forms, fault, name):
    c = Wc.BY_NAME[name]
    if fault == "halo_relu_shift":         # shifts of both signs: relu(shift) is neither all zero nor the shift itself
        b = Wc.inputs(c)["b"]
        assert c["mode"] == "affine" and bool((b > 0).any()) and bool((b < 0).any())
    if fault == "ragged_rows":
        assert c["Cout"] % 64
    if fault == "fold_neighbour":
        assert c["G"] // c["fold"] > 1
    fig = Wc.figures(c, Wc.chain(c, torch.float64, fault=fault, form=forms[name]))
    worst = max(v / lim for v, lim in fig.values())
    print(f"{fault} on {name}: {worst:.1f} x its limit")
    assert worst >= 10, (fault, fig)


# ---- the reducers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", Rr.CASES, ids=lambda c: c["name"])
def test_reducer_case_reaches_the_reducer_it_names(L, c):
    form = L.WgradForm()
    rc = L.lib().spk_wgrad_reduce_form(0x100000, 0x200000 + (4 if c["misalign_dw"] else 0), c["n_slabs"], c["Cout_all"], c["Cin"], c["taps"], c["fold"], form)
    L.check(rc, "spk_wgrad_reduce_form")
    assert (Rr.REDUCERS[form.reducer], form.fold, form.taps, form.n_slabs) == (c["reducer"], c["fold"], c["taps"], c["n_slabs"])


def test_reducer_table_covers_the_list():
    by = lambda r: [c for c in Rr.CASES if c["reducer"] == r]
    for r in Rr.REDUCERS:
        assert {c["taps"] for c in by(r)} >= {1, 9, 16, 49} and {c["fold"] for c in by(r)} == {1, 2, 3}, r
        assert any(c["scale"] != 1.0 and c["accumulate"] for c in by(r))
        assert r == "dword" or any(c["scale"] != 1.0 and c["accumulate"] and c["taps"] == 1 for c in by(r))      # (the 16-byte store of a 1x1)
    edges = {1, 3, 4, 7, 8, 9, 12, 31, 32, 33, 133}
    assert {c["n_slabs"] for c in by("dword")} >= edges and {c["n_slabs"] for c in by("vec")} >= edges - {32, 133} and {c["n_slabs"] for c in by("deep")} >= {32, 33, 133}
    assert any(c["Cin"] == 147 and c["taps"] == 1 for c in by("dword")) and any(c["misalign_dw"] and c["Cin"] % 4 == 0 for c in by("dword"))
    # one round of each grid: 2048 x 256 floats, 4096 x 256 float4s, 4096 x 16 float4s -- more elements than that, and a partial last round
    per = lambda c: c["Cout_all"] // c["fold"] * c["Cin"] * c["taps"]
    assert any(per(c) > 2048 * 256 and per(c) % (2048 * 256) for c in by("dword"))
    assert any(per(c) // 4 > 4096 * 256 and (per(c) // 4) % (4096 * 256) for c in by("vec"))
    assert any(per(c) // 4 > 4096 * 16 and (per(c) // 4) % (4096 * 16) for c in by("deep"))
    a, b = (Rr.BY_NAME[n] for n in Rr.SAME_ORDER)
    assert (a["reducer"], b["reducer"], b["misalign_dw"]) == ("vec", "dword", True) and np.array_equal(Rr.slabs_of(a), Rr.slabs_of(b))


@pytest.mark.parametrize("c", [c for c in Rr.CASES if "rounds" not in c["name"] and "large" not in c["name"]], ids=lambda c: c["name"])
def test_reducer_emulation_against_fp64(c):
    """The emulation is a float32 sum of n_slabs x fold terms in a tree at least 4 wide: its error against the fp64 sum stays under
    (n_slabs x fold / 4 + 4) roundings of the largest partial sum, and the documented orders are told apart from a plain running sum."""
    slabs = Rr.slabs_of(c)
    emu, ref = Rr.emulate(slabs, c["fold"], c["reducer"]), Rr.exact(slabs, c["fold"])
    assert emu.shape == ref.shape == (c["Cout_all"] // c["fold"], c["Cin"], c["taps"])
    mag = np.abs(slabs.astype(np.float64)).reshape(c["n_slabs"], c["fold"], *ref.shape[:1], c["taps"], c["Cin"]).sum((0, 1)).transpose(0, 2, 1)
    terms = c["n_slabs"] * c["fold"]
    assert np.all(np.abs(emu - ref) <= (terms / 4 + 4) * 2.0 ** -24 * mag)
    if terms == 1:
        assert np.array_equal(emu, slabs[0].transpose(0, 2, 1))
    if terms >= 12:                        # (and the order matters: the other reducer's order gives other bits)
        other = "deep" if c["reducer"] != "deep" else "vec"
        assert not np.array_equal(emu, Rr.emulate(slabs, c["fold"], other))
    if c["reducer"] != "deep":
        assert np.array_equal(emu, Rr.emulate(slabs, c["fold"], "vec" if c["reducer"] == "dword" else "dword"))


def test_reducer_checks_see_a_skipped_slab():
    """One slab skipped in the reduce: far over the fp64 limit of the GPU test (and over bit equality, trivially)."""
    for name in ("vec.n12", "deep.n33", "dword.scale.acc"):
        c = Rr.BY_NAME[name]
        ref, emu, bound = Rr.expected(c)
        slabs = Rr.slabs_of(c)
        short = Rr.emulate(np.delete(slabs, c["n_slabs"] // 2, axis=0), c["fold"], c["reducer"]) * np.float32(c["scale"])
        if c["accumulate"]:
            short = Rr.base_of(c) + short
        err = float(np.linalg.norm(short.astype(np.float64) - ref) / np.linalg.norm(ref))
        assert err >= 10 * bound, (name, err, bound)


# ---- the shapes of tests/test_backward_gpu.py: which form they take ---------------------------------------------------------------------
def _form_of(L, k, stride, B, Cin, Cout, H, W, mode="plain", G=1, up=None):
    """(H, W): the OUTPUT size, as those tests state it."""
    Hs, Ws = (H // 2, W // 2) if up else ((H, W) if stride == 1 else (2 * H, 2 * W))
    return Wc.query(Wc.case("q", k, stride, B, Cin, Cout, Hs, Ws, mode, up=up, G=G, kernel="-"), L)


def test_forms_of_the_older_wgrad_tests(L):
    kern = lambda *a, **kw: _form_of(L, *a, **kw)["kernel"]
    # test_wgrad_vs_autograd: only (3, 20, 40, 9, 13) reaches the pipelined form; its two "16x4 tiles" shapes have W % 4 == 0
    assert kern(3, 1, 3, 20, 40, 9, 13) == "pipe"
    assert kern(3, 1, 3, 24, 40, 6, 20) == "wide16" and kern(3, 1, 2, 70, 130, 12, 36) == "wide16"
    assert kern(3, 1, 2, 64, 64, 32, 32) == "wide16" and kern(3, 1, 8, 512, 512, 8, 8) == "wide8" and kern(3, 1, 1, 5, 3, 2, 2) == "tap"
    assert kern(1, 1, 2, 96, 160, 16, 16) == "gemm1x1" and kern(1, 2, 2, 64, 128, 8, 8) == "gemm1x1" and kern(1, 1, 2, 2048, 512, 1, 1) == "tap"
    assert kern(3, 2, 2, 48, 80, 10, 10) == "tap" and kern(7, 2, 2, 3, 64, 20, 20) == "stem"        # (that test states INPUT sizes: 20^2, 40^2)
    # test_wgrad_stride1_wide_form / _stride2_wide_form / _1x1_lds_dma_form / _stem_form: the forms their docstrings name
    for B, Cin, Cout, H, W, G, aff in [(2, 64, 64, 8, 8, 1, False), (3, 70, 130, 12, 12, 1, True), (2, 64, 64, 8, 8, 3, True), (2, 40, 72, 6, 8, 1, False)]:
        assert kern(3, 1, B, Cin, Cout, H, W, "affine" if aff else "plain", G) == "wide8"
    assert kern(3, 1, 2, 64, 128, 20, 16, "affine", 2) == "wide16"
    for B, Cin, Cout, H, W, G, aff in [(2, 32, 128, 16, 16, 1, False), (3, 40, 160, 10, 20, 1, True), (2, 64, 128, 8, 8, 1, False), (3, 24, 96, 6, 8, 1, True),
                                       (2, 32, 128, 12, 16, 3, True), (2, 32, 256, 8, 8, 2, False)]:
        assert kern(3, 2, B, Cin, Cout, H, W, "affine" if aff else "plain", G) == ("s2_16" if W >= 16 else "s2_8")
    for B, Cin, Cout, H, W, G, aff in [(2, 64, 64, 8, 8, 1, False), (3, 128, 64, 8, 4, 2, True), (2, 64, 128, 16, 16, 1, True), (2, 128, 256, 8, 8, 3, False),
                                       (1, 256, 128, 4, 8, 1, True), (5, 128, 128, 8, 12, 2, True)]:
        assert kern(1, 1, B, Cin, Cout, H, W, "affine" if aff else "plain", G) == "gemm1x1_dma"
    for B, Hin, Win, G in [(2, 40, 40, 1), (3, 50, 72, 2), (2, 34, 136, 4), (1, 128, 128, 2)]:
        assert kern(7, 2, B, 3, 64, Hin // 2, Win // 2, G=G) == "stem"
    # test_wgrad_of_upsampled_input_without_materialising_it
    for B, Cin, Cout, Hs, Ws in [(2, 64, 64, 16, 16), (1, 20, 40, 12, 12), (3, 70, 130, 6, 20), (2, 64, 64, 32, 32), (1, 128, 72, 10, 36), (8, 128, 64, 16, 16)]:
        assert kern(3, 1, B, Cin, Cout, 2 * Hs, 2 * Ws, up="bilinear") == "up"
