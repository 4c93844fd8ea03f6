"""The case tables of tests/direct_conv_cases.py held to the branches they are named for, without a GPU:
``spk_conv2d_launch_form`` (the launch path's own statements, nothing launched) answers which form every case takes; the union
must cover every branch listed below; no bound is looser than the 2e-5 of the older conv tests; and the checks of
tests/test_direct_conv_branches_gpu.py are shown to see the faults they exist for, by seeding each into the fp64 reference."""
import importlib

import pytest
import torch

import direct_conv_cases as D


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")._lib


@pytest.fixture(scope="module")
def forms(L):
    return {c["name"]: D.query(c, L) for c in D.CASES}


# (family, mode, geometry, epilogue, finisher): family 3x3s1a / 3x3s1b = tile configs 0-3 / 4-7; epilogue "raw" = a sliced launch
REQUIRED = {
    # 3x3 s1, configs 0-3: plain, x2, affine, the stats build
    ("3x3s1a", "plain", "generic", "dword", "none"), ("3x3s1a", "plain", "generic", "staged", "none"),
    ("3x3s1a", "x2", "generic", "dword", "none"), ("3x3s1a", "x2", "generic", "staged", "none"),
    ("3x3s1a", "affine", "generic", "dword", "none"), ("3x3s1a", "affine", "generic", "staged", "none"),
    ("3x3s1a", "plain_stats", "generic", "dword", "none"), ("3x3s1a", "plain_stats", "generic", "staged", "none"),
    # 3x3 s1, configs 4-7: every input stage in the FG and in the generic build; the stats build (generic only)
    ("3x3s1b", "plain", "fg", "staged", "none"), ("3x3s1b", "plain", "fg", "halved", "none"), ("3x3s1b", "plain", "fg", "dword", "none"),
    ("3x3s1b", "plain", "generic", "staged", "none"),
    ("3x3s1b", "x2", "fg", "staged", "none"), ("3x3s1b", "x2", "generic", "staged", "none"),
    ("3x3s1b", "bscale", "fg", "staged", "none"), ("3x3s1b", "bscale", "generic", "dword", "none"),
    ("3x3s1b", "x2_bscale", "fg", "halved", "none"), ("3x3s1b", "x2_bscale", "generic", "staged", "none"),
    ("3x3s1b", "affine", "fg", "staged", "none"), ("3x3s1b", "affine", "generic", "staged", "none"),
    ("3x3s1b", "plain_stats", "generic", "halved", "none"), ("3x3s1b", "plain_stats", "generic", "staged", "none"),
    ("3x3s1b", "plain_stats", "generic", "dword", "none"),
    # 3x3 s2, 7x7 s2, 4x4 s2
    ("3x3s2", "plain", "fg", "staged", "none"), ("3x3s2", "plain", "generic", "dword", "none"),
    ("3x3s2", "affine", "fg", "staged", "none"), ("3x3s2", "affine", "generic", "staged", "none"),
    ("7x7s2", "plain", "generic", "dword", "none"), ("7x7s2", "plain", "generic", "staged", "none"),
    ("4x4s2", "plain", "generic", "staged", "none"), ("4x4s2", "plain", "generic", "dword", "none"),
    # 1x1, configs 8-11
    ("1x1", "plain", "generic", "halved", "none"), ("1x1", "plain", "generic", "staged", "none"), ("1x1", "plain", "generic", "dword", "none"),
    ("1x1", "affine", "generic", "staged", "none"), ("1x1", "affine", "generic", "dword", "none"),
    ("1x1", "plain_residual", "generic", "halved", "none"), ("1x1", "plain_residual", "generic", "staged", "none"),
    ("1x1", "plain_residual", "generic", "dword", "none"),
    # the 2x2 parity kernels
    ("dgrad_s2", "plain", "generic", "dword", "none"), ("transpose4x4", "plain", "generic", "dword", "none"),
    # sliced launches: both finishers, both RES instantiations, the other kernels that end in them
    ("3x3s1a", "plain_stats", "generic", "raw", "vec"), ("3x3s1a", "plain_stats", "generic", "raw", "scalar"),
    ("3x3s1b", "plain_stats", "generic", "raw", "vec"), ("3x3s1b", "plain_stats", "generic", "raw", "scalar"),
    ("3x3s2", "plain", "generic", "raw", "vec"),
    ("1x1", "plain", "generic", "raw", "vec"), ("1x1", "plain", "generic", "raw", "scalar"),
    ("1x1", "plain_residual", "generic", "raw", "vec"), ("1x1", "plain_residual", "generic", "raw", "scalar"),
    ("wino", "-", "-", "-", "vec"), ("dgrad13", "-", "-", "-", "vec"), ("dgrad13", "-", "-", "-", "scalar"),
}


@pytest.mark.parametrize("c", D.CASES, ids=lambda c: c["name"])
def test_case_reaches_the_form_it_declares(forms, c):
    form = dict(forms[c["name"]])
    form["slices"] = form["ksplit"]
    assert c["declares"], "a case declares the form it is there for"
    got = {k: form[k] for k in c["declares"]}
    assert got == c["declares"], (c["name"], form)
    if c["family"] not in ("wino", "dgrad13"):
        assert form["config"] == c["config"] and form["mode"] == c["declares"].get("mode", D.MODES[D.mode_of(c)])
        assert form["last_split_chunks"] == form["n_chunks"] - (form["ksplit"] - 1) * form["chunks_per_split"] >= 1
        assert (form["finisher"] == 0) == (form["ksplit"] == 1) and form["grid_z"] == form["ksplit"]


def test_required_branches_are_covered(forms):
    have = {D.coverage_key(c, forms[c["name"]]) for c in D.CASES}
    assert REQUIRED <= have, sorted(REQUIRED - have)
    assert have <= REQUIRED, f"new branches reached: list them in REQUIRED so that dropping their case fails here: {sorted(have - REQUIRED)}"


def test_geometry_and_epilogue_edges_are_covered(L, forms):
    """The items of the branch list that the (family, mode, geometry, epilogue, finisher) key does not spell out."""
    ci_t = lambda c: int(importlib.import_module("speak-hack_amd").ops.conv2d_config_info(c["config"])[1])
    rows = [(c, forms[c["name"]], D.out_hw(c)) for c in D.CASES if c["family"] not in ("wino", "dgrad13")]
    tap = [r for r in rows if r[0]["family"] not in ("dgrad_s2", "transpose4x4")]

    def some(pred, of=rows):
        return [c["name"] for c, f, hw in of if pred(c, f, hw)]

    full = lambda c: set(D.FULL) <= c["opts"]
    assert {f["TW"] for _, f, _ in tap} >= {2, 4, 8, 16, 32}
    assert all(f["staged"] == 0 for _, f, _ in tap if f["TW"] < 4)
    assert some(lambda c, f, hw: f["TB"] > 1 and c["B"] % f["TB"] != 0)
    assert some(lambda c, f, hw: hw[1] % f["TW"] != 0 and hw[0] % f["TH"] != 0 and hw[1] > f["TW"] and hw[0] > f["TH"])
    assert some(lambda c, f, hw: c["Cin"] < ci_t(c), tap)
    assert some(lambda c, f, hw: f["ragged_last_chunk"] and hw[1] >= 32 and c["config"] in (4, 5, 6, 7) and c["k"] == 3 and not f["fixed_geometry"])
    assert some(lambda c, f, hw: f["fixed_geometry"] and hw[1] % 32 == 0 and hw[0] % f["TH"] == 0)
    assert some(lambda c, f, hw: f["fixed_geometry"] and hw[1] % 32 != 0 and hw[0] % f["TH"] != 0 and hw[1] > 32 and hw[0] > f["TH"] and full(c))
    assert some(lambda c, f, hw: "x2" in c["opts"] and c["Hs"] == 1 and c["Ws"] == 1) and some(lambda c, f, hw: "x2" in c["opts"] and c["Hs"] == 1 and c["Ws"] > 1)
    assert some(lambda c, f, hw: c["k"] == 7 and c["Cin"] == 3 and f["one_slot_ring"]) and some(lambda c, f, hw: c["k"] == 7 and c["Cin"] == 6 and not f["one_slot_ring"] and f["n_chunks"] == 2)
    # every epilogue form with the full flag set, with statistics from own slots and from atomics
    for staged in (0, 1, 2):
        unsliced = [r for r in tap if r[1]["ksplit"] == 1 and r[1]["staged"] == staged]
        assert some(lambda c, f, hw: full(c), unsliced), staged
        assert some(lambda c, f, hw: c["stats"] == "own", unsliced) and some(lambda c, f, hw: c["stats"] == "atomic", unsliced), staged
    # the halved form's 64-row tile: the upper 32 rows partly and wholly empty
    assert some(lambda c, f, hw: f["staged"] == 2 and c["Cout"] % 64 == 40 and c["stats"]) and some(lambda c, f, hw: f["staged"] == 2 and c["Cout"] % 64 == 24 and c["stats"])
    assert some(lambda c, f, hw: c["G"] == 2 and c["shared"] and f["ksplit"] == 1) and some(lambda c, f, hw: c["G"] == 2 and not c["shared"] and f["ksplit"] == 1)
    # dword three ways: W % 4, a misaligned tensor of each kind, the LDS-slot rule at W % 4 == 0
    dword = [r for r in tap if r[1]["ksplit"] == 1 and r[1]["staged"] == 0 and r[1]["TW"] >= 4]
    assert some(lambda c, f, hw: hw[1] % 4 != 0, dword)
    mis = set().union(*(c["misalign"] for c, f, hw in dword if hw[1] % 4 == 0))
    assert mis >= {"out", "out_pre", "noise", "residual"}, mis
    assert some(lambda c, f, hw: hw[1] % 4 == 0 and not c["misalign"], dword)
    for a, b in D.STAGED_VS_DWORD:       # one shape per staged form, staged and forced to dword by a misaligned out
        ca, cb = D.BY_NAME[a], D.BY_NAME[b]
        assert {k: v for k, v in ca.items() if k not in ("name", "misalign", "declares", "stats", "like")} == {k: v for k, v in cb.items() if k not in ("name", "misalign", "declares", "stats", "like")}
        assert forms[a]["staged"] > 0 and forms[b]["staged"] == 0 and cb["misalign"] == {"out"}
        assert cb["like"] == a and torch.equal(D.reference(ca)["y"], D.reference(cb)["y"])      # (the same operands)
    assert {forms[a]["staged"] for a, _ in D.STAGED_VS_DWORD} == {1, 2}
    # the parity kernels: both shifts, odd destinations, a bias on the transposed conv
    assert some(lambda c, f, hw: c["family"] == "dgrad_s2" and hw[0] % 2 == 1 and hw[1] % 2 == 1) and some(lambda c, f, hw: c["family"] == "transpose4x4" and "bias" in c["opts"])
    assert {c["config"] for c, f, hw in rows if c["family"] in ("dgrad_s2", "transpose4x4")} == {0, 1, 2, 3}
    # slicing and the finishers
    sliced = [r for r in rows if r[1]["ksplit"] > 1]
    assert some(lambda c, f, hw: f["last_split_chunks"] == f["chunks_per_split"] > 1, sliced)
    assert some(lambda c, f, hw: (f["n_chunks"], f["ksplit"], f["chunks_per_split"], f["last_split_chunks"]) == (5, 3, 2, 1), sliced)
    assert some(lambda c, f, hw: c["ksplit"] > f["n_chunks"] == f["ksplit"], sliced)
    scalar = [r for r in sliced if r[1]["finisher"] == 1]
    vec = [r for r in sliced if r[1]["finisher"] == 2]
    assert some(lambda c, f, hw: hw[0] * hw[1] % 4 != 0 and c["stats"], scalar)
    assert {hw[0] * hw[1] // 4 for c, f, hw in scalar if hw[0] * hw[1] % 4 == 0 and not c["misalign"] and c["stats"]} >= {36, 100}
    whole = lambda hw: hw[0] * hw[1] % 4 == 0 and (hw[0] * hw[1] // 4) in (1, 2, 4, 8, 16, 32) or hw[0] * hw[1] % 256 == 0   # a plane the vector form takes
    assert some(lambda c, f, hw: c["misalign"] and whole(hw) and c["stats"], scalar)
    assert {f["finisher_seg"] for c, f, hw in vec if c["stats"]} >= {1, 4, 16, 64}
    assert some(lambda c, f, hw: full(c) and c["stats"], scalar) and some(lambda c, f, hw: full(c) and c["stats"], vec)
    assert some(lambda c, f, hw: "residual" in c["opts"], scalar) and some(lambda c, f, hw: "residual" in c["opts"], vec)
    assert some(lambda c, f, hw: c["G"] > 1, scalar) and some(lambda c, f, hw: c["G"] > 1, vec)
    # fewer workgroups (at most 2048 x 256 threads) than elements / float4s: more than one round
    floats = lambda c, hw: c["B"] * c["G"] * c["Cout"] * hw[0] * hw[1]
    assert some(lambda c, f, hw: floats(c, hw) > 2048 * 256, scalar) and some(lambda c, f, hw: floats(c, hw) // 4 > 2048 * 256, vec)


def test_winograd_launches_cannot_reach_the_scalar_finisher(L):
    """A sliced Winograd launch ends in the vector finisher only: its planes are whole regions (a multiple of 256 pixels) and the
    launch refuses y / y_pre / noise that are not 16-byte aligned, which the query -- the same statements -- shows."""
    c = D.BY_NAME["wino.sliced"]
    assert D.query(c, L)["finisher"] == 2
    for which in ("out", "out_pre", "noise"):
        with pytest.raises(L.SpkError, match="16-byte aligned"):
            D.query(dict(c, misalign=frozenset([which])), L)


def test_query_refuses_what_is_not_a_tap_kernel_launch(L):
    c = D.case("gemm", "1x1", 1, 1, 2, 64, 128, 32, 32, 12)
    with pytest.raises(L.SpkError, match="not a tap-kernel config"):
        D.query(c, L)
    d = D.dummy_desc(D.BY_NAME["s1a.plain.tw4"], L)
    d.flags |= L.CONV_BF16X3
    with pytest.raises(L.SpkError, match="BF16X3"):
        D.query(None, L, d)
    d = D.dummy_desc(D.BY_NAME["sk.even.vec64"], L)
    d.workspace = None                                     # a sliced launch is asked about with its workspace
    with pytest.raises(L.SpkError, match="workspace"):
        D.query(None, L, d)
    assert L.lib().spk_conv2d_launch_form(None, None) < 0


@pytest.mark.parametrize("c", D.CASES, ids=lambda c: c["name"])
def test_bound_is_no_looser_than_the_older_tests(c):
    ref = D.reference(c)
    assert 0 < ref["bound"] <= D.TOL_OP, ref["bound"]
    fig = D.figures(c, ref["y32"], ref["pre"] if "y_pre" in c["opts"] else None, D.sums(ref["y32"]) if c["stats"] else None)
    for what, (v, lim) in fig.items():                     # the reference's own fp32 evaluation sits inside every limit
        assert v <= lim, (what, v, lim)


# ---- sensitivity: each fault seeded into the fp64 reference must exceed a limit by 10 x ---------------------------------------------
def _worst(c, y, pre=None, stats=None):
    fig = D.figures(c, y, pre, stats)
    return max(v / lim for v, lim in fig.values()), fig


def _mutations():
    def border_row(c):         # the last row of a partial FG tile computed with the tap one row lower (a wrong zero-padding mask)
        return D.chain(c, torch.float64, shift_tap_row=D.out_hw(c)[0] - 1)[1], None, None

    def ragged_channel(c):     # the last channel of the ragged chunk left out
        return D.chain(c, torch.float64, drop_ci=[c["Cin"] - 1])[1], None, None

    def swap(operand):
        def f(c):              # two channels of the ragged channel tile exchanged
            pre, y = D.chain(c, torch.float64, swap=(operand, c["Cout"] - 2, c["Cout"] - 1))
            return y, pre, None
        return f

    def halves(c):             # the two 32-row halves of a 64-row tile exchanged
        y = D.reference(c)["y"].clone()
        y[:, :64] = torch.cat([y[:, 32:64], y[:, :32]], 1)
        return y, None, None

    def neighbour(c):          # one pixel's value written to its x-neighbour
        y = D.reference(c)["y"].clone()
        y[-1, -1, 3, 6] = y[-1, -1, 3, 5]
        return y, None, None

    def stats_next(c):         # one channel's sums added into the next channel's
        ref = D.reference(c)
        s, q = ref["sum"].clone(), ref["sumsq"].clone()
        s[8] += s[7]
        q[8] += q[7]
        return ref["y"], None, (s, q)

    def slice_out(c):          # the last slice of the split (chunk 4 of 5: input channels 16-19) never added
        return D.chain(c, torch.float64, drop_ci=range(16, 20))[1], None, None

    return [("border row", "s1b.plain.fg.partial", border_row), ("ragged chunk", "s1b.plain.ragged", ragged_channel),
            ("bias swap", "s1b.bscale.fg", swap("bias")), ("style swap", "s1b.bscale.fg", swap("style")),
            ("demod swap", "s1b.bscale.fg", swap("demod")), ("tile halves", "s1b.x2bscale.fg", halves),
            ("x neighbour", "s1a.affine", neighbour), ("stats of the next channel", "s1b.stats.halved.c40", stats_next),
            ("missing slice", "sk.ragged.vec16", slice_out)]


@pytest.mark.parametrize("what,name,mutate", _mutations(), ids=[m[0].replace(" ", "_") for m in _mutations()])
def test_checks_see_the_seeded_fault(forms, what, name, mutate):
    c = D.BY_NAME[name]
    if what == "tile halves":
        assert c["Cout"] >= 64 and forms[name]["staged"] == 2
    if what == "missing slice":
        assert (forms[name]["n_chunks"], forms[name]["chunks_per_split"], forms[name]["ksplit"]) == (5, 2, 3) and c["Cin"] == 20
    if what in ("bias swap", "style swap", "demod swap"):
        assert c["Cout"] % 32 != 0
    y, pre, stats = mutate(c)
    worst, fig = _worst(c, y, pre, stats)
    print(f"{what} on {name}: {worst:.1f} x its limit")
    assert worst >= 10, (what, fig)
