"""The case tables of tests/small_fwd_cases.py held to the branches they are named for, without a GPU: ``spk_fc_fwd_form``,
``spk_upfirdn2d_form`` and ``spk_conv1x1_small_form`` -- the functions spk_fc_fwd, spk_upfirdn2d_fwd and the toRGB launchers
themselves dispatch by, nothing launched -- answer which form every case takes; the union must cover every branch of ``REQUIRED``;
what the launchers refuse the queries refuse; the float32 evaluation of every reference sits inside the bound its GPU test applies;
and the checks of tests/test_small_fwd_kernels_gpu.py are shown to see the faults they exist for, by seeding each into the float64
reference."""
import ctypes
import importlib
import os
import subprocess
import sys

import pytest
import torch

import small_fwd_cases as S
from test_sg2_backward_kernels_gpu import assert_rounding, rtol_for


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")._lib


SEP = [(u, d, k) for u in (1, 2) for d in (1, 2) for k in (2, 3, 4)]
REQUIRED = {
    # spk_fc_fwd: its five launch forms and what each was never run at
    "fc.scalar", "fc.vec", "fc.vec512", "fc.wide", "fc.wide4",
    "fc.scalar.I%4", "fc.scalar.x misaligned", "fc.scalar.w misaligned", "fc.scalar.x_stride%4",
    "fc.vec.one ragged trip", "fc.vec.two trips, ragged last", "fc.vec.four full trips",
    "fc.vec512.B1", "fc.vec512.B8", "fc.vec512.B11", "fc.vec512.B16", "fc.vec512.strided x", "fc.out_stride>O",
    "fc.wide.one trip, I%1024", "fc.wide.two trips", "fc.wide.two trips, ragged", "fc.wide.wide4-eligible I, O%4",
    "fc.wide.no bias", "fc.wide4.no bias",
} | {f"fc.{k}.O%4={r}" for k in ("scalar", "vec", "vec512") for r in (1, 2, 3)} \
  | {f"fc.wide4.U{U}.B{B}" for U in (2, 3, 4, 5, 6) for B in (3, 8, 11)} | {
    # spk_upfirdn2d_fwd: all 12 separable instantiations at three widths, the padding and separate() edges, the generic kernel
    "ufd.sep", "ufd.generic", "ufd.sep.NLD1", "ufd.sep.NLD2", "ufd.sep.NLD3", "ufd.sep.Ho%4", "ufd.sep<1,1,4>.Wo=128", "ufd.sep<2,2,3>.even pad0",
    "ufd.up1.pad0<0", "ufd.up1.pad0>k", "ufd.up1.pad1<0", "ufd.up2.pad0<0", "ufd.up2.pad0>k", "ufd.up2.pad1<0",
    "ufd.sep.pivot below row 0", "ufd.sep.pivot right of column 0", "ufd.sep.negative tap", "ufd.sep.non-dyadic",
    "ufd.generic.rank two", "ufd.generic.k5", "ufd.generic.k7", "ufd.generic.up3", "ufd.generic.down3", "ufd.generic.grid loop",
} | {f"ufd.sep<{u},{d},{k}>.{w}" for (u, d, k) in SEP for w in ("Wo<64", "64<Wo<128", "Wo>128") if (u, d, k, w) != (1, 1, 4, "Wo>128")} | {
    # the modulated toRGB, every row without and with a skip
    "rgb.mod.csplit.Q1", "rgb.mod.csplit.Q2", "rgb.mod.csplit.Q4", "rgb.mod.csplit.Q8", "rgb.mod.csplit.Q16, ragged last workgroup",
    "rgb.mod.csplit.C%16", "rgb.mod.vec.C<64", "rgb.mod.vec.C>=64, gate closed", "rgb.mod.scalar.HW%4", "rgb.mod.scalar.misaligned",
    "rgb.mod.no bias", "rgb.mod.O1", "rgb.mod.O2", "rgb.mod.O3", "rgb.mod.O4",
    "rgb.skip.csplit.Q2", "rgb.skip.csplit.Q4", "rgb.skip.csplit.Q8", "rgb.skip.csplit.Q16, ragged last workgroup",
    "rgb.skip.csplit.C%16", "rgb.skip.vec.C<64", "rgb.skip.vec.C>=64, gate closed", "rgb.skip.scalar.misaligned",
    "rgb.skip.no bias", "rgb.skip.O1", "rgb.skip.O2", "rgb.skip.O3", "rgb.skip.O4",
    "rgb.skip.scalar.W%4==2", "rgb.skip.every pixel on the border", "rgb.skip.csplit.W8", "rgb.skip.vec.one full grid",
    "rgb.mod.vec.grid-stride loop", "rgb.skip.vec.grid-stride loop", "rgb.mod.scalar.grid-stride loop",
    # the fromRGB expand
    "exp.C1", "exp.C2", "exp.C3", "exp.C4", "exp.O1", "exp.O5", "exp.O33", "exp.O128", "exp.n4=1", "exp.n4=64", "exp.n4=256", "exp.n4=400",
    "exp.B1", "exp.B3", "exp.scale", "exp.no scale", "exp.bias", "exp.no bias", "exp.neither scale nor bias", "exp.slope0.2", "exp.slope1.0",
    "exp.two workgroup columns, the second ragged",
}

ALL_RUNS = [(c, False) for c in S.FC_CASES + S.UFD_CASES + S.EXPAND_CASES] + S.rgb_runs()
RUN_IDS = [f"{c['kind']}.{c['name']}" + (".skip" if s else "") for c, s in ALL_RUNS]


def _named_for(c, with_skip):
    return c["skip_labels"] if with_skip else c["labels"]


@pytest.mark.parametrize("c,with_skip", ALL_RUNS, ids=RUN_IDS)
def test_case_takes_the_branches_it_is_named_for(L, c, with_skip):
    named = _named_for(c, with_skip)
    assert named, "a case names the branch it is there for"
    have = S.query(c, L, with_skip)
    assert named <= have, (sorted(named - have), sorted(have))


def test_required_branches_are_covered(L):
    named = set().union(*(_named_for(c, s) & S.query(c, L, s) for c, s in ALL_RUNS))
    reached = set().union(*(S.query(c, L, s) for c, s in ALL_RUNS))
    # the kernel, O, NLD and Ho labels follow from the forms of cases named for something else; every other label must be one that a
    # case is NAMED for and takes
    from_forms = {"fc.scalar", "fc.vec", "fc.vec512", "fc.wide", "fc.wide4", "ufd.sep", "ufd.generic", "ufd.sep.NLD1", "ufd.sep.NLD2",
                  "ufd.sep.NLD3", "ufd.sep.Ho%4"} | {f"rgb.{m}.O{o}" for m in ("mod", "skip") for o in (1, 2, 3, 4)}
    assert from_forms <= REQUIRED
    assert REQUIRED - from_forms <= named, sorted(REQUIRED - from_forms - named)
    assert from_forms <= reached, sorted(from_forms - reached)


def test_grouped_fc_table_has_both_forms():
    """spk_fc_grouped_fwd has no query: a group runs fc_dot512 when its I == 512 and the generic vector loop otherwise."""
    Is = [I for I, _ in S.FC_GROUPS]
    assert 512 in Is and {36, 260, 1024} <= set(Is) and all(I % 4 == 0 for I in Is)
    assert any(I % 256 for I in Is) and any(O % 4 for _, O in S.FC_GROUPS) and any(O > 128 for _, O in S.FC_GROUPS)
    assert S.FC_GROUPS[S.FC_GROUP_NO_BIAS][0] != 512 and set(S.FC_GROUP_BATCHES) == {3, 11}


def test_selector_shapes_take_their_forms(L):
    want = {"scalar": (0, None), "vec": (1, 5), "vec512": (2, 1), "wide": (3, 1), "wide.two trips": (3, 2), "wide4.U2": (4, 1), "wide4.U6": (4, 1)}
    for form, (B, I) in S.FC_SELECTOR_SHAPES.items():
        idx = S.fc_selector_indices(I)
        O = -(-len(idx) // 4) * 4 if form.startswith("wide4") else len(idx)
        f = S.fc_form(L, 0x100000, I, 0x800000, I, O, B)
        kernel, trips = want[form]
        assert f["kernel"] == kernel and (trips is None or f["row_trips"] == trips), (form, f)
        assert {0, 3, 4, I - 4, I - 1} <= set(idx) and (I <= 256 or {255, 256} <= set(idx)) and (I <= 6144 or {6143, 6144} <= set(idx))


def test_impulse_shapes_are_separable_and_three_waves_wide(L):
    for up, down, pad in S.IMPULSE_FORMS:
        f = S.ufd_form(L, S.ufd_filter("a4"), 1, 5, S.IMPULSE_W, up, down, pad)
        assert f["kernel"] == 1 and (f["UP"], f["DOWN"], f["K"]) == (up, down, 4) and f["grid_x"] >= 2, f
    ref = S.ufd_reference(S.impulse_input(64), S.ufd_filter("a4"), 2, 1, (2, 1))[0]
    assert int((ref != 0).sum()) == 16


# ---- what the launchers refuse, the queries refuse ------------------------------------------------------------------------------
def test_queries_refuse_what_the_launchers_refuse(L):
    lib, f = L.lib(), L.SmallForm()
    x, w = 0x100000, 0x800000
    for args, msg in (((x, 63, w, 64, 4, 2), b"row stride smaller than row"), ((x, 64, w, 64, 4, 0), b"bad shape"), ((x, 64, w, 0, 4, 2), b"bad shape"),
                      ((x, 64, w, 64, 0, 2), b"bad shape"), ((None, 64, w, 64, 4, 2), b"null"), ((x, 64, None, 64, 4, 2), b"null")):
        assert lib.spk_fc_fwd_form(*args, f) < 0 and msg in lib.spk_last_error(), args
    assert lib.spk_fc_fwd_form(x, 64, w, 64, 4, 2, None) < 0
    # the launcher answers the same for the same arguments, before anything is launched (no device is touched on these paths)
    assert lib.spk_fc_fwd(x, 63, w, None, w, 4, 2, 64, 4, 1.0, 1.0, 1.0, None) < 0 and b"row stride smaller than row" in lib.spk_last_error()
    assert lib.spk_fc_fwd(x, 64, w, None, w, 3, 2, 64, 4, 1.0, 1.0, 1.0, None) < 0 and b"row stride smaller than row" in lib.spk_last_error()

    a4 = S.ufd_filter("a4")
    arr = (ctypes.c_float * 64)(*(list(a4.flatten().tolist()) + [0.0] * 48))
    ufd = lambda *a: lib.spk_upfirdn2d_form(arr, *a, f)
    assert ufd(4, 2, 8, 8, 1, 1, 2, 1) == 0
    for args in ((8, 2, 8, 8, 1, 1, 2, 1), (0, 2, 8, 8, 1, 1, 2, 1), (4, 0, 8, 8, 1, 1, 2, 1), (4, 2, 0, 8, 1, 1, 2, 1), (4, 2, 8, 8, 0, 1, 2, 1),
                 (4, 2, 8, 8, 1, 0, 2, 1)):
        assert ufd(*args) < 0 and b"bad arguments" in lib.spk_last_error(), args
    for args in ((4, 2, 3, 8, 1, 1, 0, 0), (4, 2, 8, 8, 1, 1, -3, -2), (2, 1, 1, 1, 1, 2, 0, 0)):      # (the last: -1 / 2 is no output row)
        assert ufd(*args) < 0 and b"empty output" in lib.spk_last_error(), args
        assert lib.spk_upfirdn2d_fwd(x, w, arr, *args, 1.0, None) < 0 and b"empty output" in lib.spk_last_error(), args
    assert lib.spk_upfirdn2d_form(None, 4, 2, 8, 8, 1, 1, 2, 1, f) < 0 and lib.spk_upfirdn2d_form(arr, 4, 2, 8, 8, 1, 1, 2, 1, None) < 0

    rgb = lambda *a: lib.spk_conv1x1_small_form(*a, f)
    assert rgb(x, w, 2, 64, 3, 64, 1, 8) == 0
    for args, msg in (((x, w, 2, 64, 5, 64, 0, 0), b"O must be <= 4"), ((x, w, 0, 64, 3, 64, 0, 0), b"bad shape"), ((x, w, 2, 0, 3, 64, 0, 0), b"bad shape"),
                      ((x, w, 2, 64, 3, 0, 0, 0), b"bad shape"), ((x, w, 1, 3073, 4, 16, 0, 0), b"too large for LDS"), ((None, w, 2, 64, 3, 64, 0, 0), b"null"),
                      ((x, None, 2, 64, 3, 64, 0, 0), b"null"), ((x, w, 2, 64, 3, 63, 1, 7), b"even H x W"), ((x, w, 2, 64, 3, 24, 1, 8), b"even H x W"),
                      ((x, w, 2, 64, 3, 64, 1, 0), b"even H x W"), ((x, w, 2, 64, 3, 60, 1, 8), b"even H x W")):
        assert rgb(*args) < 0 and msg in lib.spk_last_error(), args
    assert lib.spk_conv1x1_small_form(x, w, 2, 64, 3, 64, 0, 0, None) < 0
    assert lib.spk_torgb_mod_skip_fwd(x, w, w, None, w, w, 2, 64, 3, 9, 7, 1.0, None) < 0 and b"even H x W" in lib.spk_last_error()
    assert lib.spk_conv1x1_small_fwd(x, w, None, w, 2, 64, 5, 64, 1.0, None) < 0 and b"O must be <= 4" in lib.spk_last_error()


def test_forms_read_alignment_only(L):
    """The same shape, pointers moved: the FC falls to the scalar kernel when x or w is 4 bytes off, the toRGB when x or y is."""
    fc = lambda xo, wo, stride=512: S.fc_form(L, 0x100000 + xo, stride, 0x800000 + wo, 512, 8, 4)["kernel"]
    assert (fc(0, 0), fc(4, 0), fc(0, 4), fc(16, 32), fc(0, 0, 513), fc(0, 0, 516)) == (2, 0, 0, 2, 0, 2)
    rgb = lambda xo, yo: S.rgb_form(L, 0x100000 + xo, 0x800000 + yo, 2, 32, 3, 256, False, 0)["kernel"]
    assert (rgb(0, 0), rgb(4, 0), rgb(0, 8), rgb(16, 16)) == (1, 0, 0, 1)


def test_upfirdn_form_honours_the_environment_switch(L):
    """SPK_UPFIRDN_SEP=0 sends a separable filter to the generic kernel: the query reads the launcher's own (once-per-process)
    switch, so a fresh process is asked."""
    code = ("import ctypes, sys\n"
            "class F(ctypes.Structure):\n"
            "    _fields_ = [(n, ctypes.c_int32) for n in sys.argv[2].split(',')] + [('lds_bytes', ctypes.c_int64)]\n"
            "lib = ctypes.CDLL(sys.argv[1])\n"
            "arr = (ctypes.c_float * 4)(0.25, 0.25, 0.25, 0.25)\n"
            "f = F()\n"
            "assert lib.spk_upfirdn2d_form(arr, 2, ctypes.c_int64(1), 8, 8, 1, 1, 1, 0, ctypes.byref(f)) == 0\n"
            "print(f.kernel)\n")
    names = ",".join(n for n, t in L.SmallForm._fields_ if t is ctypes.c_int32)
    for value, want in (("0", "0"), ("1", "1"), (None, "1")):
        env = {k: v for k, v in os.environ.items() if k != "SPK_UPFIRDN_SEP"}
        if value is not None:
            env["SPK_UPFIRDN_SEP"] = value
        r = subprocess.run([sys.executable, "-c", code, L.LIB_PATH, names], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr)


# ---- the bounds hold for the references' own float32 evaluation -------------------------------------------------------------------
def test_fc_float32_reference_is_inside_the_bound():
    for c in S.FC_CASES:
        t = S.fc_inputs(c["name"])
        for slope in S.SLOPES:
            ref, ref_abs = S.fc_case_reference(c["name"], slope)
            y32 = S.fc_reference(S.fc_x(c, t["xbuf"]), t["w"], t["bias"], *S.fc_muls(c["I"]), slope, dtype=torch.float32)[0]
            assert_rounding(y32, ref, ref_abs, rtol_for(c["I"] + 1), what=c["name"])


def test_upfirdn_float32_reference_is_inside_the_bound():
    for c in S.UFD_CASES:
        if c["name"] == "gen.gridloop":
            continue                                              # (the same filter and bound as gen.nonsep3; 1.3 M outputs)
        ref, ref_abs, window = S.ufd_case_reference(c["name"])
        f = S.ufd_filter(c["filt"])
        y32 = S.ufd_reference(S.ufd_input(c["name"]), f, c["up"], c["down"], c["pad"], dtype=torch.float32)[0]
        assert_rounding(y32, ref, ref_abs, rtol_for(f.numel()), atol=S.ufd_atol(c, window), what=c["name"])


def test_1x1_float32_references_are_inside_the_bound():
    for c, with_skip in S.rgb_runs():
        if c["H"] * c["W"] > 4096:
            continue
        t = S.rgb_inputs(c["name"])
        args = (t["x"], t["w"], t["mod"], t["bias"], t["skip"] if with_skip else None, c["C"] ** -0.5)
        ref, ref_abs = S.rgb_reference(*args)
        assert_rounding(S.rgb_reference(*args, dtype=torch.float32)[0], ref, ref_abs, rtol_for(c["C"] + (17 if with_skip else 1)), 2e-6, 1e-30, c["name"])
    for c in S.EXPAND_CASES:
        t = S.expand_inputs(c["name"])
        args = (t["x"], t["w"], t["bias"], t["scale"], c["slope"])
        ref, ref_abs = S.expand_reference(*args)
        assert_rounding(S.expand_reference(*args, dtype=torch.float32)[0], ref, ref_abs, rtol_for(c["C"] + 1), what=c["name"])


# ---- sensitivity: each fault seeded into the float64 reference is rejected --------------------------------------------------------
def _rejected(got, ref, ref_abs, rtol, **kw):
    with pytest.raises(AssertionError, match="outside rounding"):
        assert_rounding(got, ref, ref_abs, rtol, **kw)


def _fc_fault(name, slope, mutate_inputs=None, mutate_output=None):
    c, t = S.FC_BY_NAME[name], dict(S.fc_inputs(name))
    ref, ref_abs = S.fc_case_reference(name, slope)
    x, w, bias = S.fc_x(c, t["xbuf"]).clone(), t["w"].clone(), None if t["bias"] is None else t["bias"].clone()
    if mutate_inputs:
        x, w, bias = mutate_inputs(x, w, bias)
    bad = S.fc_reference(x, w, bias, *S.fc_muls(c["I"]), slope)[0]
    if mutate_output:
        bad = mutate_output(bad)
    assert_rounding(ref.clone(), ref, ref_abs, rtol_for(c["I"] + 1), what=name)             # (the unseeded reference passes)
    _rejected(bad, ref, ref_abs, rtol_for(c["I"] + 1))


@pytest.mark.parametrize("slope", S.SLOPES)
def test_fc_checks_see_the_seeded_faults(slope):
    def last_four_dropped(x, w, bias):
        x[:, -4:] = 0
        return x, w, bias

    def second_chunk_dropped(x, w, bias):
        x[:, 1024:2048] = 0
        return x, w, bias

    def bias_of_the_neighbour_row(x, w, bias):
        return x, w, bias[torch.arange(len(bias)) ^ 1]

    def batch_rows_swapped(y):                       # row b <-> row min(b + 8, B - 1), b = 0
        b1 = min(8, y.shape[0] - 1)
        y = y.clone()
        y[[0, b1]] = y[[b1, 0]]
        return y

    for name in ("scalar.i7", "vec.i36", "vec.i260", "vec512.b11", "wide.i2052", "wide.i8192", "wide.i6148", "wide4.u6.b11"):
        _fc_fault(name, slope, last_four_dropped)
    for name in ("wide.i2052", "wide.i8192", "wide4.u2.b3", "wide4.u6.b11"):
        _fc_fault(name, slope, second_chunk_dropped)
    for name in ("vec.i260", "vec512.b11", "wide.i8192", "wide4.u3.b11", "wide4.u2.b3"):
        _fc_fault(name, slope, None, batch_rows_swapped)
    for name in ("scalar.xoff", "vec512.b8", "wide.i2048.o6", "wide4.u4.b8"):
        _fc_fault(name, slope, bias_of_the_neighbour_row)


def test_fc_selector_sees_a_dropped_tail():
    """The exact comparison: a selector row that reads the column before its own, or a dropped last float4, changes bits."""
    B, I = S.FC_SELECTOR_SHAPES["wide.two trips"]
    x = S.recipe_input("sfw.fc.sel.cpu", (B, I))
    idx = S.fc_selector_indices(I)
    want = x[:, idx]
    x_bad = x.clone()
    x_bad[:, -4:] = 0
    assert not torch.equal(x_bad[:, idx], want) and not torch.equal(x[:, [max(i - 1, 0) for i in idx]], want)


def _ufd_fault(name, mutate):
    c = S.UFD_BY_NAME[name]
    ref, ref_abs, window = S.ufd_case_reference(name)
    f = S.ufd_filter(c["filt"])
    x, fb = mutate(S.ufd_input(name).clone(), f.clone())
    bad = S.ufd_reference(x, fb, c["up"], c["down"], c["pad"])[0]
    _rejected(bad, ref, ref_abs, rtol_for(f.numel()), atol=S.ufd_atol(c, window))


def test_upfirdn_checks_see_the_seeded_faults():
    def not_flipped(x, f):
        return x, torch.flip(f, [0, 1])

    def fx_fy_exchanged(x, f):
        return x, f.t().contiguous()

    def column_64_read_as_63(x, f):
        x[..., 64] = x[..., 63]
        return x, f

    def one_tap_dropped(c):
        def mutate(x, f):                               # (with up = down = 2 only the taps of pad0's parity ever meet a sample)
            t = f.shape[0] - 1 - (c["pad"][0] % 2 if c["up"] == c["down"] == 2 else 0)
            f[t, t] = 0
            return x, f
        return mutate

    wide = [c["name"] for c in S.UFD_CASES if c["W"] > 64 and c["name"] != "gen.gridloop"]
    assert len(wide) >= 12
    for c in S.UFD_CASES:
        if c["name"] == "gen.gridloop":
            continue
        # with up = down = 2 only the taps of pad0's parity meet a sample: <2,2,2> has one such tap per axis (a transposition cannot
        # show), <2,2,3> under StyleGAN2's pad0 = 3 the centre alone (nor can a flip: sep223.evenpad0 is in the table for that);
        # make_kernel's filters are symmetric
        k = S.ufd_filter(c["filt"]).shape[0]
        used = {i for i in range(k) if c["up"] != 2 or c["down"] != 2 or (k - 1 - i - c["pad"][0]) % 2 == 0}
        _ufd_fault(c["name"], one_tap_dropped(c))
        if {k - 1 - i for i in used} != used:
            _ufd_fault(c["name"], not_flipped)
        if len(used) > 1 and c["filt"] != "m123":
            _ufd_fault(c["name"], fx_fy_exchanged)
    for name in wide:
        _ufd_fault(name, column_64_read_as_63)
    # the exact comparison of the impulse test
    for up, down, pad in S.IMPULSE_FORMS:
        f = S.ufd_filter("a4")
        ref = S.ufd_reference(S.impulse_input(64), f, up, down, pad)[0]
        assert not torch.equal(S.ufd_reference(S.impulse_input(63), f, up, down, pad)[0], ref)
        assert not torch.equal(S.ufd_reference(S.impulse_input(64), f.t(), up, down, pad)[0], ref)
        assert not torch.equal(S.ufd_reference(S.impulse_input(64), torch.flip(f, [0, 1]), up, down, pad)[0], ref)


def test_torgb_skip_check_sees_a_shifted_skip():
    for c, with_skip in S.rgb_runs():
        if not with_skip or c["H"] * c["W"] > 4096 or c["W"] < 4:
            continue
        t = S.rgb_inputs(c["name"])
        sc = c["C"] ** -0.5
        ref, ref_abs = S.rgb_reference(t["x"], t["w"], t["mod"], t["bias"], t["skip"], sc)
        bad = S.rgb_reference(t["x"], t["w"], t["mod"], t["bias"], torch.roll(t["skip"], 1, dims=3), sc)[0]     # one low-resolution column
        _rejected(bad, ref, ref_abs, rtol_for(c["C"] + 17))
