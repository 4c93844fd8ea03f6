"""The case table of tests/wino_cases.py held to what it is named for, without a GPU: ``spk_conv2d_wino_form`` (the planner of the
Winograd launch, nothing launched) answers which of the 22 instantiations of ``wino_kernel`` every case takes, its split and how many
items its persistent workgroups walk on 256 and on 64 compute units; the union must be exactly the 22 kernels and the listed walked
forms; the schedule model proves that the walks cross image and slice boundaries; no bound is looser than the older tests' 5e-6 and
the fp32 emulation sits inside every element limit; and the query refuses what the launch refuses."""
import importlib

import pytest
import torch

import wino_cases as W

N_CU = 256


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")._lib


@pytest.fixture(scope="module")
def forms(L):
    """Every case at the batch that meets its walk target on 256 CUs."""
    return {c["name"]: W.query(c, L, N_CU, W.batch_for(c, N_CU, L)) for c in W.CASES}


WALKS = [c for c in W.CASES if c["walk"] > 1]


@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c["name"])
def test_case_reaches_the_form_it_declares(L, forms, c):
    B = W.batch_for(c, N_CU, L)
    assert {"mod", "rgb", "up", "shape", "epi"} <= set(c["declares"]), "a case declares the kernel it is there for"
    for n_cu in (N_CU, 64):                  # (the kernel, the split and the finisher do not depend on the device; the grid does)
        form = W.query(c, L, n_cu, B)
        assert {k: form[k] for k in c["declares"]} == c["declares"], (n_cu, form)
        assert form["groups"] == c["G"] and form["co_tiles"] == c["G"] * -(-c["Cout"] // 64) and form["n_chunks"] == c["Cin"] // 8
        assert form["chunks_per_slice"] * form["ksplit"] == form["n_chunks"] and form["chunks_per_slice"] % 2 == 0
        assert form["items"] == B * W.regions_per_image(c, form) * form["ksplit"]
        assert form["grid_x"] % 8 == 0 and 8 <= form["grid_x"] <= max(8, n_cu // form["co_tiles"]) and form["grid_x"] < form["items"] + 8
        assert (form["finisher"] == 0) == (form["ksplit"] == 1) and form["lds_bytes"] == 155648
        # the schedule model and the library agree on the walks, and the model deals every item exactly once
        walks = W.schedule(form)
        assert sorted(it for w in walks for it in w) == [(r, z) for r in range(form["items"] // form["ksplit"]) for z in range(form["ksplit"])]
        assert (min(map(len, walks)), max(map(len, walks))) == (form["walk_min"], form["walk_max"])
    form = forms[c["name"]]
    assert W.meets_walk(c, form), form
    assert B == 2 or not W.meets_walk(c, W.query(c, L, N_CU, B - 1)), "batch_for: the smallest batch"
    if c["walk"] == 1:
        assert W.meets_walk(c, W.query(c, L, 64, B))


def test_the_22_kernels_and_the_walked_forms_are_covered(forms):
    one = {W.kernel_key(forms[c["name"]]) for c in W.CASES if c["walk"] == 1 and forms[c["name"]]["ksplit"] == 1}
    assert one == W.KERNELS, (sorted(W.KERNELS - one), sorted(one - W.KERNELS))
    walked = {W.kernel_key(f) + (int(f["ksplit"] > 1), int(f["groups"] > 1)) for f in (forms[c["name"]] for c in WALKS)}
    assert walked == W.WALKED, (sorted(W.WALKED - walked), sorted(walked - W.WALKED))
    # every instantiation with the full flag set its form allows
    for key in W.KERNELS:
        mod, rgb, up, shape, epi = key
        full = set(W.MOD_SET if mod else W.RGB_SET if rgb else W.FULL if epi == W.GENERIC else W.LEAN_SET)
        assert [c["name"] for c in W.CASES if c["walk"] == 1 and W.kernel_key(forms[c["name"]]) == key and full <= c["opts"]], key
    # the GENERIC rows, one case for each cause alone
    gen = [c for c in W.CASES if c["walk"] == 1 and W.kernel_key(forms[c["name"]]) == (0, 0, 0, W.WIDE, W.GENERIC)]
    lean_like = lambda c: not ({"y_pre", "accum"} & c["opts"]) and 0 < c["slope"] <= 1
    assert {c["Cout"] for c in gen if lean_like(c) and c["Cout"] % 64} >= {40, 200}
    whole = [c for c in gen if c["Cout"] % 64 == 0]
    assert [c for c in whole if "y_pre" in c["opts"] and "accum" not in c["opts"] and 0 < c["slope"] <= 1]
    assert [c for c in whole if "accum" in c["opts"] and "y_pre" not in c["opts"] and 0 < c["slope"] <= 1]
    assert [c for c in whole if not ({"y_pre", "accum"} & c["opts"]) and c["slope"] > 1 and "lrelu" in c["opts"]]
    assert [c for c in whole if not ({"y_pre", "accum"} & c["opts"]) and c["slope"] <= 0 and "lrelu" in c["opts"]]
    # x 4 bytes off: a plain and an x2 case
    assert {forms[c["name"]]["up"] for c in W.CASES if c["misalign_x"]} == {0, 1}
    for a, b in W.NOSTORE_VS_LEAN:           # the same launch but for y
        ca, cb = W.BY_NAME[a], W.BY_NAME[b]
        assert {k: v for k, v in ca.items() if k not in ("name", "like", "declares", "opts")} == {k: v for k, v in cb.items() if k not in ("name", "like", "declares", "opts")}
        assert ca["opts"] == cb["opts"] | {"nostore"} and forms[a]["epi"] == W.LEAN_NOSTORE and forms[b]["epi"] == W.LEAN
    assert {W.BY_NAME[a]["walk"] for a, _ in W.NOSTORE_VS_LEAN} == {1, 3}


def test_walks_of_one_two_and_three_chunk_pairs(forms):
    for mod, up in ((0, 0), (0, 1), (1, 0)):
        pairs = {f["chunks_per_slice"] // 2 for f in (forms[c["name"]] for c in WALKS)
                 if (f["mod"], f["rgb"], f["up"], f["shape"], f["ksplit"], f["groups"]) == (mod, 0, up, W.WIDE, 1, 1)}
        assert pairs >= {1, 2, 3}, (mod, up, pairs)


def test_walks_cross_image_and_slice_boundaries(forms):
    """Proved on the schedule model: every walk case has a workgroup whose consecutive items lie in different images (so every
    per-image operand -- style, noise, in_scale, demod -- changes mid-stream); a plain case also has consecutive items of ONE image;
    among the sliced cases one changes the slice from item to item and one keeps it."""
    same_image, slice_changes, slice_stays = [], [], []
    for c in WALKS:
        form = forms[c["name"]]
        assert form["walk_max"] >= 3 and form["walk_min"] < form["walk_max"]
        steps = W.walk_pairs(c, form)
        assert any(a[0] != b[0] for a, b in steps), c["name"]
        if any(a[0] == b[0] for a, b in steps) and W.kernel_key(form)[:3] == (0, 0, 0) and form["ksplit"] == 1 and form["groups"] == 1:
            same_image.append(c["name"])
        if form["ksplit"] > 1:
            (slice_changes if all(a[1] != b[1] for a, b in steps) else slice_stays if all(a[1] == b[1] for a, b in steps) else []).append(c["name"])
            assert ((form["grid_x"] >> 3) % form["ksplit"] != 0) == all(a[1] != b[1] for a, b in steps)
    assert same_image and slice_changes and slice_stays, (same_image, slice_changes, slice_stays)


def test_no_case_is_larger_than_the_cap(L, forms):
    for c in W.CASES:
        B, (Hs, Ws), Cy = W.batch_for(c, N_CU, L), W.in_hw(c), c["G"] * c["Cout"]
        assert B * (c["G"] * c["Cin"] * Hs * Ws * 4 + Cy * c["H"] * c["W"] * (4 + 8)) <= W.SIZE_CAP, c["name"]


def test_a_larger_batch_keeps_the_first_images(L):
    """The bound is measured on two images; the GPU test runs the walk cases at the batch of the device."""
    c = W.BY_NAME["walk.mod.wide.c16"]
    small, large = W.inputs(c, 2), W.inputs(c, 5)
    for name, v in small.items():
        if name != "w" and v.shape[0] == 2 and large[name].shape[0] == 5:
            assert torch.equal(v, large[name][:2]), name
    assert all(torch.equal(a, b) for a, b in zip(small["w"], large["w"])) and torch.equal(small["bias"], large["bias"])
    assert not torch.equal(large["style"][0], large["style"][1]) and not torch.equal(large["bscale"][3], large["bscale"][4])


@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c["name"])
def test_bound_is_no_looser_than_the_older_tests(c):
    b = W.bounds(c)
    assert 0 < b["bound"] <= W.TOL, b["per"]
    fig = W.figures(c, b["emu"], b["ref"])
    for what, (v, lim) in fig.items():                     # the emulation sits inside every limit, element limits included
        assert v <= lim, (what, v, lim)


def test_winograd_emulation_is_the_convolution():
    x, w = torch.randn(2, 8, 8, 12, dtype=torch.float64), torch.randn(5, 8, 3, 3, dtype=torch.float64)
    got = W.wino_conv32(x.float(), w.float())
    assert W.rel_l2(got, torch.nn.functional.conv2d(x.float().double(), w.float().double(), padding=1)) < 1e-6
    s = torch.rand(2, 8) + 0.5
    got = W.wino_conv32(x.float(), w.float(), s)
    assert W.rel_l2(got, torch.nn.functional.conv2d(x.float().double() * s.double().view(2, 8, 1, 1), w.float().double(), padding=1)) < 1e-6


# ---- sensitivity: the faults the walk cases exist for, seeded into the fp64 reference, exceed a limit ------------------------------
def test_checks_see_an_operand_of_the_wrong_image(forms):
    c = W.BY_NAME["walk.mod.wide.c16"]
    t = dict(W.inputs(c, 2))
    ref = dict(zip(("pre", "y", "rgb"), W.chain64(c, t)))
    for name in ("demod", "bscale", "style", "noise"):     # image 1 computed with image 0's operand
        v = t[name].clone()
        v[1] = v[0]
        got = dict(zip(("pre", "y", "rgb"), W.chain64(c, dict(t, **{name: v}))))
        worst = max(v / lim for v, lim in W.figures(c, got, ref).values())
        print(f"{name} of the wrong image: {worst:.0f} x its limit")
        assert worst >= 10, name


# ---- the query refuses what the launch refuses -----------------------------------------------------------------------------------
def _refused(L, c, match, B=2, **patch):
    d = W.dummy_desc(c, L, B)
    for k, v in patch.items():
        setattr(d, k, v)
    with pytest.raises(L.SpkError, match=match):
        W.query(None, L, N_CU, desc=d)


def test_query_refuses_what_the_launch_refuses(L):
    rgb, plain, x2 = W.BY_NAME["rgb.wide.lean"], W.BY_NAME["plain.wide.lean"], W.BY_NAME["x2.wide.lean"]
    base = W.dummy_desc(rgb, L, 2)
    # toRGB with a sliced contraction, y_pre, accumulate or modulation
    _refused(L, dict(rgb, Cin=64, want=2), "SPK_EPI_TORGB with a sliced contraction")
    _refused(L, rgb, "SPK_EPI_TORGB needs", y_pre=0x7000000)
    _refused(L, rgb, "SPK_EPI_TORGB needs", flags=base.flags | L.EPI_ACCUM)
    _refused(L, rgb, "SPK_EPI_TORGB needs", flags=base.flags | L.CONV_IN_BATCH_SCALE, in_scale=0x7000000)
    _refused(L, dict(rgb, Cout=65), "SPK_EPI_TORGB needs")
    # x2 with groups or a batch scale
    _refused(L, x2, "SPK_CONV_UPSAMPLE2X is the bilinear x2 of a plain launch", flags=W.flags_of(x2, L) | L.CONV_IN_BATCH_SCALE, in_scale=0x7000000)
    _refused(L, dict(x2, opts=frozenset(["x2"]), G=2), "SPK_CONV_UPSAMPLE2X is the bilinear x2 of a plain launch")
    # a grouped launch with epilogue flags
    _refused(L, dict(plain, opts=frozenset(["bias"]), G=3), "a grouped launch takes SPK_EPI_ACCUM only")
    W.query(dict(plain, opts=frozenset(["accum"]), G=3), L, N_CU, 2)
    # H x W that no region shape tiles; Cin % 16
    _refused(L, dict(plain, H=12), "not a whole number of 32 x 8 or 16 x 16 regions")
    _refused(L, dict(plain, H=16, W=24), "not a whole number of 32 x 8 or 16 x 16 regions")
    _refused(L, dict(plain, Cin=24), "not a whole number of 32 x 8 or 16 x 16 regions")
    # the 2 GB limit: of x, for an x2 launch of the LOW-resolution tensor
    big = dict(plain, H=512, W=512, Cin=16, Cout=8)
    assert W.query(big, L, N_CU, 127)["items"] == 127 * 64 * 16
    _refused(L, big, "exceeds 2 GB", B=128)
    bigx2 = dict(x2, H=1024, W=1024, Cin=16, Cout=8)
    assert W.query(bigx2, L, N_CU, 127)["items"] == 127 * 128 * 32
    _refused(L, bigx2, "SPK_CONV_UPSAMPLE2X needs an output of twice the input size", B=128)
    # alignment, the workspace of a sliced launch, other descriptors
    _refused(L, plain, "16-byte aligned", y=0x7000004)
    _refused(L, plain, "16-byte aligned", x=0x7000002)
    _refused(L, W.BY_NAME["sliced.ks2"], "workspace", workspace=None)
    _refused(L, plain, "SPK_CONV_WINOGRAD descriptors only", flags=0)
    assert L.lib().spk_conv2d_wino_form(None, N_CU, None) < 0 and L.lib().spk_conv2d_wino_form(W.dummy_desc(plain, L, 2), 0, L.WinoForm()) < 0
