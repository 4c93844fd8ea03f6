"""The case table of tests/gemm_conv_cases.py held to the branches it is named for, without a GPU: ``spk_conv2d_gemm_form`` (the
statements of run_1x1_gemm / run_1x1_gemm2 / run_stem themselves, nothing launched) answers which form every case takes; the union
must cover every branch listed below; no bound is looser than the 2e-5 of the older conv tests; what the three launchers refuse is
refused by the query; and the checks of tests/test_gemm_conv_branches_gpu.py are shown to see the faults they exist for, by
seeding each into the fp64 reference."""
import importlib

import pytest
import torch

import direct_conv_cases as D
import gemm_conv_cases as GC


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")._lib


@pytest.fixture(scope="module")
def forms(L):
    return {c["name"]: GC.query(c, L) for c in GC.CASES}


REQUIRED = {
    # config 12, both builds: k-tiles 1, 2, 3 and an odd count >= 5 (the double-buffer loop's second half, then its first again)
    "12.plain.kt1", "12.affine.kt1", "12.plain.kt3", "12.plain.ktodd>=5", "12.plain.kt2", "12.affine.kt2", "12.affine.kt3", "12.affine.ktodd>=5",
    "12.ragged k 4", "12.ragged k 20", "12.co.one ragged", "12.co.two, second ragged", "12.co.whole", "12.hw32", "12.hw64", "12.hw96",
    "12.partial px tile", "12.tile spans images", "12.stats.own", "12.stats.atomic", "12.G2.own", "12.G2.shared", "12.transposed",
    "12.epi.bias+out_scale", "12.epi.residual+lrelu+accum", "12.epi.off",
    # configs 14 / 15, both builds: the ring before it wraps, wrapping once (4 k-tiles) and twice (7)
    "g2.14.plain", "g2.14.affine", "g2.15.plain", "g2.15.affine",
    "g2.plain.kt1", "g2.affine.kt1", "g2.plain.kt2", "g2.affine.kt2", "g2.plain.kt3", "g2.affine.kt3", "g2.plain.kt4", "g2.affine.kt4", "g2.plain.kt7", "g2.affine.kt7",
    "g2.overlap4", "g2.overlap12",
    "g2.14.cout40", "g2.14.cout72", "g2.14.cout128", "g2.14.cout136", "g2.15.cout8", "g2.15.cout64", "g2.15.cout72",
    "g2.second pass empty", "g2.second pass 8 rows", "g2.px.full", "g2.px.masked", "g2.hw4", "g2.hw40",
    "g2.grid<8", "g2.grid3", "g2.grid12", "g2.grid 9..16", "g2.grid>=17",
    "g2.half.even H", "g2.half.odd H", "g2.half.spans images", "g2.half.bias",
    "g2.residual", "g2.residual over two passes", "g2.stats.own", "g2.stats.own.partial", "g2.stats.atomic", "g2.stats.atomic.partial",
    "g2.G3 ragged second co tile", "g2.shared input", "g2.transposed", "g2.14.transposed ragged k", "g2.15.transposed ragged k",
    "g2.partial px tile", "g2.tile spans images",
    # the stem: its three builds, both ways of the sums, the four input sizes
    "stem.build.plain", "stem.build.stats", "stem.build.epi", "stem.stats.own", "stem.stats.atomic",
    "stem.epi.bias+lrelu", "stem.epi.bias", "stem.epi.lrelu",
    "stem.in.9x7", "stem.in.33x63", "stem.in.50x72", "stem.in.95x191", "stem.odd input", "stem.interior tile", "stem.mostly empty tile",
    "stem.second tile row nearly empty", "stem.partial tile in x", "stem.G2.own", "stem.G3.shared", "stem.grouped with B > 1",
}


@pytest.mark.parametrize("c", GC.CASES, ids=lambda c: c["name"])
def test_case_reaches_the_form_it_declares(forms, c):
    form = forms[c["name"]]
    assert c["declares"], "a case declares the form it is there for"
    assert {k: form[k] for k in c["declares"]} == c["declares"], (c["name"], form)
    assert form["config"] == c["config"]
    assert form["accum_half"] == ("accum_half" in c["opts"]) and form["residual"] == ("residual" in c["opts"])
    if c["config"] == 16:
        assert form["px_tiles"] == form["tiles_x"] * form["tiles_y"] * c["B"] == form["grid_x"] and form["grid_y"] == c["G"]
    else:
        H, W = D.out_hw(c)
        assert 128 * (form["px_tiles"] - 1) + form["last_px_count"] == c["B"] * H * W
        assert form["last_k_overlap"] + form["last_k_channels"] == (16 if c["config"] != 12 else form["last_k_channels"])
        assert form["grid_x"] * form["grid_y"] == form["px_tiles"] * form["co_tiles"] * c["G"]


def test_required_branches_are_covered(forms):
    have = set().union(*(GC.branches(c, forms[c["name"]]) for c in GC.CASES))
    assert REQUIRED <= have, sorted(REQUIRED - have)


def test_grid_sizes_of_the_work_item_permutation(forms):
    """Configs 14 / 15 spread a one-dimensional grid over eight XCDs: below 8 items, above 8 with a remainder, 17 or more with one."""
    grids = {forms[c["name"]]["grid_x"] for c in GC.CASES if c["config"] in (14, 15)}
    assert {3, 12} <= grids and any(n >= 17 and n % 8 for n in grids), grids


def test_lds_bytes_are_the_kernels_own(forms):
    want = {12: (2 * (128 * 33 + 32 * 132) + 256) * 4, 14: 3 * (16 * 128 + 16 * 128 + 256) * 4, 15: 3 * (16 * 64 + 16 * 128 + 256) * 4,
            16: (148 * 64 + 3 * 37 * 70 + 512) * 4}
    for c in GC.CASES:
        assert forms[c["name"]]["lds_bytes"] == want[c["config"]], c["name"]


def test_launch_form_query_still_refuses_these(L):
    for name in ("c12.k1", "g14.k1.c40", "g15.k7.c8", "stem.tiny"):
        with pytest.raises(L.SpkError, match="not a tap-kernel config"):
            form = L.Conv2dForm()
            L.check(L.lib().spk_conv2d_launch_form(GC.dummy_desc(GC.BY_NAME[name], L), form), "spk_conv2d_launch_form")


def _refused(L, c, match, off=(), **change):
    d = GC.dummy_desc(c, L, off)
    for k, v in change.items():
        setattr(d, k, v)
    with pytest.raises(L.SpkError, match=match):
        GC.query(None, L, d)


def test_query_shows_what_the_launchers_refuse(L):
    B = GC.BY_NAME
    c12, c12res, c12aff = B["c12.k1"], B["c12.k3.res"], B["c12.k3.aff"]
    g14, g14res, g15aff, half = B["g14.k1.c40"], B["g14.k2.c72.res"], B["g15.k4.c64.aff"], B["g15.half.even"]
    st, ststats = B["stem.tiny"], B["stem.odd.stats"]
    # misaligned tensors
    for c in (c12, g14, B["g15.k7.c8"]):
        for which in ("x", "w", "out"):
            _refused(L, c, "16-byte aligned x, y and weights", off=(which,))
    _refused(L, c12res, "16-byte aligned residual", off=("residual",))
    _refused(L, g14res, "16-byte aligned residual", off=("residual",))
    _refused(L, B["g15.hw4.res"], "16-byte aligned residual", off=("residual",))
    for which in ("in_scale", "in_shift"):
        _refused(L, g15aff, "16-byte aligned in_scale / in_shift", off=(which,))
        _refused(L, B["g14.k3.c128.aff"], "16-byte aligned in_scale / in_shift", off=(which,))
    for which in ("w", "out"):
        _refused(L, st, "y and w_packed must be 16-byte aligned", off=(which,))
    # shapes
    _refused(L, D.case("r", GC.GEMM, 1, 1, 2, 16, 40, 4, 4, 12), "config 12 \\(GEMM form\\) takes stride-1 1x1 convs")          # H*W % 32
    _refused(L, D.case("r", GC.GEMM, 1, 1, 2, 18, 40, 4, 8, 12), "config 12 \\(GEMM form\\) takes stride-1 1x1 convs")          # Cin % 4
    for cfg in (14, 15):
        take = "configs 14 / 15 \\(GEMM form\\) take stride-1 1x1 convs"
        _refused(L, D.case("r", GC.GEMM, 1, 1, 2, 12, 40, 4, 4, cfg), take)                                                    # Cin < 16
        _refused(L, D.case("r", GC.GEMM, 1, 1, 2, 16, 44, 4, 4, cfg), take)                                                    # Cout % 8
        _refused(L, D.case("r", GC.GEMM, 1, 1, 2, 16, 40, 3, 2, cfg), take)                                                    # H*W % 4
        _refused(L, D.case("r", GC.GEMM, 1, 1, 2, 16, 40, 2, 6, cfg, opts=("accum_half",)), "SPK_EPI_ACCUM_HALF needs")          # W % 4
    _refused(L, half, "SPK_EPI_ACCUM_HALF needs", accum_half=None)
    _refused(L, dict(half, config=12), "config 12 \\(GEMM form\\) takes bias / lrelu / accum / stats / in-affine / residual only")
    _refused(L, D.case("r", GC.STEM, 7, 2, 1, 3, 64, 9, 11, 16), "config 16 is the 7x7 stride-2 stem")                          # W % 4 (6)
    _refused(L, D.case("r", GC.STEM, 7, 2, 1, 4, 64, 9, 7, 16), "config 16 is the 7x7 stride-2 stem")                           # Cin 4
    # epilogues they do not carry
    _refused(L, dict(ststats, opts=frozenset(["bias"])), "the stem form takes")                                                # sums + bias
    _refused(L, st, "the stem form takes", out_scale=0.5)
    _refused(L, dict(st, opts=frozenset(["accum"])), "the stem form takes")
    for c, msg in ((c12, "config 12 \\(GEMM form\\) takes bias"), (g14, "configs 14 / 15 \\(GEMM form\\) take bias"),
                   (B["g15.k7.c8"], "configs 14 / 15 \\(GEMM form\\) take bias"), (st, "the stem form takes")):
        _refused(L, c, msg, flags=GC.flags_of(c, L) | L.EPI_NOISE, noise=0x200000, noise_w=0x201000)
        _refused(L, c, msg, flags=GC.flags_of(c, L) | L.EPI_STYLE, style=0x200000, style_stride=2 * c["Cout"])
        _refused(L, c, msg, y_pre=0x300000)
    # what the query itself refuses
    _refused(L, D.case("r", "1x1", 1, 1, 2, 16, 40, 4, 8, 8), "not a GEMM-form or stem config")
    _refused(L, c12, "conv2d gemm form: serves", flags=L.CONV_WINOGRAD)
    assert L.lib().spk_conv2d_gemm_form(None, None) < 0
    assert c12aff["opts"] >= {"affine"}          # (config 12 reads in_scale / in_shift element by element: no alignment rule there)
    GC.query(c12aff, L, off=("in_scale", "in_shift"))


@pytest.mark.parametrize("c", GC.CASES + GC.CROSS_FORM, ids=lambda c: c["name"])
def test_bound_is_no_looser_than_the_older_tests(c):
    ref = D.reference(c)
    assert 0 < ref["bound"] <= D.TOL_OP, ref["bound"]
    fig = D.figures(c, ref["y32"], None, D.sums(ref["y32"]) if c["stats"] else None)
    for what, (v, lim) in fig.items():                     # the reference's own fp32 evaluation sits inside every limit
        assert v <= lim, (what, v, lim)


def test_reference_extensions():
    """accum_half and the transposed operator of the fp64 chain, against their definitions written out."""
    c = GC.BY_NAME["g15.half.odd"]
    t = D.inputs(c)
    y = D.reference(c)["y"]
    base = D.chain(dict(c, opts=c["opts"] - {"accum_half"}), torch.float64)[1]
    dil = torch.zeros_like(base)
    dil[:, :, ::2, ::2] = t["half"].double()
    assert torch.equal(y, base + dil) and float(dil[:, :, 1::2].abs().max()) == 0 and float(dil[:, :, :, 1::2].abs().max()) == 0
    c = GC.BY_NAME["g14.tf"]
    t = D.inputs(c)
    assert tuple(t["w"][0].shape) == (c["Cin"], c["Cout"], 1, 1)          # the forward conv's weight: [its Cout][its Cin]
    xg = torch.zeros(c["B"], c["Cout"], c["Hs"], c["Ws"], dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(xg, t["w"][0].double()).backward(t["x"].double())
    assert D.rel_l2(D.reference(c)["y"], xg.grad) < 1e-14


# ---- sensitivity: each fault seeded into the fp64 reference must exceed a limit by 10 x ---------------------------------------------
def _tile_pixels(c, tile):
    """(image, pixel) index tensors of the flattened positions [128 tile, 128 tile + 128) inside the tensor."""
    H, W = D.out_hw(c)
    p = torch.arange(128 * tile, min(128 * (tile + 1), c["B"] * H * W))
    return p // (H * W), p % (H * W)


def _mutations():
    f64 = torch.float64

    def overlap_twice(c):      # the moved-back last k-tile counts the channels the previous tile already has
        kt = -(-c["Cin"] // 16)
        return D.chain(c, f64, double_ci=range(c["Cin"] - 16, 16 * (kt - 1)))[1], None

    def last_tile_dropped(c):
        kt = -(-c["Cin"] // 16)
        return D.chain(c, f64, drop_ci=range(16 * (kt - 1), c["Cin"]))[1], None

    def image0(c):             # every lane of a pixel tile that spans images reads the tile's first image
        t = dict(D.inputs(c))
        x = t["x"].clone()
        b, pix = _tile_pixels(c, 0)
        xv = x.view(x.shape[0], x.shape[1], -1).permute(0, 2, 1)          # [image][pixel][channel], a view
        xv[b, pix] = xv[int(b[0]), pix]
        t["x"] = x
        return D.chain(c, f64, t=t)[1], None

    def half_at_odd_rows(c):
        y = D.reference(c)["y"].clone()
        h = D.inputs(c)["half"].double()
        y[:, :, 1::2, ::2] += h[:, :, :y.shape[2] // 2]
        return y, None

    def residual_late(c):
        return D.chain(c, f64, residual_late=True)[1], None

    def second_pass(c):        # rows 64 .. 127 of the co tile keep what the destination held
        y = D.reference(c)["y"].clone()
        y[:, 64:128] = 0
        return y, None

    def tile_missing_from_sums(c):
        ref = D.reference(c)
        y = ref["y"].clone()
        b, pix = _tile_pixels(c, 1)
        y.view(y.shape[0], y.shape[1], -1).permute(0, 2, 1)[b, pix] = 0
        return ref["y"], D.sums(y)

    def parity_swap(c):        # the stem's patch one column off: even and odd columns exchanged
        t = dict(D.inputs(c))
        t["x"] = torch.roll(t["x"], 1, dims=3)
        return D.chain(c, f64, t=t)[1], None

    def edge(which):
        def f(c):              # the patch rows / columns past the image hold the last row / column instead of zeros
            return D.chain(c, f64, edge_pad=which)[1], None
        return f

    return [("overlap counted twice", "g14.k3.c128.aff", overlap_twice), ("overlap counted twice (4)", "g15.k2.c72.res", overlap_twice),
            ("last k-tile dropped", "g14.k2.c72.res", last_tile_dropped), ("last k-tile dropped (7)", "g14.k7.aff", last_tile_dropped),
            ("image 0 throughout", "g14.k1.c40", image0), ("image 0 throughout (12)", "c12.k1", image0),
            ("half at odd rows", "g14.half.odd.bias", half_at_odd_rows), ("residual after the activation", "g14.k2.c72.res", residual_late),
            ("second pass not written", "g14.k3.c128.aff", second_pass), ("tile missing from the sums", "g14.k7.aff", tile_missing_from_sums),
            ("tile missing from the sums (12)", "c12.k2.aff", tile_missing_from_sums), ("stem parity swap", "stem.partx", parity_swap),
            ("stem last patch row", "stem.odd.stats", edge("row")), ("stem last patch column", "stem.odd.stats", edge("col"))]


@pytest.mark.parametrize("what,name,mutate", _mutations(), ids=[m[0].replace(" ", "_") for m in _mutations()])
def test_checks_see_the_seeded_fault(forms, what, name, mutate):
    c, form = GC.BY_NAME[name], forms[name]
    if what.startswith("overlap"):
        assert form["last_k_overlap"] > 0
    if what.startswith("image 0"):
        assert form["tile_spans_images"]
    if what == "second pass not written":
        assert form["passes"] == 2 and form["last_pass_rows"] > 0
    if what.startswith("tile missing"):
        assert form["px_tiles"] >= 2
    y, stats = mutate(c)
    if c["stats"] and stats is None:
        stats = D.sums(y)
    fig = D.figures(c, y, None, stats)
    worst = max(v / lim for v, lim in fig.values())
    print(f"{what} on {name}: {worst:.1f} x its limit")
    assert worst >= 10, (what, fig)
