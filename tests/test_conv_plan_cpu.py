"""The forward conv planners seen through the two form queries, without a GPU: over the case tables of tests/direct_conv_cases.py and
tests/gemm_conv_cases.py and a short stretch of the seeded sweep of tools/dump_conv_decisions.py -- a descriptor is served by one
form query at most, a refusal leaves nothing behind, the workspace queries cover what a sliced launch checks, and
spk_conv2d_stats_slots is the launch's grid_x."""
import importlib
import os
import random
import sys

import pytest

import direct_conv_cases as D
import gemm_conv_cases as G

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import dump_conv_decisions as T  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")._lib


@pytest.fixture(scope="module")
def descs(L):
    """(name, make): make() builds the descriptor afresh, so that a test may change it."""
    out = [(c["name"], (lambda c=c: D.dummy_desc(c, L))) for c in D.CASES]
    out += [(c["name"], (lambda c=c: G.dummy_desc(c, L))) for c in list(G.CASES) + list(G.CROSS_FORM)]
    rnd = random.Random(7)
    drawn = [T.drawn(L, rnd, i)[1] for i in range(1200)]

    def copy(d):
        e = L.Conv2dDesc()
        for n, _ in L.Conv2dDesc._fields_:
            setattr(e, n, getattr(d, n))
        return e
    return out + [(f"drawn{i}", (lambda d=d: copy(d))) for i, d in enumerate(drawn)]


def fields(s):
    return tuple(getattr(s, n) for n, _ in s._fields_)


def ask(L, d):
    cf, gf = L.Conv2dForm(), L.GemmForm()
    rc_c = L.lib().spk_conv2d_launch_form(d, cf)
    err_c = L.lib().spk_last_error() if rc_c else b""
    rc_g = L.lib().spk_conv2d_gemm_form(d, gf)
    err_g = L.lib().spk_last_error() if rc_g else b""
    return rc_c, cf, rc_g, gf, (rc_c, err_c, fields(cf), rc_g, err_g, fields(gf))


def test_one_form_query_serves_a_descriptor(L, descs):
    served = {0: 0, 1: 0}
    for name, make in descs:
        d = make()
        rc_c, _, rc_g, _, _ = ask(L, d)
        assert not (rc_c == 0 and rc_g == 0), name
        if d.flags & L.CONV_BF16X3:
            assert rc_c != 0 and rc_g != 0, name
        if not name.startswith("drawn"):
            assert (rc_c == 0) != (rc_g == 0), name              # every table case is served
        served[rc_c == 0 or rc_g == 0] += 1
    assert served[1] > len(descs) // 2 and served[0] > len(descs) // 20, served      # neither mostly refused nor all served


def test_a_refused_query_leaves_the_next_answer_unchanged(L, descs):
    refused = D.dummy_desc(D.BY_NAME["sk.even.vec64"], L)
    refused.workspace = None                                        # refused by the planner, after routing and geometry
    assert L.lib().spk_conv2d_launch_form(refused, L.Conv2dForm()) != 0 and L.lib().spk_conv2d_gemm_form(refused, L.GemmForm()) != 0
    for name, make in descs[::3]:
        first = ask(L, make())[4]
        assert L.lib().spk_conv2d_launch_form(refused, L.Conv2dForm()) != 0 and L.lib().spk_conv2d_gemm_form(refused, L.GemmForm()) != 0
        assert ask(L, make())[4] == first, name


def test_workspace_queries_cover_the_sliced_launches(L, descs):
    lib = L.lib()
    seen = {"tap": 0, "wino": 0, "dgrad13": 0}
    for name, make in descs:
        d = make()
        rc, cf, _, _, _ = ask(L, d)
        if rc != 0 or cf.ksplit <= 1:
            continue
        groups = max(d.groups, 1)
        need = cf.ksplit * d.B * groups * d.Cout * d.H * d.W * 4
        if d.flags & L.CONV_WINOGRAD:
            family, ws = "wino", lib.spk_conv2d_wino_workspace_bytes(d.ksplit, d.B, d.Cin, groups * d.Cout, d.H, d.W)
        elif cf.config == 13:
            family, ws = "dgrad13", lib.spk_conv2d_dgrad_s2_workspace_bytes(d.B, d.Cin, d.Cout, d.Hin, d.Win, d.H, d.W, groups)
            if lib.spk_conv2d_dgrad_s2_config(d.B, d.Cin, d.Cout, d.Hin, d.Win) != 13:
                ws = need           # config 13 asked for by hand where the library would not pick it: that query speaks for its own pick
        else:
            family, ws = "tap", lib.spk_conv2d_workspace_bytes_grouped(d.config, d.ksplit, d.kh, d.kw, d.stride, d.B, d.Cin, d.Cout, d.H, d.W, groups)
        assert ws >= need, (name, family, ws, need)
        seen[family] += 1
        d.workspace_bytes = need - 1                                # one byte short
        rc, short, _, _, _ = ask(L, d)
        if family == "dgrad13":
            assert rc == 0 and short.ksplit == 1 and short.finisher == 0, name      # runs unsliced
        else:
            assert rc != 0, name
            assert lib.spk_conv2d_launch_form(d, L.Conv2dForm()) != 0 and b"workspace" in lib.spk_last_error(), name
    assert min(seen.values()) >= 3, seen


def test_stats_slots_is_the_grid_x_of_the_launch(L, descs):
    lib = L.lib()
    n = 0
    for name, make in descs:
        d = make()
        if d.flags & (L.CONV_WINOGRAD | L.CONV_DGRAD_S2 | L.CONV_TRANSPOSE4X4_S2 | L.CONV_BF16X3):
            continue                                                # the query speaks of the direct convs
        rc_c, cf, rc_g, gf, _ = ask(L, d)
        slots = lib.spk_conv2d_stats_slots(d.config, d.kh, d.kw, d.stride, d.B, d.Cin, d.Cout, d.H, d.W)
        if rc_c == 0:
            assert slots == cf.grid_x, (name, slots, cf.grid_x)
            n += 1
        if rc_g == 0:           # configs 14 / 15 run a one-dimensional grid: the pixel tiles are its px_tiles
            assert slots == (gf.px_tiles if gf.config in (14, 15) else gf.grid_x), (name, slots)
            n += 1
    assert n > 500
