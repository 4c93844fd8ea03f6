"""csrc/conv1x1_gemm.hip (tile config 12), csrc/conv1x1_gemm2.hip (configs 14, 15) and csrc/conv7x7_stem.hip (config 16) branch by
branch, against the fp64 evaluation of the whole operator (tests/gemm_conv_cases.py on the machinery of tests/direct_conv_cases.py):
every case runs at its forced config, ``spk_conv2d_gemm_form`` is asked again of the very descriptor that is launched (real
pointers) and must answer the declared form, y lands in a NaN-filled destination between guard floats that must stay untouched,
y and the BatchNorm sums are held to the reference, a second identical launch must reproduce y bit for bit, and with one copy of
the sums per pixel tile every copy beyond the launch's pixel tiles must stay zero.

The bound is measured on the reference, never on the kernel: per case max(4 x the error of the same chain in fp32 on the CPU,
sqrt(kh kw Cin) 2^-24); a single element: |y - ref| <= 8 x bound x rms(ref); the sums: rel-L2 over channels < 1e-6 and per channel
within 8 x bound x rms(ref) x B H W (x 2 max|ref| for the squares).  Which build, k-tile count, ragged tile, pass, pixel tile and
grid each case reaches is asserted without a GPU in tests/test_gemm_conv_forms_cpu.py, which also seeds the faults these checks
exist for into the reference (each lands >= 10 x over a limit).

The packers of configs 12, 14, 15 and 16 are compared bit for bit with a NumPy restatement of the documented layouts.

Measured on an MI355X (rel-L2 against the fp64 operator, and the bounds of the same cases; max |diff| as a share of its limit):
    config 12 (10 cases)        4.0e-8 .. 1.8e-7   (1.6e-7 .. 8.9e-7)    max |diff| / limit <= 0.31
    config 14 (9 cases)         6.1e-8 .. 1.1e-7   (2.7e-7 .. 6.0e-7)    <= 0.46
    config 15 (10 cases)        5.0e-8 .. 1.5e-7   (2.4e-7 .. 6.3e-7)    <= 0.43
    stem, config 16 (8 cases)   1.6e-7 .. 2.2e-7   (7.2e-7 .. 8.6e-7)    <= 0.46
    BatchNorm sums, rel-L2 over channels (limit 1e-6): configs 12 / 14 / 15 1.9e-8 .. 5.0e-8, per channel <= 0.06 of the limit (sum),
        <= 0.03 (squares); the stem 1.8e-7 .. 2.0e-7, per channel <= 0.01
    configs 12, 14, 15 and the tap kernel (config 8) on one shape (3 x 52 -> 72 @ 8 x 8): rel-L2 1.1e-7 (4.3e-7) each, and bit for
        bit equal to one another (distance 0 against a limit of 3.5e-6)
    the packers: bit for bit the documented layouts, tf 0 and 1, one weight and a list of three.
The kernels sit a factor 2 to 6 inside the bound everywhere; no case found a fault."""
import importlib

import numpy as np
import pytest
import torch

import direct_conv_cases as D
import gemm_conv_cases as GC
from oracle.weights_recipe import recipe_tensor
from test_direct_conv_branches_gpu import Launch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class GemmLaunch(Launch):
    """A case of tests/gemm_conv_cases.py on the device: the form comes from ``spk_conv2d_gemm_form``; with own slots the sums get
    two copies more than the launch has pixel tiles."""
    extra_slots = 2

    def query(self):
        return self.ops.desc_gemm_form(self.desc)


def _hold(c, y, stats):
    fig = D.figures(c, y, None, stats)
    for what, (v, lim) in fig.items():            # the figures first, then the assertions
        print(f"{c['name']}: {what} {v:.2e} (limit {lim:.2e}, {v / lim:.3f} of it)")
    for what, (v, lim) in fig.items():
        assert v <= lim, (c["name"], what, v, lim)


@pytest.mark.parametrize("c", GC.CASES, ids=lambda c: c["name"])
def test_branch(pkg, dev, c):
    run = GemmLaunch(pkg, dev, c)
    assert {k: run.form[k] for k in c["declares"]} == c["declares"], run.form      # the launched descriptor takes the declared form
    y, _, stats = run.run()
    _hold(c, y, stats)
    if c["stats"] == "own":
        used = run.stats.abs().sum((1, 2)).cpu() != 0
        tiles = run.form["px_tiles"]
        assert run.form["stats_own"] == 1 and run.stats.shape[0] == tiles + 2
        assert not bool(used[tiles:].any()), "a copy of the sums beyond the launch's pixel tiles was written"
        assert int(used[:tiles].sum()) >= 2, "the sums did not go to the pixel tiles' own copies"
    y2, _, _ = run.run()
    assert torch.equal(y, y2), "a second identical launch differs"


@pytest.mark.parametrize("cfg,Cout,Cin,tf", GC.PACK_SHAPES)
def test_packed_gemm_weights_are_the_documented_layout(pkg, dev, cfg, Cout, Cin, tf):
    ops = pkg.ops
    ws = [recipe_tensor(f"gcc.pack.{Cout}.{Cin}.w{i}", (Cout, Cin, 1, 1), Cin ** -0.5) for i in range(3)]
    want = [GC.pack_expected(w.numpy(), cfg, tf) for w in ws]
    one = ops.pack_conv_weight(ws[0].to(dev), cfg, tf)
    many = ops.pack_conv_weights_list([w.to(dev) for w in ws], cfg, tf)
    torch.cuda.synchronize()
    assert one.numel() == want[0].size and np.array_equal(one.cpu().numpy(), want[0])
    assert many.numel() == 3 * want[0].size and np.array_equal(many.cpu().numpy(), np.concatenate(want))
    opCin = Cout if tf else Cin
    if cfg != 12 and opCin % 16:                   # the zeros the moved-back k-tile relies on are there
        n_kt = -(-opCin // 16)
        img = one.cpu().view(-1, n_kt, 16, 128 if cfg == 14 else 64)
        assert float(img[:, -1, :16 * n_kt - opCin].abs().max()) == 0.0 and float(img[:, -1, 16 * n_kt - opCin:].abs().max()) > 0.0


def test_packed_stem_weights_are_the_documented_layout(pkg, dev):
    ops = pkg.ops
    ws = [recipe_tensor(f"gcc.pack.stem.w{i}", (64, 3, 7, 7), 147 ** -0.5) for i in range(3)]
    want = [GC.pack_expected(w.numpy(), 16, 0) for w in ws]
    one = ops.pack_conv_weight(ws[0].to(dev), 16)
    many = ops.pack_conv_weights_list([w.to(dev) for w in ws], 16)
    torch.cuda.synchronize()
    assert np.array_equal(one.cpu().numpy(), want[0]) and float(one[147 * 64:].abs().max()) == 0.0
    assert np.array_equal(many.cpu().numpy(), np.concatenate(want))


def test_gemm_forms_and_the_tap_kernel_on_one_shape(pkg, dev):
    """One shape through configs 12, 14, 15 and the tap kernel (config 8): each is held to the reference; the distances between
    them are put on record and stay within twice the single-element limit of that one reference."""
    ys = {}
    for c in GC.CROSS_FORM:
        run = (GemmLaunch if c["config"] >= 12 else Launch)(pkg, dev, c)
        assert run.form["config"] == c["config"]
        ys[c["config"]] = run.run()[0]
        _hold(c, ys[c["config"]], None)
    ref = D.reference(GC.CROSS_FORM[0])
    assert all(torch.equal(ref["y"], D.reference(c)["y"]) for c in GC.CROSS_FORM)          # (the same operands)
    limit = 2 * D.MAX_FACTOR * ref["bound"] * D.rms(ref["y"])
    dist = {(a, b): float((ys[a] - ys[b]).abs().max()) for a in ys for b in ys if a < b}
    for (a, b), d in dist.items():
        print(f"config {a} against config {b}: max |difference| {d:.2e} (limit {limit:.2e}, {d / limit:.3f} of it)")
    assert max(dist.values()) <= limit, dist
