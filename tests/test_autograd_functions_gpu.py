"""Every ``torch.autograd.Function`` of ``speak-hack_amd/autograd.py`` on its own against the fp64 composition of
tests/autograd_cases.py: forward value and first-order gradients for every requires-grad pattern of the case table, the
second-order pass ``grad(|grad((y * c).sum(), x, create_graph=True)|^2, [inputs, c])`` for the twice-differentiable Functions
(inside and outside ``input_grad_only()``, bitwise equal), ``RuntimeError`` from that pass for every ``once_differentiable``
one, and second stream against in-order launches, bitwise, for the gated / spectrally normalised weights.

Bound: rel-L2 <= ``TOL_OP`` = 2e-5 against fp64; where the same composition in fp32 on the CPU is itself worse than a quarter of
that, 4x that fp32 error (``autograd_cases.bound``).  The inputs cannot flip a LeakyReLU mask (tests/test_autograd_cases_cpu.py),
so no element is excluded.  Every comparison prints ``AGSTAT <order> <Function> <case> <what> hip=<err> fp32=<err>``.

Measured on an MI355X (worst rel-L2 per Function over its cases, next to the fp32 composition's own error on the same
gradient; "-" = not twice differentiable):

    Function                  1st hip     fp32     2nd hip     fp32
    AvgPool2xBlendBwdFn       3.9e-08  3.9e-08     4.4e-08  5.4e-08
    AvgPool2xBlendFn          4.2e-08  4.2e-08     8.4e-08  8.4e-08
    BiasNoiseStyleFn          1.0e-07  6.8e-08           -        -
    Blur2dFn                  6.3e-08  6.3e-08           -        -
    ConvBiasLReLUFn           2.7e-07  2.3e-07     2.8e-07  2.5e-07     (second order runs ConvDgradFn and _LReluMaskFn)
    ConvDgradFn               2.7e-07  2.3e-07           -        -
    FCDgradFn                 7.6e-08  7.5e-08           -        -
    FCFn                      8.0e-08  8.3e-08     1.2e-07  1.6e-07     (second order runs FCDgradFn)
    FusedConvFn               2.5e-07  2.1e-07           -        -
    FusedUpscaleFn            2.9e-07  2.4e-07           -        -
    GlobalAvgPoolFn           6.3e-08  8.8e-08     4.2e-08  7.1e-08
    InstanceNormAffineFn      1.0e-07  1.3e-07           -        -
    MinibatchStdFn            2.5e-08  2.5e-08     4.4e-07  2.1e-07
    ModConvFn                 4.0e-07  1.9e-07           -        -
    ModToRGBFn                2.5e-07  1.2e-07           -        -
    PixelNormFn               7.4e-08  3.9e-08           -        -
    SpectralNormAllFn         1.3e-07  3.6e-08           -        -
    StyleFCGroupFn            6.1e-08  8.2e-08           -        -
    ToRGBFn                   1.2e-07  1.1e-07           -        -
    UpFirDnFn                 6.6e-08  7.7e-08           -        -
    Upsample2xFn              6.1e-08  6.4e-08           -        -
    Upscale2dFn               5.5e-08  4.4e-08           -        -
    WeightGateFn              0        0                 -        -     (an identity)
    _LReluMaskFn              5.1e-09  5.1e-09     5.1e-09  5.1e-09

No comparison needed the 4x-fp32 rule: the fp32 composition is below 5e-6 everywhere, so the bound is 2e-5 throughout.
tests/test_autograd_sharing_gpu.py under the same bound: 2.7e-08 .. 2.7e-07 (fp32 composition 4.7e-08 .. 1.1e-06).
"""
import contextlib
import importlib

import pytest
import torch

import autograd_cases as AC
from conftest import rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available()
    pkg = importlib.import_module("speak-hack_amd")
    return importlib.import_module("speak-hack_amd.autograd"), pkg.ops


def hip_leaves(case, req, c_grad=False):
    return AC.leaves(AC.inputs(case.name), case.diff, torch.float32, torch.device("cuda:0"), req, c_grad)


def compare(order, case, what, got, ref64, ref32):
    """rel-L2 of ``got`` against fp64 under the bound rule; an exactly-zero (or unused) reference wants exactly zero (or None)."""
    if ref64 is None or float(ref64.abs().max()) == 0.0:
        assert got is None or float(got.abs().max()) == 0.0, (case.name, what, "expected an exactly zero gradient")
        return
    assert got is not None, (case.name, what, "gradient missing")
    assert tuple(got.shape) == tuple(ref64.shape), (case.name, what, tuple(got.shape), tuple(ref64.shape))
    assert bool(torch.isfinite(got).all()), (case.name, what)
    e, e32 = rel_l2(got, ref64), rel_l2(ref32, ref64)
    print(f"AGSTAT {order} {case.fn} {case.name} {what} hip={e:.3e} fp32={e32:.3e}")
    assert e <= AC.bound(e32), (case.name, what, e, e32, AC.bound(e32))


FIRST = [(c.name, req) for c in AC.CASES for req in c.subsets()]


@pytest.mark.parametrize("name,req", FIRST, ids=[f"{n}-{'+'.join(r)}" for n, r in FIRST])
def test_first_order(mods, name, req):
    A, ops = mods
    case = AC.BY_NAME[name]
    ref64, ref32 = AC.reference(name, torch.float64), AC.reference(name, torch.float32)
    t = hip_leaves(case, req)
    y = case.hip(A, ops, t)
    compare(1, case, "y", y.detach(), ref64["y"], ref32["y"])
    (y * t["c"]).sum().backward()
    for n in case.diff:
        if n in req:
            compare(1, case, n, t[n].grad, ref64["grads"][n], ref32["grads"][n])
        else:
            assert t[n].grad is None, (name, n)


def _second(A, ops, case, inside):
    t = hip_leaves(case, case.diff, c_grad=True)
    names = case.diff + ("c",)
    y = case.hip(A, ops, t)
    with (A.input_grad_only() if inside else contextlib.nullcontext()):
        (g,) = torch.autograd.grad((y * t["c"]).sum(), t[case.wrt], create_graph=True)
    gs = torch.autograd.grad((g * g).sum(), [t[n] for n in names], allow_unused=True)
    return g.detach(), dict(zip(names, gs))


@pytest.mark.parametrize("name", [c.name for c in AC.CASES if c.second == "twice"])
def test_second_order(mods, name):
    A, ops = mods
    case = AC.BY_NAME[name]
    ref64, ref32 = AC.reference(name, torch.float64), AC.reference(name, torch.float32)
    g, gs = _second(A, ops, case, inside=False)
    g_in, gs_in = _second(A, ops, case, inside=True)
    assert torch.equal(g, g_in), name
    for n in gs:                                  # input_grad_only() skips work autograd would discard: bitwise the same
        assert (gs[n] is None) == (gs_in[n] is None) and (gs[n] is None or torch.equal(gs[n], gs_in[n])), (name, n)
    compare(2, case, "g", g, ref64["g"], ref32["g"])
    for n in gs:
        if n.startswith("bias"):                  # a bias enters |dy/dx|^2 through the masks only
            assert gs[n] is None or float(gs[n].abs().max()) == 0.0, (name, n)
            assert ref64["grads2"][n] is None or float(ref64["grads2"][n].abs().max()) == 0.0, (name, n)
        compare(2, case, n, gs[n], ref64["grads2"][n], ref32["grads2"][n])
    live = [n for n in gs if ref64["grads2"][n] is not None and float(ref64["grads2"][n].abs().max()) > 0]
    assert "c" in live, name                      # (the pass is not vacuous: the penalty depends on c in every case)


@pytest.mark.parametrize("name", [c.name for c in AC.CASES if c.second == "raise"])
def test_once_differentiable_backward_raises_when_recorded(mods, name):
    A, ops = mods
    case = AC.BY_NAME[name]
    t = hip_leaves(case, case.diff, c_grad=True)
    y = case.hip(A, ops, t)
    (g,) = torch.autograd.grad((y * t["c"]).sum(), t[case.wrt], create_graph=True)
    assert g.requires_grad                     # (the recorded gradient hangs on the node that raises, not on nothing)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        (g * g).sum().backward()


@pytest.mark.parametrize("name", [c.name for c in AC.CASES if c.side])
def test_side_stream_gradients_match_in_order_launches(mods, monkeypatch, name):
    A, ops = mods
    case = AC.BY_NAME[name]
    dev = torch.device("cuda:0")

    def run():
        t = hip_leaves(case, case.diff)
        y = case.hip(A, ops, t)
        (y * t["c"]).sum().backward()
        out = {n: t[n].grad.clone() for n in case.diff}
        if case.second == "twice":
            _, gs = _second(A, ops, case, inside=True)
            out.update({f"2:{n}": v.clone() for n, v in gs.items() if v is not None})
        return out

    assert ops.side_stream(dev) is not None
    aside = run()
    monkeypatch.setattr(ops, "side_stream", lambda device: None)
    inline = run()
    assert set(aside) == set(inline)
    bad = [k for k in inline if not torch.equal(aside[k], inline[k])]
    assert not bad, (name, bad)
