"""The case table of tests/autograd_cases.py, checked without a GPU: every ``torch.autograd.Function`` of
``speak-hack_amd/autograd.py`` has a case; no LeakyReLU pre-activation of any case is close enough to zero for fp32 rounding to
flip its mask; the dispatch branch a case asks for is the one the host-side route functions pick; and the fp64 compositions the
GPU tests compare against pass ``torch.autograd.gradcheck``."""
import importlib
import inspect

import pytest
import torch

import autograd_cases as AC


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("speak-hack_amd")


def functions_of(module):
    return sorted(n for n, o in vars(module).items() if inspect.isclass(o) and issubclass(o, torch.autograd.Function)
                  and o.__module__ == module.__name__)


def test_every_function_has_a_case(pkg):
    A = importlib.import_module("speak-hack_amd.autograd")
    defined = functions_of(A)
    assert len(defined) >= 24, defined
    covered = {c.fn for c in AC.CASES}
    assert not set(defined) - covered, f"no case in tests/autograd_cases.py for {sorted(set(defined) - covered)}"
    assert not covered - set(defined), f"cases for Functions that do not exist: {sorted(covered - set(defined))}"
    for c in AC.CASES:
        assert set(c.also) <= set(defined), c.name


def test_twice_differentiable_set_is_the_documented_one(pkg):
    """The module docstring of autograd.py: the discriminators' Functions are differentiable twice, every other backward is
    ``once_differentiable``."""
    A = importlib.import_module("speak-hack_amd.autograd")
    for name in functions_of(A):
        once = "once_differentiable" in inspect.getsource(getattr(A, name).backward)
        assert once == (name not in AC.TWICE), name


def test_subsets_rule():
    for c in AC.CASES:
        subs, n = c.subsets(), len(c.diff)
        assert len(set(subs)) == len(subs) and c.diff in subs and all((d,) in subs for d in c.diff), c.name
        assert len(subs) == (2 ** n - 1 if n <= 4 else 2 * n + 1), c.name
        assert set(c.diff) <= set(AC.inputs(c.name)) and c.wrt in c.diff, c.name


@pytest.mark.parametrize("name", [c.name for c in AC.CASES])
def test_no_preactivation_can_flip_its_mask(name):
    case = AC.BY_NAME[name]
    t = AC.inputs(name)
    _, zs = case.ref(t)
    for z in zs:
        rms = float(z.pow(2).mean().sqrt())
        assert float(z.abs().min()) >= AC.MARGIN * rms, (name, float(z.abs().min()), rms)
    for v in t.values():                              # every input is an fp32 number: the HIP side sees the same values
        assert torch.equal(v, v.float().double())


def test_cases_with_a_lrelu_report_their_preactivations():
    with_z = {c.fn for c in AC.CASES if c.ref(AC.inputs(c.name))[1]}
    assert {"ConvBiasLReLUFn", "FusedConvFn", "ModConvFn", "FCFn", "FCDgradFn", "StyleFCGroupFn", "_LReluMaskFn"} <= with_z


@pytest.mark.parametrize("name", [c.name for c in AC.CASES if c.route is not None])
def test_requested_branch_is_the_one_taken(pkg, name):
    assert AC.BY_NAME[name].route(pkg.ops), name


def test_branch_table_reaches_both_sides(pkg):
    """The shapes of the table still split the way the case names say (a change of a routing threshold must move the cases)."""
    ops = pkg.ops
    assert ops.conv3x3_route(3, 256, 256, 32, 32)[0] == "wino" and ops.conv3x3_route(2, 12, 8, 8, 8)[0] == "direct"
    # FusedConvFn keeps the x2 image for the Winograd weight gradient, its source for the direct one
    assert ops.use_wgrad_wino(4, 256, 256, 32, 32) and not ops.use_wgrad_wino(3, 256, 256, 32, 32)
    assert ops.wgrad_mod_supported(2, 16, 24, 16, 16, False) and not ops.wgrad_mod_supported(2, 16, 12, 4, 4, False)


def _smallest_per_function():
    best = {}
    for c in AC.CASES:
        n = sum(AC.inputs(c.name)[k].numel() for k in c.diff)
        if c.fn not in best or n < best[c.fn][0]:
            best[c.fn] = (n, c.name)
    return sorted(v[1] for v in best.values())


@pytest.mark.parametrize("name", _smallest_per_function())
def test_reference_gradients_pass_gradcheck(name):
    case = AC.BY_NAME[name]
    t = AC.leaves(AC.inputs(name), case.diff, torch.float64)

    def f(*args):
        return case.ref({**t, **dict(zip(case.diff, args))})[0]

    assert torch.autograd.gradcheck(f, [t[k] for k in case.diff], eps=1e-6, atol=1e-6, rtol=1e-5, fast_mode=True)


def test_bound_rule():
    assert AC.bound(0.0) == AC.TOL_OP and AC.bound(4e-6) == AC.TOL_OP and AC.bound(1e-5) == 4e-5
