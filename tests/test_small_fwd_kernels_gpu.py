"""Direct fp64 tests of the small forward kernels, branch by branch: the FC forward and its grouped form (csrc/fc.hip), upfirdn2d
(csrc/stylegan2_ops.hip), the modulated toRGB 1x1 with and without a skip and the fromRGB expand (csrc/pointwise.hip).  The cases
and their float64 references are tests/small_fwd_cases.py's; every case is first held, with its real device pointers, to the
branches it is named for (``spk_fc_fwd_form`` / ``spk_upfirdn2d_form`` / ``spk_conv1x1_small_form``: what the launchers dispatch by).

The criterion is rounding level ELEMENT BY ELEMENT (``assert_rounding`` of test_sg2_backward_kernels_gpu.py): |got - ref64| <=
rtol * ref_abs + atol with ``ref_abs`` the same contraction on absolute values, plus its rel-L2 cap.  LeakyReLU with a slope in
[0, 1] is 1-Lipschitz, so the pre-activation's bound holds for the activated output and no element is masked.  The selector (FC)
and impulse (upfirdn2d) tests hold bit for bit."""
import importlib

import pytest
import torch

import small_fwd_cases as S
from oracle.weights_recipe import recipe_input, recipe_tensor
from test_sg2_backward_kernels_gpu import assert_rounding, place, rtol_for

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
ids = lambda cases: [c["name"] for c in cases]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd.ops")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("speak-hack_amd._lib")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def on_device(t, dev, off=0):
    """``t`` on ``dev``, contiguous, starting ``off`` floats past a 16-byte boundary."""
    v = torch.empty(t.numel() + off, device=dev, dtype=torch.float32)[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def opt(t, dev):
    return None if t is None else t.to(dev)


def sentinel_view(dev, rows, stride, r0, c0, B, O):
    buf = torch.full((rows, stride), SENTINEL, device=dev)
    return buf, buf[r0:r0 + B, c0:c0 + O]


def assert_rest_untouched(buf, r0, c0, B, O):
    host = buf.cpu()
    inside = torch.zeros_like(host, dtype=torch.bool)
    inside[r0:r0 + B, c0:c0 + O] = True
    assert bool((host[~inside] == SENTINEL).all()), "fc wrote outside its [B, O] block"
    assert bool((host[inside] != SENTINEL).all()), "fc left part of its [B, O] block unwritten"


# ---- FC forward ------------------------------------------------------------------------------------------------------------------
def _run_fc(ops, L, dev, c, slope, out_spec):
    t = S.fc_inputs(c["name"])
    B, I, O = c["B"], c["I"], c["O"]
    x = S.fc_x(c, on_device(t["xbuf"], dev, c["x_off"]))
    w = on_device(t["w"], dev, c["w_off"])
    have = S.fc_branches(c, S.fc_form(L, x.data_ptr(), x.stride(0), w.data_ptr(), I, O, B), L)
    assert c["labels"] <= have, (sorted(c["labels"] - have), sorted(have))
    buf = out = None
    if out_spec is not None:
        buf, out = sentinel_view(dev, *out_spec, B, O)
    y = ops.fc(x, w, opt(t["bias"], dev), *S.fc_muls(I), slope, out=out)
    ref, ref_abs = S.fc_case_reference(c["name"], slope)
    assert_rounding(y, ref, ref_abs, rtol_for(I + 1), what=f"fc {c['name']} slope {slope}")
    if buf is not None:
        assert_rest_untouched(buf, out_spec[2], out_spec[3], B, O)


@pytest.mark.parametrize("slope", S.SLOPES)
@pytest.mark.parametrize("c", S.FC_CASES, ids=ids(S.FC_CASES))
def test_fc(ops, L, dev, c, slope):
    _run_fc(ops, L, dev, c, slope, c["out"])


@pytest.mark.parametrize("name", ["scalar.i7", "vec.i260", "vec512.b11", "wide.i6148", "wide4.u3.b11"])
def test_fc_writes_its_block_of_out_only(ops, L, dev, name):
    """``out=`` a view into a larger sentinel-filled buffer, on every launch form: the rows before and after [0, B) and the columns
    left and right of [0, O) stay."""
    c = S.FC_BY_NAME[name]
    _run_fc(ops, L, dev, c, 0.2, (c["B"] + 3, c["O"] + 6, 2, 5))


@pytest.mark.parametrize("form", list(S.FC_SELECTOR_SHAPES))
def test_fc_selector_rows_are_exact(ops, L, dev, form):
    """w[o] = e_{i(o)}, wmul = 1, slope 1, no bias: every other product is an exact zero, so out[:, o] is x[:, i(o)] BIT FOR BIT --
    tail elements and chunk seams that a rounding bound over thousands of terms could let through."""
    B, I = S.FC_SELECTOR_SHAPES[form]
    idx = S.fc_selector_indices(I)
    if form.startswith("wide4"):
        idx = idx + [idx[-1]] * (-len(idx) % 4)
    O = len(idx)
    x = recipe_input(f"sfw.fc.sel.{form}", (B, I))
    w = torch.zeros(O, I)
    w[torch.arange(O), torch.tensor(idx)] = 1.0
    xd, wd = x.to(dev), w.to(dev)
    f = S.fc_form(L, xd.data_ptr(), I, wd.data_ptr(), I, O, B)
    assert L.FC_KERNELS[f["kernel"]] == form.split(".")[0] and (form != "wide.two trips" or f["row_trips"] == 2), f
    y = ops.fc(xd, wd, None, 1.0, 1.0, 1.0).cpu()
    want = x[:, idx]
    assert torch.equal(y, want), f"{form}: columns {[idx[o] for o in range(O) if not torch.equal(y[:, o], want[:, o])]} differ"


@pytest.mark.parametrize("B", S.FC_GROUP_BATCHES)
def test_fc_grouped(ops, dev, B):
    """Five groups in one launch -- the generic vector loop at I = 36 (one ragged trip), 260 (two, the last ragged) and 1024 (four),
    fc_dot512 twice -- every x a column block of one wider buffer, one group without a bias: each against float64, and each
    torch.equal to ``ops.fc`` on the same operands (the header's "their results are bitwise equal", generic branch included)."""
    key = f"sfw.fcg.{B}"
    total = sum(I for I, _ in S.FC_GROUPS)
    xall = recipe_input(key + ".x", (B, total + 4))
    xall_d = xall.to(dev)
    items, refs, col = [], [], 0
    for gi, (I, O) in enumerate(S.FC_GROUPS):
        w = recipe_tensor(f"{key}.{gi}.w", (O, I), 1.0)
        bias = None if gi == S.FC_GROUP_NO_BIAS else recipe_tensor(f"{key}.{gi}.b", (O,), 1.0)
        (wmul, bmul), slope = S.fc_muls(I), S.SLOPES[gi % 2]
        xv = xall_d[:, col:col + I]
        assert xv.stride(0) == total + 4 and xv.data_ptr() % 16 == 0
        items.append((xv, w.to(dev), opt(bias, dev), wmul, bmul, slope))
        refs.append(S.fc_reference(xall[:, col:col + I], w, bias, wmul, bmul, slope))
        col += I
    outs = ops.fc_grouped(items)
    for (I, O), out, (ref, ref_abs), item in zip(S.FC_GROUPS, outs, refs, items):
        assert_rounding(out, ref, ref_abs, rtol_for(I + 1), what=f"fc_grouped [{I}x{O}] B={B}")
        assert torch.equal(out, ops.fc(*item)), f"fc_grouped [{I}x{O}] B={B}: not bitwise equal to the single launch"


def test_fc_refusals(ops, L, dev):
    buf = torch.zeros(64, device=dev)
    w = torch.zeros((4, 8), device=dev)
    narrow = torch.as_strided(buf, (2, 8), (4, 1))                     # row stride 4 < 8
    with pytest.raises(L.SpkError, match="row stride smaller than row"):
        ops.fc(narrow, w)
    with pytest.raises(L.SpkError, match="row stride smaller than row"):
        ops.fc(buf[:16].view(2, 8), w, out=torch.as_strided(buf, (2, 4), (3, 1)))
    x = torch.zeros((2, 16), device=dev)
    good = (x[:, :8], w, None, 1.0, 1.0, 1.0)
    ops.fc_grouped([good])
    with pytest.raises(L.SpkError, match="16-byte aligned multiples of 4 floats"):
        ops.fc_grouped([good, (x[:, :6], torch.zeros((4, 6), device=dev), None, 1.0, 1.0, 1.0)])        # I % 4
    with pytest.raises(L.SpkError, match="16-byte aligned multiples of 4 floats"):
        ops.fc_grouped([good, (x[:, 1:9], w, None, 1.0, 1.0, 1.0)])                                    # x 4 bytes off
    with pytest.raises(L.SpkError, match="16-byte aligned multiples of 4 floats"):
        ops.fc_grouped([(torch.zeros((2, 18), device=dev)[:, :8], w, None, 1.0, 1.0, 1.0)])            # x_stride % 4
    with pytest.raises(L.SpkError, match="bad arguments"):
        ops.fc_grouped([good] * (L.FC_MAX_GROUPS + 1))
    assert bool((buf == 0).all())


# ---- upfirdn2d -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.UFD_CASES, ids=ids(S.UFD_CASES))
def test_upfirdn2d(ops, L, dev, c):
    """Asymmetric dyadic filters with fx != fy (a flip, a transposition or a wrong factor changes the answer; the factorisation is
    exact) against oracle.modconv_ref.upfirdn2d in float64.  The non-dyadic filter alone gains an additive term: separate() accepts
    factors whose product is within 1e-6 * max|f| of every tap, so 1e-6 * max|f| * (sum of |x| under the window) -- derived from that
    threshold, not measured."""
    f = S.ufd_filter(c["filt"])
    have = S.ufd_branches(c, S.ufd_form(L, f, c["planes"][0] * c["planes"][1], c["H"], c["W"], c["up"], c["down"], c["pad"]), L)
    assert c["labels"] <= have, (sorted(c["labels"] - have), sorted(have))
    y = ops.upfirdn2d(S.ufd_input(c["name"]).to(dev), f, c["up"], c["down"], c["pad"])
    ref, ref_abs, window = S.ufd_case_reference(c["name"])
    assert_rounding(y, ref, ref_abs, rtol_for(f.numel()), atol=S.ufd_atol(c, window), what=f"upfirdn2d {c['name']}")


@pytest.mark.parametrize("up,down,pad", S.IMPULSE_FORMS, ids=[f"up{u}.down{d}" for u, d, _ in S.IMPULSE_FORMS])
def test_upfirdn2d_impulse_is_exact(ops, L, dev, up, down, pad):
    """x one-hot at row 2 and column c, c at the wave seams of a 130-wide row: every output is one product of dyadic numbers (or
    zero), so it equals the float64 reference BIT FOR BIT -- a neighbour's register, a wrong segment or a wrong tap moves it."""
    f = S.ufd_filter("a4")
    form = S.ufd_form(L, f, 1, 5, S.IMPULSE_W, up, down, pad)
    assert form["kernel"] == 1 and (form["UP"], form["DOWN"], form["K"]) == (up, down, 4)
    for col in S.IMPULSE_COLS:
        x = S.impulse_input(col)
        ref = S.ufd_reference(x, f, up, down, pad)[0]
        y = ops.upfirdn2d(x.to(dev), f, up, down, pad).cpu().double()
        assert y.shape == ref.shape and int((ref != 0).sum()) > 0
        assert torch.equal(y, ref), f"impulse at column {col}: {int((y != ref).sum())} outputs differ"


def test_upfirdn2d_refusals(ops, L, dev):
    x = torch.zeros((1, 1, 3, 8), device=dev)
    with pytest.raises(L.SpkError, match="empty output"):
        ops.upfirdn2d(x, S.ufd_filter("a4"), 1, 1, (0, 0))              # 3 rows under a 4-tap filter
    with pytest.raises(L.SpkError, match="empty output"):
        ops.upfirdn2d(torch.zeros((1, 1, 1, 1), device=dev), S.ufd_filter("a2"), 1, 2, (0, 0))
    with pytest.raises(L.SpkError, match="bad arguments"):
        ops.upfirdn2d(torch.zeros((1, 1, 9, 9), device=dev), torch.ones(8, 8), 1, 1, (0, 0))


# ---- the modulated toRGB, with and without a skip ----------------------------------------------------------------------------------
RGB_RUNS = S.rgb_runs()


@pytest.mark.parametrize("c,with_skip", RGB_RUNS, ids=[c["name"] + (".skip" if s else ".mod") for c, s in RGB_RUNS])
def test_torgb_mod(ops, L, dev, c, with_skip):
    """einsum("oc,bc,bchw->bohw") * in_scale + bias + upsample2x(skip) in float64; with a skip the bound counts its 16 taps."""
    t = S.rgb_inputs(c["name"])
    B, C, O, H, W = c["B"], c["C"], c["O"], c["H"], c["W"]
    in_scale = C ** -0.5
    x = place(t["x"], dev, c["misaligned"])
    skip = t["skip"] if with_skip else None
    y = ops.conv1x1_small_mod(x, t["w"].to(dev), t["mod"].to(dev), opt(t["bias"], dev), in_scale, opt(skip, dev))
    named = c["skip_labels"] if with_skip else c["labels"]
    have = S.rgb_branches(c, S.rgb_form(L, x.data_ptr(), y.data_ptr(), B, C, O, H * W, with_skip, W if with_skip else 0), L, with_skip)
    assert named <= have, (sorted(named - have), sorted(have))
    ref, ref_abs = S.rgb_reference(t["x"], t["w"], t["mod"], t["bias"], skip, in_scale)
    assert_rounding(y, ref, ref_abs, rtol_for(C + (17 if with_skip else 1)), what=f"toRGB {c['name']}" + (" + skip" if with_skip else ""))


def test_torgb_mod_refusals(ops, L, dev):
    z = lambda *s: torch.zeros(s, device=dev)
    with pytest.raises(L.SpkError, match="O must be <= 4"):
        ops.conv1x1_small_mod(z(1, 8, 4, 4), z(5, 8, 1, 1), z(1, 8))
    with pytest.raises(L.SpkError):
        ops.conv1x1_small_mod(z(1, 8, 4, 6), z(3, 8, 1, 1), z(1, 8), skip=z(1, 3, 2, 2))        # a skip of the wrong size


# ---- fromRGB expand ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.EXPAND_CASES, ids=ids(S.EXPAND_CASES))
def test_conv1x1_expand(ops, dev, c):
    t = S.expand_inputs(c["name"])
    y = ops.conv1x1_expand(t["x"].to(dev), t["w"].to(dev), opt(t["bias"], dev), opt(t["scale"], dev), c["slope"])
    ref, ref_abs = S.expand_reference(t["x"], t["w"], t["bias"], t["scale"], c["slope"])
    assert_rounding(y, ref, ref_abs, rtol_for(c["C"] + 1), what=f"expand {c['name']}")


def test_conv1x1_expand_refusals(ops, L, dev):
    z = lambda *s: torch.zeros(s, device=dev)
    with pytest.raises(L.SpkError, match="C <= 4 inputs"):
        ops.conv1x1_expand(z(1, 5, 4, 4), z(8, 5, 1, 1))
    with pytest.raises(L.SpkError, match="HW a multiple of 4"):
        ops.conv1x1_expand(z(1, 3, 3, 5), z(8, 3, 1, 1))
    with pytest.raises(L.SpkError, match="16-byte aligned"):
        ops.conv1x1_expand(on_device(torch.zeros(1, 3, 4, 4), dev, 1), z(8, 3, 1, 1))
