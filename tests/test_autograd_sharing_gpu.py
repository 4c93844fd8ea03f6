"""How several graph nodes share one gradient tensor in ``speak-hack_amd/autograd.py`` (``_first_or_add``, ``_wgrad_shared``,
``SpectralNormAllFn``'s ``_spk_sn_dw``, ``_wgrad_aside`` on the second stream), against fp64 sums instead of against another
HIP schedule: one layer in three forwards before one backward and a second backward without ``zero_grad``; the whole
discriminator step (four forwards and two R1 passes in one backward, then the generator step's backward piled on top); one
gated Parameter weight used by two ``FusedConvFn`` nodes; a loss and a gradient penalty on the SAME forward, where a weight has
two users in one backward pass (the conv's own backward and ``ConvDgradFn``)."""
import copy
import importlib

import pytest
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils import spectral_norm

import autograd_cases as AC
from conftest import grad_close, rel_l2
from test_discriminator_gpu import make, r1, ref_forward

pytestmark = pytest.mark.gpu

LAYER_SEED = 0           # a seed for which no pre-activation of the six forwards below is within MARGIN * rms of zero (asserted)


@pytest.fixture(scope="module")
def A():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd.autograd")


def layer_inputs(seed=LAYER_SEED):
    """(conv, [(x, c)] * 6): a spectral-norm wrapped 3x3 conv with a bias, train mode, and six (input, loss weight) pairs."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)                                   # (spectral_norm draws its initial u, v from the global generator)
    conv = spectral_norm(nn.Conv2d(12, 8, 3, padding=1))
    with torch.no_grad():
        conv.weight_orig.copy_(AC.q4(g, 8, 12, 3, 3))
        conv.bias.copy_(AC.odd32(g, 8))
    pairs = [(AC.q4(g, 2, 12, 8, 8).float(), AC.rnd(g, 2, 8, 8, 8).float()) for _ in range(6)]
    return conv.train(), pairs


def layer_reference(dtype, seed=LAYER_SEED):
    """torch's own hook on a copy of the layer: [(weight_orig.grad, bias.grad, [d loss / d W_hat per forward]) after pass 1 and after
    pass 2 (no zero_grad between)], and every pre-activation."""
    conv, pairs = layer_inputs(seed)
    conv = conv.to(dtype)
    out, zs = [], []
    for part in (pairs[:3], pairs[3:]):
        loss, hats = 0.0, []
        for x, c in part:
            z = conv(x.to(dtype))                       # the pre-forward hook: one power iteration, then W / sigma
            conv.weight.retain_grad()
            hats.append(conv.weight)
            zs.append(z.detach())
            loss = loss + (F.leaky_relu(z, 0.2) * c.to(dtype)).sum()
        loss.backward()
        out.append((conv.weight_orig.grad.clone(), conv.bias.grad.clone(), [h.grad.clone() for h in hats]))
    return out, zs


def close(what, got, ref64, ref32):
    e, e32 = rel_l2(got, ref64), rel_l2(ref32, ref64)
    print(f"AGSTAT share {what} hip={e:.3e} fp32={e32:.3e}")
    assert e <= AC.bound(e32), (what, e, e32)


def test_one_layer_three_forwards_then_a_second_backward(A):
    dev = torch.device("cuda:0")
    ref64, zs = layer_reference(torch.float64)
    ref32, _ = layer_reference(torch.float32)
    for z in zs:
        assert float(z.abs().min()) >= AC.MARGIN * float(z.pow(2).mean().sqrt())
    conv, pairs = layer_inputs()
    conv.to(dev)
    seen = {"weight_orig": [], "bias": []}
    for n in seen:
        getattr(conv, n).register_post_accumulate_grad_hook(lambda p, n=n: seen[n].append(p.grad.clone()))
    for k, part in enumerate((pairs[:3], pairs[3:])):
        loss, hats = 0.0, []
        for x, c in part:
            (h,) = A.spectral_norm_all([conv], True)             # u / v move with every forward
            h.retain_grad()
            hats.append(h)
            loss = loss + (A.conv_bias_lrelu(x.to(dev), h, conv.bias, 3, 1, 0.2) * c.to(dev)).sum()
        loss.backward()                                          # (the second one: a fresh graph, no zero_grad)
        for n in seen:                                           # one hook call per backward, on the complete gradient of the pass
            assert len(seen[n]) == k + 1, (n, len(seen[n]))
            assert torch.equal(seen[n][k], getattr(conv, n).grad), n
        close(f"pass{k + 1} weight_orig", conv.weight_orig.grad, ref64[k][0], ref32[k][0])
        close(f"pass{k + 1} bias", conv.bias.grad, ref64[k][1], ref32[k][1])
        for j, h in enumerate(hats):
            close(f"pass{k + 1} weight{j}", h.grad, ref64[k][2][j], ref32[k][2][j])


def _bce(pred, label):
    return F.binary_cross_entropy_with_logits(pred, torch.full_like(pred, label))


def d_step_loss(forward, mod, xs, r1_of):
    """training.discriminator_loss without the generator: two real and two fake inputs, then the R1 penalty on both reals."""
    real = (_bce(forward(mod, xs[0]), 0.9) + _bce(forward(mod, xs[1]), 0.9)) / 2
    fake = (_bce(forward(mod, xs[2]), 0.1) + _bce(forward(mod, xs[3]), 0.1)) / 2
    return real + fake + 10.0 * (r1_of(mod, xs[0]) + r1_of(mod, xs[1])) / 2


def g_step_loss(forward, mod, xs):
    """training.generator_loss's adversarial term: the data gradient flows through D and piles up on D's parameters."""
    return (_bce(forward(mod, xs[4]), 0.9) + _bce(forward(mod, xs[5]), 0.9)) / 2


def test_discriminator_step_then_generator_step_without_zero_grad():
    disc = importlib.import_module("speak-hack_amd.discriminator")
    T = importlib.import_module("speak-hack_amd.training")
    dev = torch.device("cuda:0")
    B, res = 2, 32
    d32 = make(disc, res, 21, True)
    d64, dg = copy.deepcopy(d32).double(), copy.deepcopy(d32).to(dev)
    g = torch.Generator().manual_seed(22)
    xs = [torch.rand(B, 3, res, res, generator=g) * 2 - 1 for _ in range(6)]
    hip_forward = lambda m, t: m(t)
    out = {}
    for name, mod, cast, fwd, r1_of in (("ref32", d32, lambda t: t.clone(), ref_forward, lambda m, t: r1(ref_forward, m, t.clone())),
                                        ("ref64", d64, lambda t: t.double(), ref_forward, lambda m, t: r1(ref_forward, m, t.clone())),
                                        ("hip", dg, lambda t: t.to(dev), hip_forward, T.compute_r1_reg)):
        xin = [cast(x) for x in xs]
        fakes = [x.requires_grad_(True) for x in xin[4:]]
        d_step_loss(fwd, mod, xin, r1_of).backward()
        after_d = {n: p.grad.detach().cpu().double().clone() for n, p in mod.named_parameters()}
        g_step_loss(fwd, mod, xin).backward()                    # no zero_grad: D step + G step
        after_g = {n: p.grad.detach().cpu().double().clone() for n, p in mod.named_parameters()}
        out[name] = (after_d, after_g, [x.grad.detach().cpu().double() for x in fakes])
    for k, what in ((0, "D step"), (1, "D step + G step")):
        got, r32, r64 = (out[n][k] for n in ("hip", "ref32", "ref64"))
        assert set(got) == set(r64) and any(n.endswith("weight_orig") for n in got)
        for n in r64:
            ok, info = grad_close(got[n], r32[n], r64[n], pixels=B * res * res)
            assert ok, (what, n, info)
    for j in range(2):                                           # ... and the data gradient the generator receives
        ok, info = grad_close(out["hip"][2][j], out["ref32"][2][j], out["ref64"][2][j], pixels=B * res * res)
        assert ok, ("fake input", j, info)


def test_gated_weight_shared_by_two_convs(A):
    """One gated Parameter weight feeding two ``FusedConvFn`` nodes of one forward (the decoder's ``forward_pair``): the
    parameter's gradient is the sum of both."""
    ops = importlib.import_module("speak-hack_amd").ops
    dev = torch.device("cuda:0")
    assert ops.side_stream(dev) is not None
    g = torch.Generator().manual_seed(3)
    t = {"weight": AC.q4(g, 8, 12, 3, 3), "bias": AC.odd32(g, 8), "x0": AC.q4(g, 2, 12, 8, 8), "x1": AC.q4(g, 2, 12, 8, 8),
         "c0": AC.rnd(g, 2, 8, 8, 8).float().double(), "c1": AC.rnd(g, 2, 8, 8, 8).float().double()}

    def reference(dtype):
        w, b = (t[k].to(dtype).requires_grad_(True) for k in ("weight", "bias"))
        loss = sum((F.leaky_relu(F.conv2d(t[f"x{i}"].to(dtype), w, b, padding=1), 0.2) * t[f"c{i}"].to(dtype)).sum() for i in range(2))
        return torch.autograd.grad(loss, [w, b])

    ref64, ref32 = reference(torch.float64), reference(torch.float32)
    w, b = (nn.Parameter(t[k].float().to(dev)) for k in ("weight", "bias"))
    (gw,) = A.gate_weights([w])
    pk = ops.PackedConvWeight()
    loss = sum((A.fused_conv(t[f"x{i}"].float().to(dev), gw, b, None, None, None, False, 0.2, pk) * t[f"c{i}"].float().to(dev)).sum()
               for i in range(2))
    loss.backward()
    close("gated weight", w.grad, ref64[0], ref32[0])
    close("gated bias", b.grad, ref64[1], ref32[1])


@pytest.mark.parametrize("name", [c.name for c in AC.CASES if c.fn == "ConvBiasLReLUFn"])
def test_loss_and_penalty_on_one_forward(A, name):
    """``(y * c).sum() + |d (y * c).sum() / dx|^2`` in ONE backward: the weight is used by the conv's own backward and by
    ``ConvDgradFn``.  For a spectrally normalised weight the second user accumulates inside the kernel (``_wgrad_shared``) and
    hands autograd nothing; for a Parameter the engine adds.  Either way the gradient is the fp64 sum of both."""
    ops = importlib.import_module("speak-hack_amd").ops
    case = AC.BY_NAME[name]

    def grads(run, dtype, device=None):
        t = AC.leaves(AC.inputs(name), case.diff, dtype, device)
        y = run(t)
        loss = (y * t["c"]).sum()
        (g,) = torch.autograd.grad(loss, t["x"], create_graph=True)
        (loss + (g * g).sum()).backward()
        return {n: t[n].grad for n in case.diff}

    ref64, ref32 = (grads(lambda t: case.ref(t)[0], dt) for dt in (torch.float64, torch.float32))
    got = grads(lambda t: case.hip(A, ops, t), torch.float32, torch.device("cuda:0"))
    for n in case.diff:
        assert got[n] is not None, (name, n)
        close(f"{name} loss+penalty {n}", got[n], ref64[n], ref32[n])
