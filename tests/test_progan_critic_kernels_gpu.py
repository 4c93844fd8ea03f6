"""The ProGAN critic's own kernels (csrc/progan_critic.hip) called directly and compared element by element with a float64
CPU evaluation: the 2x2 average pool with the optional blend and its adjoint (both access paths), and the minibatch-std
channel and its adjoint (bitwise reproducible, NaN at B = 1 where torch.std gives NaN)."""
import importlib

import pytest
import torch
import torch.nn.functional as F

from oracle.weights_recipe import recipe_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd.ops")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("speak-hack_amd._lib")


DEV = "cuda:0"


def offset4(t):
    """A copy of ``t`` whose storage starts 4 bytes past a 16-byte boundary (forces the scalar path)."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def close(got, ref, rtol=2e-6, atol=1e-6):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape
    err = (got - ref).abs()
    bound = atol + rtol * ref.abs()
    assert bool((err <= bound).all()), float((err - bound).max())


# (B, C, H, W): planes B*C ragged against the 256-lane workgroups; W % 8 == 0 (16-byte path) and not (scalar path)
POOL_SHAPES = [(1, 1, 2, 2), (3, 5, 8, 8), (2, 7, 16, 24), (1, 3, 6, 10), (5, 3, 4, 4), (2, 17, 64, 64)]


@pytest.mark.parametrize("shape", POOL_SHAPES)
@pytest.mark.parametrize("blend", [False, True])
@pytest.mark.parametrize("offset", [False, True])
def test_avgpool2x_blend_fwd_bwd_vs_fp64(ops, shape, blend, offset):
    B, C, H, W = shape
    tag = f"pool.{shape}.{blend}"
    a, b = (0.7, 0.3) if blend else (1.0, 0.0)
    if not blend and shape[0] == 2:
        a = 1.75                                   # a != 1 without z as well
    x = recipe_input(tag + ".x", shape)
    z = recipe_input(tag + ".z", (B, C, H // 2, W // 2)) if blend else None
    dy = recipe_input(tag + ".dy", (B, C, H // 2, W // 2))
    xd, zd, dyd = (None if t is None else t.to(DEV) for t in (x, z, dy))
    if offset:
        xd, zd, dyd = (None if t is None else offset4(t) for t in (xd, zd, dyd))
    y = ops.avgpool2x_blend(xd, zd, a, b)
    ref = a * F.avg_pool2d(x.double(), 2, 2) + (b * z.double() if blend else 0)
    close(y, ref)
    dx, dz = ops.avgpool2x_blend_bwd(dyd, a, b, need_dz=blend)
    # the adjoint: dx = (a/4) dy on each 2x2 window, dz = b dy
    close(dx, (a / 4) * dy.double().repeat_interleave(2, -2).repeat_interleave(2, -1))
    if blend:
        close(dz, b * dy.double())
    else:
        assert dz is None


def test_avgpool2x_blend_paths_agree_bitwise(ops):
    """The 16-byte and the scalar path compute the same expression in the same order."""
    x = recipe_input("pool.paths.x", (2, 9, 16, 32)).to(DEV)
    z = recipe_input("pool.paths.z", (2, 9, 8, 16)).to(DEV)
    assert torch.equal(ops.avgpool2x_blend(x, z, 0.3, 0.7), ops.avgpool2x_blend(offset4(x), offset4(z), 0.3, 0.7))
    dx0, dz0 = ops.avgpool2x_blend_bwd(z, 0.3, 0.7, True)
    dx1, dz1 = ops.avgpool2x_blend_bwd(offset4(z), 0.3, 0.7, True)
    assert torch.equal(dx0, dx1) and torch.equal(dz0, dz1)


def test_avgpool2x_blend_refuses_odd_sizes(ops, L):
    for shape in [(1, 2, 5, 4), (1, 2, 4, 7)]:
        x = torch.zeros(shape, device=DEV)
        with pytest.raises(L.SpkError, match="even"):
            ops.avgpool2x_blend(x)
    lib = L.lib()
    y = torch.zeros(8, device=DEV)
    assert lib.spk_avgpool2x_blend_fwd(x.data_ptr(), None, y.data_ptr(), 1.0, 0.0, 2, 3, 4, None) == -1       # SPK_EINVAL
    assert lib.spk_avgpool2x_blend_bwd(y.data_ptr(), x.data_ptr(), None, 1.0, 0.0, 2, 4, 3, None) == -1


def mbstd_ref(x):
    x = x.double()
    s = torch.std(x, dim=0).mean()
    return torch.cat([x, s.expand(x.shape[0], 1, *x.shape[2:])], 1)


@pytest.mark.parametrize("B", [2, 3, 8])
@pytest.mark.parametrize("C", [1, 17, 512])
@pytest.mark.parametrize("hw", [(4, 4), (8, 4)])
def test_minibatch_std_fwd_bwd_vs_fp64(ops, B, C, hw):
    shape = (B, C) + hw
    x = recipe_input(f"mbstd.{shape}.x", shape)
    dy = recipe_input(f"mbstd.{shape}.dy", (B, C + 1) + hw)
    xd = x.to(DEV)
    y, ws = ops.minibatch_std(xd)
    close(y, mbstd_ref(x), rtol=1e-5, atol=1e-6)
    assert torch.equal(y[:, :C], xd)
    x64 = x.double().requires_grad_(True)
    (ref_dx,) = torch.autograd.grad(mbstd_ref(x64), x64, dy.double())
    dx = ops.minibatch_std_bwd(xd, dy.to(DEV), ws)
    # the std term is a sum over B*H*W values times 1/(C*H*W): bound it by that scale
    g = float(dy[:, C].double().abs().sum())
    close(dx, ref_dx, rtol=1e-5, atol=1e-6 * (1 + g / (C * hw[0] * hw[1])))
    # bitwise reproducible: fixed summation order, no atomics
    y2, ws2 = ops.minibatch_std(xd)
    used = 2 * C * hw[0] * hw[1] + 1               # mean, std per position, then s; the rest of the workspace is padding
    assert torch.equal(y, y2) and torch.equal(ws[:used], ws2[:used])
    assert torch.equal(dx, ops.minibatch_std_bwd(xd, dy.to(DEV), ws2))


def test_minibatch_std_batch_of_one_is_nan_like_torch(ops):
    x = recipe_input("mbstd.b1", (1, 17, 4, 4))
    y, _ = ops.minibatch_std(x.to(DEV))
    ref = mbstd_ref(x)
    yc = y.cpu().double()
    assert torch.equal(torch.isnan(yc), torch.isnan(ref)) and bool(torch.isnan(ref[:, 17]).all())
    assert torch.equal(yc[:, :17], ref[:, :17])
