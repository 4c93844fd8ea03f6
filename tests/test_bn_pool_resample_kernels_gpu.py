"""Direct fp64 tests of the memory-bound kernels around the MFMA ones, at the smallest shapes that reach every branch of their
SHIPPED host dispatch: the BatchNorm / pool pieces of csrc/bn_pool.hip (``bn_add_relu``, ``maxpool3x3s2``, ``global_avgpool``,
``dilate2x``, ``bn_replay_running``, ``bn_backward``), the x2 resampling kernels of csrc/pointwise.hip (``upsample2x``,
``upsample2x_bilinear``) and their adjoint in csrc/decoder_bwd.hip (``upsample2x_bilinear_bwd``).

Those dispatches branch on ``HW % 4``, ``Win % 4``, ``Hin % 2``, 16-byte pointer alignment (``place(..., misaligned=True)`` puts a
tensor 4 bytes past a 16-byte boundary), the plane count and capped grids; DESIGN.md section 2 lists which case reaches which
branch.  Every reference is evaluated here, in float64 on the CPU, with plain torch.

Not reached: the lab forms behind SPK_UPSAMPLE_FORM / SPK_UPSAMPLE_BWD_FORM (read once per process, not shipped routes), and the
65536-workgroup cap of ``upsample2x_bilinear_bwd``, whose second grid-stride trip needs more than 134M elements -- too large for a
test of a few seconds.

Rule (a), used where a kernel sums a long plane in fp32 (or runs a large shape): the bound is max(the project's fixed bound,
4 x the error of torch's own fp32 CPU evaluation of the same op against the same fp64 reference); the factor 4 covers a different
summation order.  The fp32 errors measured for the shapes used are written next to each use; none comes from a kernel's output."""
import functools
import importlib
import itertools

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from oracle.weights_recipe import recipe_input, recipe_tensor

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24                     # unit roundoff of float32
EPS = 1e-5


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def offset_copy(t, dev):
    """``t`` on ``dev`` as a contiguous view 4 bytes past a 16-byte boundary."""
    v = torch.empty(t.numel() + 1, device=dev, dtype=torch.float32)[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def place(t, dev, misaligned=False):
    if misaligned:
        return offset_copy(t, dev)
    t = t.to(dev)
    assert t.data_ptr() % 16 == 0
    return t


def v4(t):
    return t.view(1, -1, 1, 1)


# ---- 1. upsample2x forward (csrc/pointwise.hip) -------------------------------------------------------------------------------
def bilinear64(x):
    return F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False)


def zero_border64(x):
    """upfirdn2d(up = 2, [1,3,3,1] (x) [1,3,3,1] * 4 / 64, pad (2,1)) in float64: the construction of tests/test_wino_gpu.py."""
    B, C, H, W = x.shape
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64)
    k = (k1[:, None] * k1[None, :]) / 64.0 * 4.0
    up = torch.zeros(B, C, 2 * H, 2 * W, dtype=torch.float64)
    up[:, :, ::2, ::2] = x.double()
    return F.conv2d(F.pad(up, (2, 1, 2, 1)), k.flip(0, 1).view(1, 1, 4, 4).repeat(C, 1, 1, 1), groups=C)


def assert_upsampled(y, ref, what):
    assert y.shape == ref.shape, what
    err = float((y.double().cpu() - ref).abs().max())
    assert err <= 2e-6 * max(1.0, float(ref.abs().max())), (what, err)


@pytest.mark.parametrize("zero_border", [False, True])
@pytest.mark.parametrize("shape", [
    (2, 3, 2, 4), (1, 2, 6, 12),                              # Hin even: upsample2x_vec2x2_kernel (first / last row pair; 3 pairs)
    (2, 3, 3, 8), (1, 2, 5, 4), (2, 5, 7, 12), (1, 3, 1, 4),  # Hin odd: upsample2x_vec2_kernel (interior rows; one-row plane)
])
def test_upsample2x_vector_forms_both_borders(pkg, dev, shape, zero_border):
    x = recipe_input(f"bpr.up.{shape}", shape)
    xd = place(x, dev)
    y = pkg.ops.upsample2x(xd, zero_border=zero_border)
    assert_upsampled(y, zero_border64(x) if zero_border else bilinear64(x), (shape, zero_border))
    if not zero_border:              # one kernel behind both entry points: the same bits
        assert torch.equal(pkg.ops.upsample2x_bilinear(xd), y)


@pytest.mark.parametrize("shape,misaligned", [
    ((2, 3, 6, 10), False), ((1, 1, 5, 1), False), ((1, 2, 1, 1), False),      # Win % 4 != 0
    ((2, 3, 4, 8), True),                                                      # Win % 4 == 0, input 4 bytes off
    ((1, 65536, 1, 4), False),                                                 # Win % 4 == 0, planes >= 65536 (grid.y limit)
])
def test_upsample2x_scalar_kernel(pkg, dev, shape, misaligned):
    """``upsample2x_kernel`` by width, by misalignment and by plane count, through both entry points."""
    x = recipe_input(f"bpr.ups.{shape}", shape)
    xd = place(x, dev, misaligned)
    ref = bilinear64(x)
    assert_upsampled(pkg.ops.upsample2x_bilinear(xd), ref, (shape, "bilinear"))
    assert_upsampled(pkg.ops.upsample2x(xd, zero_border=False), ref, (shape, "upsample2x"))


def test_upsample2x_zero_border_refusals(pkg, dev):
    """The zero-border form exists only as the 16-byte kernels: everything else is refused, never served by another tap rule."""
    E = pkg._lib.SpkError
    with pytest.raises(E):                                           # Win % 4 != 0
        pkg.ops.upsample2x(place(recipe_input("bpr.upr.w", (2, 3, 6, 10)), dev), zero_border=True)
    with pytest.raises(E):                                           # input not 16-byte aligned
        pkg.ops.upsample2x(place(recipe_input("bpr.upr.m", (2, 3, 4, 8)), dev, True), zero_border=True)
    with pytest.raises(E):                                           # 65536 planes
        pkg.ops.upsample2x(place(recipe_input("bpr.upr.p", (1, 65536, 1, 4)), dev), zero_border=True)


# ---- 2. upsample2x backward (csrc/decoder_bwd.hip) ----------------------------------------------------------------------------
def up_adjoint64(g, in_shape):
    x = torch.zeros(in_shape, dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad(bilinear64(x), x, g.double())
    return gx


@pytest.mark.parametrize("shape,misaligned", [
    ((2, 3, 4, 8), False),                                             # Win % 4 == 0, Hin even: upsample2x_bwd_vec2_kernel
    ((2, 3, 5, 8), False), ((1, 2, 3, 4), False), ((1, 2, 7, 12), False),   # Win % 4 == 0, Hin odd: upsample2x_bwd_vec_kernel
    ((2, 2, 5, 6), False),                                             # Win % 4 != 0: upsample2x_bwd_kernel
    ((2, 3, 4, 8), True),                                              # gradient 4 bytes off: upsample2x_bwd_kernel
])
def test_upsample2x_bwd_every_form(pkg, dev, shape, misaligned):
    B, C, H, W = shape
    x = recipe_input(f"bpr.upb.x.{shape}", shape)
    g = recipe_input(f"bpr.upb.g.{shape}", (B, C, 2 * H, 2 * W))
    ref = up_adjoint64(g, shape)
    dx = pkg.ops.upsample2x_bilinear_bwd(place(g, dev, misaligned))
    assert dx.shape == ref.shape
    assert rel_l2(dx, ref) < 2e-5, rel_l2(dx, ref)
    # every element at rounding level: an output is a sum of <= 16 products with exact weights, <= 10 roundings deep, so
    # |dx - ref| <= 16 u * up^T(|g|) (the same contraction on absolute values, immune to cancellation).  One wrong border tap fails.
    err = (dx.double().cpu() - ref).abs()
    assert bool((err <= 16 * U32 * up_adjoint64(g.abs(), shape)).all()), float(err.max())
    # adjoint identity with the GPU forward: <up(x), g> = <x, up^T(g)>.  The forward's elements carry <= 4 roundings, the
    # adjoint's <= 10, so the two inner products (summed in float64) differ by <= (4 + 10) u * <up(|x|), |g|>; 16 u allowed.
    y = pkg.ops.upsample2x_bilinear(place(x, dev, misaligned))
    lhs = float((y.double().cpu() * g.double()).sum())
    rhs = float((x.double() * dx.double().cpu()).sum())
    scale = float((bilinear64(x.abs()) * g.double().abs()).sum())
    assert abs(lhs - rhs) <= 16 * U32 * scale, (lhs, rhs, scale)


# ---- 3. bn_add_relu ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,misaligned,large", [
    ((2, 19, 11, 14), None, False),     # HW % 4 != 0: bn_add_relu_kernel<false>
    ((2, 7, 8, 20), None, False),       # HW % 4 == 0, aligned: bn_add_relu_kernel<true>; C = 7 coprime to 4 and to B
    ((2, 7, 8, 20), "b", False),        # HW % 4 == 0, b 4 bytes off: the dword form
    ((2, 7, 8, 20), "a", False),        # HW % 4 == 0, a 4 bytes off: the dword form
    ((1, 2, 129, 130), None, True),     # dword form, HW = 16770 > 64 * 256: grid.y capped, a second trip
    ((1, 2, 260, 256), None, True),     # 16-byte form, HW / 4 = 16640 > 64 * 256: grid.y capped, a second trip
])
def test_bn_add_relu_every_form_and_branch(pkg, dev, shape, misaligned, large):
    C = shape[1]
    key = f"bpr.bar.{shape}"
    a, b = recipe_input(key + ".a", shape), recipe_input(key + ".b", shape)
    sa, ba, sb, bb = (recipe_tensor(f"{key}.{n}", (C,), 0.5) for n in ("sa", "ba", "sb", "bb"))
    ad, bd = place(a, dev, misaligned == "a"), place(b, dev, misaligned == "b")
    sad, bad, sbd, bbd = (t.to(dev) for t in (sa, ba, sb, bb))

    def forms(dt):
        A, Bt, SA, BA, SB, BB = (t.to(dt) for t in (a, b, sa, ba, sb, bb))
        return {"full": F.relu(A * v4(SA) + v4(BA) + Bt * v4(SB) + v4(BB)),
                "affine_a_plus_b": F.relu(A * v4(SA) + v4(BA) + Bt),
                "affine_a_only": F.relu(A * v4(SA) + v4(BA)),
                "plain_sum_no_relu": A + Bt}

    got = {"full": pkg.ops.bn_add_relu(ad, sad, bad, bd, sbd, bbd),
           "affine_a_plus_b": pkg.ops.bn_add_relu(ad, sad, bad, bd),
           "affine_a_only": pkg.ops.bn_add_relu(ad, sad, bad),
           "plain_sum_no_relu": pkg.ops.bn_add_relu(ad, None, None, bd, relu=False)}
    ref64, ref32 = forms(torch.float64), forms(torch.float32)
    for name, ref in ref64.items():
        # rule (a) for the two large shapes: torch's fp32 evaluation measures 2.7e-8 .. 6.0e-8 over the four forms at both shapes
        # (an elementwise op: no long sum), so the project's 1e-6 is the bound everywhere
        bound = max(1e-6, 4 * rel_l2(ref32[name], ref)) if large else 1e-6
        e = rel_l2(got[name], ref)
        assert got[name].shape == ref.shape and e < bound, (name, e, bound)


# ---- 4. maxpool3x3s2 forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [
    (1, 2, 2, 2),            # one output per plane: eight of the nine taps are padding
    (2, 3, 7, 9),            # odd sizes, several planes
    (1, 5, 1024, 1026),      # 5 * 512 * 513 = 1,313,280 outputs > 4096 workgroups * 256: a second grid-stride trip
])
def test_maxpool3x3s2_negative_windows_and_grid_stride(pkg, dev, shape):
    C = shape[1]
    x = recipe_input(f"bpr.mp.{shape}", shape)
    neg = (x - 5.0).clamp(max=-0.125)                # every value negative: the padding has to be -inf, a 0 would win every border window
    assert bool((neg < 0).all())
    ref = F.max_pool2d(neg.double(), 3, 2, 1)
    got = pkg.ops.maxpool3x3s2(neg.to(dev))
    assert got.shape == ref.shape and rel_l2(got, ref) < 1e-7
    assert bool((got < 0).all())
    # folded affine + ReLU with one channel of negative scale (the maximum moves to the smallest input there)
    s, o = 1.0 + recipe_tensor("bpr.mp.s", (C,), 0.3), recipe_tensor("bpr.mp.o", (C,), 0.3)
    s[0] = -s[0].abs()
    ref = F.max_pool2d(F.relu(x.double() * v4(s.double()) + v4(o.double())), 3, 2, 1)
    got = pkg.ops.maxpool3x3s2(x.to(dev), s.to(dev), o.to(dev))
    assert got.shape == ref.shape and rel_l2(got, ref) < 1e-6


# ---- 5. global_avgpool ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (8, 8), (17, 241)])      # HW = 1, 63 (one idle lane), 64, 4097 (65 trips, ragged)
def test_global_avgpool_plane_sizes(pkg, dev, H, W):
    shape = (3, 7, H, W)                             # 21 planes: the last workgroup holds one live wave of four
    x = recipe_input(f"bpr.ap.{shape}", shape)
    ref = x.double().mean((2, 3), keepdim=True)
    got = pkg.ops.global_avgpool(x.to(dev))
    # rule (a): torch's fp32 mean against the fp64 mean measures 0 (HW = 1), 9.1e-8 (63), 7.6e-8 (64), 1.4e-7 (4097) for these
    # inputs, so the project's 1e-6 is the bound at every size
    bound = max(1e-6, 4 * rel_l2(x.mean((2, 3), keepdim=True), ref))
    assert got.shape == ref.shape and rel_l2(got, ref) < bound, (rel_l2(got, ref), bound)


# ---- 6. dilate2x ---------------------------------------------------------------------------------------------------------------
def dilated(x, Ho, Wo):
    B, C, H, W = x.shape
    y = torch.zeros(B, C, Ho, Wo, dtype=x.dtype)
    y[:, :, 0:2 * H:2, 0:2 * W:2] = x
    return y


@pytest.mark.parametrize("shape,Ho,Wo", [
    ((2, 3, 4, 5), 8, 10), ((2, 3, 4, 5), 7, 9), ((2, 3, 4, 5), 8, 9), ((2, 3, 4, 5), 7, 10),
    ((1, 5, 512, 513), 1024, 1025),                  # 5,248,000 outputs > 4096 workgroups * 256: five grid-stride trips
])
def test_dilate2x_exact(pkg, dev, shape, Ho, Wo):
    x = recipe_input(f"bpr.dil.{shape}", shape)
    xd = x.to(dev)
    # the op allocates its output uninitialised: hand the allocator a block of that size full of NaN first, so that a zero the
    # kernel does not write shows
    junk = torch.full((shape[0], shape[1], Ho, Wo), float("nan"), device=dev)
    del junk
    y = pkg.ops.dilate2x(xd, Ho, Wo)
    assert torch.equal(y.cpu(), dilated(x, Ho, Wo))


def test_dilate2x_refuses_other_sizes(pkg, dev):
    x = recipe_input("bpr.dil.r", (2, 3, 4, 5)).to(dev)
    with pytest.raises(pkg._lib.SpkError):
        pkg.ops.dilate2x(x, 9, 10)                   # Ho = 2H + 1
    with pytest.raises(pkg._lib.SpkError):
        pkg.ops.dilate2x(x, 8, 11)                   # Wo = 2W + 1


# ---- 7. bn_replay_running ------------------------------------------------------------------------------------------------------
def test_bn_replay_running_equals_batch_norm_and_bn_finalize_bitwise(pkg, dev):
    """One launch over three BatchNorms: C = 37, C = 300 (the ``c += 256`` loop iterates) and a count = 1 item (the unbiased
    variance is guarded: v * 1 / 0 otherwise).  Against float64 ``F.batch_norm(training=True)`` on a tensor with exactly the sums
    handed over, and bitwise against ``bn_finalize`` from the same sums -- the claim of the kernel's comment."""
    mom = 0.1
    items, finals, refs = [], [], []
    for i, shape in enumerate([(4, 37, 3, 5), (2, 300, 2, 3), (1, 5, 1, 1)]):
        C = shape[1]
        count = shape[0] * shape[2] * shape[3]
        y = recipe_input(f"bpr.rep.y{i}", shape) * 2.0 + 0.7
        stats = torch.cat([y.double().sum((0, 2, 3)), (y.double() ** 2).sum((0, 2, 3))]).to(dev)
        rm = recipe_tensor(f"bpr.rep.rm{i}", (C,), 0.3)
        rv = recipe_tensor(f"bpr.rep.rv{i}", (C,), 1.0).abs() + 0.5
        rm_ref, rv_ref = rm.double(), rv.double()
        if count > 1:
            F.batch_norm(y.double(), rm_ref, rv_ref, None, None, True, mom, EPS)
        else:
            # torch refuses one value per channel in training mode; the project's rule there (bn_finalize_kernel) is the biased
            # variance, which for one value is exactly 0
            rm_ref = (1 - mom) * rm_ref + mom * y.double().view(C)
            rv_ref = (1 - mom) * rv_ref
        refs.append((rm_ref, rv_ref))
        items.append((stats, count, rm.to(dev), rv.to(dev)))
        finals.append((stats, count, C, rm.to(dev), rv.to(dev)))
    pkg.ops.bn_replay_running(items, mom)
    for (stats, count, C, rm_f, rv_f), (_, _, rm_d, rv_d), (rm_ref, rv_ref) in zip(finals, items, refs):
        assert bool(torch.isfinite(rm_d).all()) and bool(torch.isfinite(rv_d).all()), count
        assert rel_l2(rm_d, rm_ref) < 1e-6 and rel_l2(rv_d, rv_ref) < 1e-6, count
        pkg.ops.bn_finalize(stats, count, torch.ones(C, device=dev), torch.zeros(C, device=dev), rm_f, rv_f, mom, EPS)
        assert torch.equal(rm_d, rm_f) and torch.equal(rv_d, rv_f), count


# ---- 8. bn_backward ------------------------------------------------------------------------------------------------------------
MASKS = ("none", "recompute", "tensor")
G_SCALE_FULL = 0.75                  # (exact in binary: dz = g * 0.75 rounds once)


def bn_pre_activation(r32, case, mask, batch_stats):
    """float64 pre-activation of the ReLU the mask mode stands for, from the float32 ``r`` the kernel reads."""
    r = r32.double()
    if batch_stats:
        z = F.batch_norm(r, None, None, case["gamma"].double(), case["beta"].double(), True, 0.1, EPS)
    else:
        z = F.batch_norm(r, case["rm"].double(), case["rv"].double(), case["gamma"].double(), case["beta"].double(), False, 0.1, EPS)
    return z + case["idt"].double() if mask == "tensor" else z


def bn_settled_r(case, mask, batch_stats):
    """``r`` with every pre-activation |z| < 1e-4 pushed to about 1e-3, so that no mask depends on rounding."""
    r = case["r"].clone()
    if mask == "none":
        return r
    if batch_stats:
        invstd = 1.0 / torch.sqrt(r.double().var((0, 2, 3), unbiased=False) + EPS)
    else:
        invstd = 1.0 / torch.sqrt(case["rv"].double() + EPS)
    step = (1e-3 / (case["gamma"].double() * invstd)).float()
    for _ in range(8):
        bad = bn_pre_activation(r, case, mask, batch_stats).abs() < 1e-4
        if not bool(bad.any()):
            break
        r = torch.where(bad, r + v4(step), r)
    assert not bool((bn_pre_activation(r, case, mask, batch_stats).abs() < 1e-4).any())
    return r


def bn_reference(case, r32, mask, g_per_plane, batch_stats, dt):
    """(dr, dgamma, dbeta, dz, consumer output) by autograd of F.batch_norm + the consumer, evaluated in ``dt``."""
    r, gamma, beta = (t.to(dt).clone().requires_grad_(True) for t in (r32, case["gamma"], case["beta"]))
    if batch_stats:
        z = F.batch_norm(r, None, None, gamma, beta, True, 0.1, EPS)
    else:
        z = F.batch_norm(r, case["rm"].to(dt), case["rv"].to(dt), gamma, beta, False, 0.1, EPS)
    z.retain_grad()
    out = F.relu(z) if mask == "recompute" else (F.relu(z + case["idt"].to(dt)) if mask == "tensor" else z)
    HW = r.shape[2] * r.shape[3]
    if g_per_plane:                  # the global-average-pool gradient: one value per plane, g_scale = 1 / HW
        (out.sum((2, 3)) * (case["gp"].to(dt) / HW)).sum().backward()
    else:
        (out * (case["g"].to(dt) * G_SCALE_FULL)).sum().backward()
    return r.grad, gamma.grad, beta.grad, z.grad, out.detach()


@functools.lru_cache(maxsize=None)
def bn_case(shape):
    """Inputs and references of one shape, computed once and shared by the alignment variants of that shape."""
    B, C, H, W = shape
    key = f"bpr.bnb.{shape}"
    case = {"r": recipe_input(key + ".r", shape) * 1.5 + 0.3,
            "gamma": 1.0 + recipe_tensor(key + ".gamma", (C,), 0.3), "beta": recipe_tensor(key + ".beta", (C,), 0.3),
            "idt": recipe_input(key + ".idt", shape), "g": recipe_input(key + ".g", shape), "gp": recipe_input(key + ".gp", (B, C)),
            "rm": recipe_tensor(key + ".rm", (C,), 0.2), "rv": recipe_tensor(key + ".rv", (C,), 1.0).abs() + 0.5, "combos": {}}
    for mask, batch_stats in itertools.product(MASKS, (True, False)):
        r32 = bn_settled_r(case, mask, batch_stats)
        r64 = r32.double()
        if batch_stats:
            mean, invstd = r64.mean((0, 2, 3)), 1.0 / torch.sqrt(r64.var((0, 2, 3), unbiased=False) + EPS)
        else:
            mean, invstd = case["rm"].double(), 1.0 / torch.sqrt(case["rv"].double() + EPS)
        scale = case["gamma"].double() * invstd
        shift = case["beta"].double() - mean * scale
        for g_per_plane in (False, True):
            ref64 = bn_reference(case, r32, mask, g_per_plane, batch_stats, torch.float64)
            ref32 = bn_reference(case, r32, mask, g_per_plane, batch_stats, torch.float32)
            assert torch.equal(ref32[4] > 0, ref64[4] > 0) or mask == "none"       # (the masks do not depend on rounding)
            cb = dict(r=r32, stats=tuple(t.float() for t in (scale, shift, mean, invstd)), ref=ref64, cancels=None,
                      err32=tuple(rel_l2(ref32[k], ref64[k]) for k in range(3)))
            if B == 1 and g_per_plane and batch_stats and mask == "none":
                # one image, one unmasked value d per plane, batch statistics: dz is constant over the channel, so
                # dr = scale (d - mean(d) - rhat mean(d rhat)) and dgamma = d sum(rhat) are EXACTLY zero.  A relative error against
                # zero says nothing (torch's fp32 evaluation measures 1e+8 there); these two are held to the same 2e-5 relative to
                # the terms that cancel: ||scale d|| for dr, ||sum |d rhat| || for dgamma
                d = (case["gp"].double() / (H * W)).view(1, C, 1, 1).expand(shape)
                rhat = (r64 - v4(mean)) * v4(invstd)
                cb["cancels"] = (float((v4(scale) * d).norm()), float((d * rhat).abs().sum((0, 2, 3)).norm()))
                assert float(ref64[0].norm()) < 1e-9 * cb["cancels"][0] and float(ref64[1].norm()) < 1e-9 * cb["cancels"][1]
            case["combos"][(mask, batch_stats, g_per_plane)] = cb
    return case


@pytest.mark.parametrize("shape,misaligned", [
    ((3, 13, 9, 9), None),          # HW % 4 != 0: bn_bwd_reduce_kernel / bn_bwd_apply_kernel
    ((2, 5, 8, 8), "r"),            # HW % 4 == 0, r 4 bytes off: the dword kernels
    ((2, 5, 8, 8), "g"),            # HW % 4 == 0, g 4 bytes off: the dword kernels (a per-plane g is read as dwords anyway)
    ((2, 5, 8, 8), None),           # HW <= 1024: one wave per plane (<64> forms), 16 vectors for 64 lanes
    ((5, 7, 32, 32), None),         # HW = 1024: one wave per plane, four trips; 35 planes = 8 full workgroups + 3 waves
    ((1, 3, 48, 48), None),         # HW = 2304: a workgroup per plane (<256> forms), one chunk
    ((1, 2, 272, 256), None),       # HW = 69632: 17 chunks wanted, capped at 16: a second trip of the apply pass
])
def test_bn_backward_full_cross_on_every_kernel_family(pkg, dev, shape, misaligned):
    """mask mode x g_per_plane x batch_stats x want_dz (24 combinations) on each kernel family of the reduce and apply passes."""
    ops = pkg.ops
    case = bn_case(shape)
    B, C, H, W = shape
    mode = {"none": ops.MASK_NONE, "recompute": ops.MASK_RECOMPUTE, "tensor": ops.MASK_TENSOR}
    for (mask, batch_stats, g_per_plane), cb in case["combos"].items():
        dr_ref, dgamma_ref, dbeta_ref, dz_ref, out = cb["ref"]
        r_d = place(cb["r"], dev, misaligned == "r")
        g_d = place(case["gp"] if g_per_plane else case["g"], dev, misaligned == "g")
        scale, shift, mean, invstd = (t.to(dev) for t in cb["stats"])
        mask_src = out.float().to(dev) if mask == "tensor" else None
        for want_dz in (False, True):
            res = ops.bn_backward(g_d, r_d, (scale, shift), mean, invstd, mode[mask], mask_src=mask_src,
                                  g_scale=1.0 / (H * W) if g_per_plane else G_SCALE_FULL, g_per_plane=g_per_plane,
                                  want_dz=want_dz, batch_stats=batch_stats)
            assert len(res) == (4 if want_dz else 3)
            what = (mask, batch_stats, g_per_plane, want_dz)
            # rule (a): torch's fp32 autograd of the same chain against the same fp64 reference; largest values over the 12
            # references of a shape (dr / dgamma / dbeta): (3,13,9,9) 1.1e-7 / 1.3e-7 / 1.1e-7, (2,5,8,8) 8.6e-8 / 2.4e-7 / 1.1e-7,
            # (5,7,32,32) 2.0e-7 / 3.4e-7 / 5.3e-7, (1,3,48,48) 1.1e-6 / 2.9e-7 / 1.3e-6: four times any of them is below the
            # project's 2e-5, which is the bound there.  (1,2,272,256): 5.8e-5 / 2.4e-6 / 3.7e-5 -- torch's CPU BatchNorm backward
            # adds the 69632 values of a channel one after the other in fp32, which shows most with a per-plane g (equal terms):
            # up to 2.3e-4 for dr and 1.5e-4 for dbeta of those combinations, 2e-5 for the rest
            for k, (name, ref) in enumerate((("dr", dr_ref), ("dgamma", dgamma_ref), ("dbeta", dbeta_ref))):
                if cb["cancels"] is not None and k < 2:      # exactly zero by cancellation (see bn_case)
                    size = float(res[k].double().norm())
                    assert res[k].shape == ref.shape and size <= 2e-5 * cb["cancels"][k], (what, name, size, cb["cancels"][k])
                    continue
                bound = max(2e-5, 4 * cb["err32"][k])
                assert res[k].shape == ref.shape and rel_l2(res[k], ref) < bound, (what, name, rel_l2(res[k], ref), bound)
            if want_dz:              # dz = g * g_scale where the mask holds: one fp32 product, 2^-24 relative
                assert res[3].shape == dz_ref.shape and rel_l2(res[3], dz_ref) < 1e-6, (what, "dz", rel_l2(res[3], dz_ref))
