"""GPU tests of the counter-based decoder noise (csrc/noise.hip; definition: include/spk.h): ``spk_noise_fill`` against the fp64
numpy restatement (tests/philox_ref.py) on every store branch, its invariances bit for bit, the statistics of the device values,
the seeded ``DecoderPlan`` against explicit noise, and seeded ``IRFD.reenact`` / ``reenact_video``.

The bound of the value comparisons is measured, not guessed: the largest |device - fp64 restatement| over the cases of
``FILL_CASES`` and the ``frame0 = 2**32 + 5`` case, as printed by ``test_fill_vs_restatement`` on an MI355X, is
``MEASURED_MAX_DEV``; the bound is 4x that, and must stay at or below 1e-5 -- a wrong bit anywhere gives an error of order 1.
(fp32 logf / sqrtf / sincospi and one product on |z| <= 5.77 -- ulp 4.8e-7 -- put the expectation at a few 1e-7.)  Measured
per case: 3.17e-7 (vector [16, 64, 64]), 3.9e-8 ([1]), 1.31e-7 ([5]), 3.42e-7 ([4097]), 3.17e-7 (unaligned dst), 5.89e-7 (second
trip), 2.05e-7 (frame0 = 2**32 + 5): BOUND = 2.356e-6."""
import importlib

import numpy as np
import pytest
import torch

import philox_ref as P
from conftest import rel_l2
from oracle import irfd_ref as IR
from oracle.weights_recipe import fill_state_dict, recipe_input

pytestmark = pytest.mark.gpu

MEASURED_MAX_DEV = 5.890e-7        # largest |device - restatement| over the fill cases, measured on an MI355X (the 2 098 180-pixel plane)
BOUND = 4 * MEASURED_MAX_DEV
TOL_FRAMES = 5e-4                  # the frame bound of tests/test_reenact_gpu.py
SEED = 0x9E3779B97F4A7C15
TRIP = 2048 * 256 * 4              # pixels one trip of the grid-stride loop covers: GRID_CAP workgroups x 256 threads x 4 (csrc/noise.hip)

# (name, hw, B, dst offset in floats from a 16-byte boundary): every store branch of the kernel
FILL_CASES = [
    ("vector: the decoder's first planes", [16, 64, 64], 2, 0),
    ("scalar: one pixel", [1], 3, 0),
    ("scalar: a tail of one", [5], 3, 0),
    ("scalar: many blocks and a tail", [4097], 3, 0),
    ("scalar: dst one float past a 16-byte boundary", [16, 64], 2, 1),
    ("vector: a second trip of the grid-stride loop", [TRIP + 1028], 1, 0),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


def _fill(pkg, dev, hw, B, seed, *, offset=0, **kw):
    n = B * sum(hw)
    store = torch.full((n + offset + 4,), float("nan"), device=dev)
    assert store.data_ptr() % 16 == 0
    dst = store[offset:offset + n]
    pkg.ops.noise_fill(dst, hw, B, seed, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(store[:offset]).all() and torch.isnan(store[offset + n:]).all(), "wrote outside dst"
    return dst


def _max_dev(got, hw, B, seed, frame0, **kw):
    ref = np.concatenate([a.reshape(-1) for a in P.noise_layers(seed, frame0, hw, B, **kw)])
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float(np.abs(got - ref).max())


@pytest.mark.parametrize("name,hw,B,offset", FILL_CASES, ids=[c[0] for c in FILL_CASES])
def test_fill_vs_restatement(pkg, dev, name, hw, B, offset):
    assert BOUND <= 1e-5
    assert name.startswith("vector") == (offset == 0 and all(v % 4 == 0 for v in hw))
    got = _fill(pkg, dev, hw, B, SEED, offset=offset, frame0=3)
    err = _max_dev(got, hw, B, SEED, 3)
    print(f"noise fill [{name}] hw={hw} B={B}: max |device - fp64 restatement| = {err:.3e} (bound {BOUND:.1e})")
    assert err <= BOUND
    if offset:       # the scalar stores carry the bits of the float4 stores
        assert torch.equal(got, _fill(pkg, dev, hw, B, SEED, frame0=3))


def test_fill_at_a_frame_index_past_32_bits(pkg, dev):
    hw, B, f0 = [16, 64], 2, 2 ** 32 + 5
    got = _fill(pkg, dev, hw, B, SEED, frame0=f0)
    err = _max_dev(got, hw, B, SEED, f0)
    print(f"noise fill frame0=2**32+5: max |device - fp64 restatement| = {err:.3e}")
    assert err <= BOUND
    assert not torch.equal(got, _fill(pkg, dev, hw, B, SEED, frame0=5))          # the high word of the frame is live


@pytest.fixture(scope="module")
def decoder_fill(pkg, dev):
    shapes = pkg.SynthesisNetwork().noise_shapes(5)
    assert len(shapes) == 13 and shapes[-1] == (5, 1, 256, 256)
    return shapes, pkg.ops.decoder_noise(shapes, SEED, device=dev)


def test_invariance_frames(pkg, dev, decoder_fill):
    shapes, full = decoder_fill
    three = pkg.ops.decoder_noise([(3,) + s[1:] for s in shapes], SEED, frame0=2, device=dev)
    for a, b in zip(full, three):
        assert b.shape[0] == 3 and torch.equal(a[2:5], b)
    assert not torch.equal(full[5][0], full[5][1])


def test_invariance_layers(pkg, dev, decoder_fill):
    shapes, full = decoder_fill
    hw = [s[2] * s[3] for s in shapes]
    alone = _fill(pkg, dev, hw[3:5], 5, SEED, layer0=3)
    assert torch.equal(alone, torch.cat([full[3].reshape(-1), full[4].reshape(-1)]))
    assert hw[3] == hw[4] and not torch.equal(full[3], full[4])                     # same shape, another layer id


def test_invariance_fixed(pkg, dev, decoder_fill):
    shapes, full = decoder_fill
    fixed = pkg.ops.decoder_noise(shapes, SEED, fixed=True, device=dev)
    for a, f in zip(full, fixed):
        assert f.shape == a.shape
        for b in range(5):
            assert torch.equal(f[b], a[0])


def test_statistics_of_the_device_values(pkg, dev):
    """The CPU test's statistics (seed 1234, layer 12, frame 0, n = 2**18; frame 1 and layer 11 as the other samples) on what
    the kernel writes: each within +-4 of its own standard error."""
    n = 2 ** 18
    z = _fill(pkg, dev, [n], 1, 1234, layer0=12).cpu().numpy()
    other_frame = _fill(pkg, dev, [n], 1, 1234, layer0=12, frame0=1).cpu().numpy()
    other_layer = _fill(pkg, dev, [n], 1, 1234, layer0=11).cpu().numpy()
    st = P.standard_errors(z, other_frame, other_layer)
    print("device statistics (standard errors):", {k: round(v, 2) for k, v in st.items()}, "max |z|", float(np.abs(z).max()))
    for name, v in st.items():
        assert abs(v) <= 4.0, (name, v)
    assert float(np.abs(z).max()) <= 5.77


# ---- the seeded plan ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def syn32(pkg, dev):
    s = pkg.SynthesisNetwork(resolution=32).eval()
    s.load_state_dict(fill_state_dict(s.state_dict(), prefix="noise.syn32."))
    assert float(s.layers[1].noise1.weight.detach().abs().max()) > 0
    return s.to(dev)


@pytest.mark.parametrize("algo", ["auto", "direct"])
def test_seeded_plan_equals_explicit_noise(pkg, dev, syn32, algo, monkeypatch):
    L, PL = pkg._lib, importlib.import_module("speak-hack_amd.plan")
    B = 3
    w = recipe_input("noise.syn32.w", (B, syn32.num_layers, 512)).to(dev)
    shapes = syn32.noise_shapes(B)
    with torch.no_grad(), pkg.ops.conv3x3_algo(algo):
        got = syn32(w, seed=7, frame0=2)
        ref = syn32(w, noises=pkg.ops.decoder_noise(shapes, 7, frame0=2, device=dev))
        assert got.shape == (B, 3, 32, 32) and torch.equal(got, ref)
        row = pkg.ops.decoder_noise([(1,) + s[1:] for s in shapes], 7, frame0=2, device=dev)
        got_fixed = syn32(w, seed=7, frame0=2, fixed_noise=True)
        assert torch.equal(got_fixed, syn32(w, noises=[n.expand(B, -1, -1, -1).contiguous() for n in row]))
        assert not torch.equal(got_fixed, got)
        # the seeded forward is the launch list alone and leaves the device generator where it was
        plan = next(p for p in syn32.__dict__["_plans"].values() if isinstance(p, PL.DecoderPlan) and p.seeded and p.B == B)
        assert plan.ops[0][0] == L.OP_NOISE_FILL and [k for k, _ in plan.ops].count(L.OP_NOISE_FILL) == 1
        lib = L.lib()
        calls = {"list": 0, "fill": 0}
        real_list, real_fill = lib.spk_launch_list, lib.spk_noise_fill

        def count_list(*a):
            calls["list"] += 1
            return real_list(*a)

        def count_fill(*a):
            calls["fill"] += 1
            return real_fill(*a)

        monkeypatch.setattr(lib, "spk_launch_list", count_list)
        monkeypatch.setattr(lib, "spk_noise_fill", count_fill)
        rng = torch.cuda.get_rng_state(dev)
        again = syn32(w, seed=7, frame0=2)
        monkeypatch.undo()
        assert calls == {"list": 1, "fill": 0}, calls
        assert torch.equal(torch.cuda.get_rng_state(dev), rng) and torch.equal(again, got)
        syn32(w)                                                            # the unseeded run draws from the device generator
        assert not torch.equal(torch.cuda.get_rng_state(dev), rng)
        # launch by launch (no plan): the list comes from ops.decoder_noise
        syn32.use_plan = False
        try:
            assert torch.equal(syn32(w, seed=7, frame0=2), syn32(w, noises=pkg.ops.decoder_noise(shapes, 7, frame0=2, device=dev)))
        finally:
            del syn32.use_plan


def test_plan_run_refuses_mixed_arguments(pkg, dev, syn32):
    PL = importlib.import_module("speak-hack_amd.plan")
    w = recipe_input("noise.syn32.w2", (2, syn32.num_layers, 512)).to(dev)
    seeded, plain = PL.DecoderPlan(syn32, 2, dev, seeded=True), PL.DecoderPlan(syn32, 2, dev)
    noises = pkg.ops.decoder_noise(syn32.noise_shapes(2), 1, device=dev)
    with pytest.raises(ValueError):
        seeded.run(w, noises, seed=1)
    with pytest.raises(ValueError):
        seeded.run(w)
    with pytest.raises(ValueError):
        plain.run(w, seed=1)
    with pytest.raises(ValueError):
        seeded.run(w, seed=2 ** 64)
    assert torch.equal(seeded.run(w, seed=1), plain.run(w, noises))


# ---- reenact ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def irfd_and_sd(dev):
    import model
    m = model.IRFD()
    sd = IR.irfd_recipe_state_dict()
    sd.update({"Gd." + k: v for k, v in fill_state_dict(m.Gd.state_dict(), prefix="Gd.").items()})
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("D.") for k in missing)
    return m.to(dev).eval(), sd


@pytest.fixture(scope="module")
def clip(pkg, dev, irfd_and_sd):
    """64^2 inputs, T = 5; ``dn``: the explicit noise of seed 11; ``base``: the seeded clip in chunks of 2."""
    m, _ = irfd_and_sd
    T = 5
    ident = recipe_input("noise.reenact.id", (1, 3, 64, 64), "uniform").to(dev)
    pose = recipe_input("noise.reenact.pose", (T, 3, 64, 64), "uniform").to(dev)
    emo = recipe_input("noise.reenact.emo", (T, 3, 64, 64), "uniform").to(dev)
    dn = pkg.ops.decoder_noise(m.Gd.synthesis.noise_shapes(T), 11, device=dev)
    base = m.reenact(ident, pose, emo, seed=11, chunk=2)
    assert base.shape == (T, 3, 256, 256) and base.dtype == torch.float32
    return ident, pose, emo, dn, base


def test_reenact_seed_equals_explicit_noise(irfd_and_sd, clip):
    m, _ = irfd_and_sd
    ident, pose, emo, dn, base = clip
    assert torch.equal(base, m.reenact(ident, pose, emo, noises=dn, chunk=2))
    fixed = m.reenact(ident, pose, emo, seed=11, noise="fixed", chunk=2)
    row0 = [n[:1].expand(5, -1, -1, -1).contiguous() for n in dn]
    assert torch.equal(fixed, m.reenact(ident, pose, emo, noises=row0, chunk=2))
    assert not torch.equal(fixed[1], base[1])


def test_reenact_seed_is_invariant_under_chunking_and_slicing(irfd_and_sd, clip):
    """Chunkings are not compared bit for bit (a plan's kernel routes depend on B): the frame bound of test_reenact_gpu.py."""
    m, _ = irfd_and_sd
    ident, pose, emo, dn, base = clip
    err = rel_l2(m.reenact(ident, pose, emo, seed=11, chunk=5), base)
    unseeded = rel_l2(m.reenact(ident, pose, emo, chunk=5), m.reenact(ident, pose, emo, chunk=2))
    print(f"reenact chunk=5 against chunk=2: rel-L2 {err:.3e} at seed 11, {unseeded:.3e} without a seed")
    assert err < TOL_FRAMES < unseeded                  # (the noise term is live in the fixture)
    part = m.reenact(ident, pose[2:5], emo[2:5], seed=11, frame0=2, chunk=2)
    err = rel_l2(part, base[2:5])
    print(f"reenact frames [2:5] rendered alone with frame0=2: rel-L2 {err:.3e}")
    assert err < TOL_FRAMES
    assert rel_l2(m.reenact(ident, pose[2:5], emo[2:5], seed=11, chunk=2), base[2:5]) > TOL_FRAMES      # frame0 is live


def test_reenact_video_seeded(pkg, dev, irfd_and_sd):
    m, _ = irfd_and_sd
    g = torch.Generator().manual_seed(5)
    ident = torch.randint(0, 256, (50, 70, 3), generator=g, dtype=torch.uint8).to(dev)
    pose = torch.randint(0, 256, (3, 90, 80, 3), generator=g, dtype=torch.uint8).to(dev)
    got = m.reenact_video(ident, pose, size=64, seed=11, chunk=2)
    f = pkg.ops.frames_from_u8
    ref = m.reenact(f(ident, 64), f(pose, 64), seed=11, chunk=2, output="uint8")
    assert got.dtype == torch.uint8 and got.shape == (3, 256, 256, 3) and torch.equal(got, ref)
    fixed = m.reenact_video(ident, pose, size=64, seed=11, noise="fixed", frame0=4, chunk=2)
    assert torch.equal(fixed, m.reenact(f(ident, 64), f(pose, 64), seed=11, noise="fixed", frame0=4, chunk=2, output="uint8"))


def test_nothing_moved_without_a_seed(pkg, irfd_and_sd, clip):
    m, _ = irfd_and_sd
    L, PL = pkg._lib, importlib.import_module("speak-hack_amd.plan")
    ident, pose, emo, dn, base = clip
    before = m.reenact(ident, pose, emo, noises=dn, chunk=2)
    plans = [p for p in m.Gd.__dict__["_plans"].values() if isinstance(p, PL.DecoderPlan) and p.B == 2 and p.output == "f32"]
    plain = [p for p in plans if not p.seeded]
    assert plain and all(L.OP_NOISE_FILL not in [k for k, _ in p.ops] for p in plain)
    m.reenact(ident, pose, emo, seed=12, noise="fixed", chunk=2)
    seeded = [p for p in m.Gd.__dict__["_plans"].values() if isinstance(p, PL.DecoderPlan) and p.B == 2 and p.output == "f32" and p.seeded]
    assert seeded and all(p.ops[0][0] == L.OP_NOISE_FILL and len(p.ops) == len(plain[0].ops) + 1 for p in seeded)
    assert torch.equal(m.reenact(ident, pose, emo, noises=dn, chunk=2), before)       # seeded and unseeded plans share no state
