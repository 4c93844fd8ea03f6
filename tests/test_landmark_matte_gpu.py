"""GPU checks of the landmark matte (csrc/landmark_matte.hip): ``ops.matte_from_landmarks`` against the numpy fp64 model
tests/matte_ref.py (written from the definition in include/spk.h), through the aligned paste, and ``ops.LandmarkMatte`` through
``IRFD.reenact_video`` against its hand composition.

Bound, on every pixel: ``|got - model| <= 1e-7``.  Half an fp32 ulp below 1 is 3e-8 (the one rounding of the result); the two fp64
evaluations differ by contraction and the order of their sums at the 1e-10 level at these sizes; 1e-7 leaves about a factor of
three.  Where the model's ``d + grow <= -1e-6`` the output must be exactly 0, where it is ``>= softness + 1e-6`` exactly 1; each
case holds both kinds of pixel and ramp pixels (counted with the model alone in tests/test_landmark_matte_cpu.py, asserted here
again).  Each case prints its largest difference."""
import importlib

import numpy as np
import pytest
import torch

import landmark_ref as LR
import matte_ref as M
from oracle import irfd_ref as IR
from oracle.weights_recipe import fill_state_dict, recipe_noises

pytestmark = pytest.mark.gpu
BOUND = 1e-7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


def run(pkg, dev, c, pts=None, sim=None, **kw):
    """the case's call on the device, with the case's arguments unless ``kw`` replaces them"""
    args = dict(softness=c["softness"], grow=c["grow"], smooth=c["radius"])
    args.update(kw)
    pts, sim = c["pts"] if pts is None else pts, c["sim"] if sim is None else sim
    return pkg.ops.matte_from_landmarks(torch.from_numpy(pts).to(dev), torch.from_numpy(sim).to(dev), c["size"], c["contour"], **args)


def model(c, pts=None, sim=None, **kw):
    args = dict(grow=c["grow"], radius=c["radius"])
    args.update(kw)
    softness = args.pop("softness", c["softness"])
    dg = M.matte64(c["pts"] if pts is None else pts, c["sim"] if sim is None else sim, c["size"], c["contour"], softness, **args)[0]
    return dg, softness


def check(got, dg, softness, what, populated=True):
    """``got`` [N,Hs,Ws] from the device against the model's ``dg = d + grow``: the bound everywhere, exact zeros and ones"""
    assert got.dtype == torch.float32 and tuple(got.shape) == dg.shape
    got = got.cpu().numpy().astype(np.float64)
    worst = float(np.abs(got - M.ramp(dg, softness).astype(np.float64)).max())
    zero, one = dg <= -1e-6, dg >= softness + 1e-6
    between = (dg > 0) & (dg < softness)
    kinds = [int(k.sum(axis=(1, 2)).min()) for k in (zero, one, between)]
    print(f"{what}: largest |got - model| = {worst:.3e} (bound {BOUND:.0e}); per frame at least {kinds[0]} pixels that must be 0, "
          f"{kinds[1]} that must be 1, {kinds[2]} on the ramp")
    assert worst <= BOUND
    assert (got[zero] == 0.0).all() and (got[one] == 1.0).all()
    if populated:                                                         # the inputs: every frame holds all three kinds of pixel
        assert kinds[0] >= M.POPULATED[0] and kinds[1] >= M.POPULATED[1] and kinds[2] >= M.POPULATED[2], kinds
    return worst


# ---- against the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.CASES))
def test_matte_against_the_model(pkg, dev, name):
    """N = 5, K = 12, 16 x 16 and 12 x 20; the identity, rotations, s < 1 and s > 2; Kc = 3, 7 (one index twice) and 12; a concave and a
    self-crossing outline; vertices on pixel centres; grow 0, 1.5 and -1; radius 0 and 2."""
    c = M.case(name)
    got = run(pkg, dev, c)
    assert got.device.type == "cuda" and got.is_contiguous()
    check(got, *model(c), name)
    assert torch.equal(got, run(pkg, dev, c))                             # two calls on the same inputs: the same bits
    # host rows are the device rows; a host contour tensor is the list
    host = pkg.ops.matte_from_landmarks(torch.from_numpy(c["pts"]).to(dev), c["sim"].tolist(), c["size"], torch.tensor(c["contour"]),
                                        softness=c["softness"], grow=c["grow"], smooth=c["radius"])
    assert torch.equal(host, got)
    # the other grows and the other radius of the issue's list, on every outline
    for kw in (dict(grow=1.5), dict(grow=-1.0), dict(radius=2 - c["radius"])):
        if all(c[k] == v for k, v in kw.items()):
            continue
        dev_kw = {("smooth" if k == "radius" else k): v for k, v in kw.items()}
        check(run(pkg, dev, c, **dev_kw), *model(c, **kw), f"{name}, {kw}", populated=False)
    check(run(pkg, dev, c, smooth=2, sigma=3.0, softness=0.75, offset=0.5), *model(c, radius=2, sigma=3.0, softness=0.75, offset=0.5),
          f"{name}, sigma 3, softness 0.75, offset 0.5", populated=False)


def test_matte_of_the_largest_contour_over_several_workgroups(pkg, dev):
    """One frame, 64 x 64, Kc = 128 of K = 130: the contour's upper bound, and four bands of rows, a workgroup each."""
    c = M.big_case()
    assert len(c["contour"]) == 128 and c["pts"].shape == (1, 130, 2)
    check(run(pkg, dev, c), *model(c), "64 x 64, Kc = 128")


def test_drop_outs_are_bridged_fall_back_or_give_zeros(pkg, dev):
    c = M.case("crossed 12x20 grown smoothed")
    fb = np.array([(3, 2), (17, 2), (17, 9), (10, 5), (10, 5), (3, 9), (2, 5)], dtype=np.float32)
    # a frame of NaN landmarks inside the windows of its neighbours, and one landmark of another frame: bridged
    pts = c["pts"].copy()
    pts[2] = np.nan
    pts[4, c["contour"][1], 1] = np.inf
    dg, softness = model(c, pts=pts)
    assert np.isfinite(dg).all()
    check(run(pkg, dev, c, pts=pts), dg, softness, "NaN landmarks in frame 2, an Inf in frame 4, radius 2")
    # a frame whose whole window is NaN: the fallback's polygon with one, zeros without; its neighbours see only what is left
    pts = c["pts"].copy()
    pts[1:4] = np.nan
    with_fb = run(pkg, dev, c, pts=pts, smooth=1, fallback=torch.from_numpy(fb))
    dg, softness = model(c, pts=pts, radius=1, fallback=fb)
    check(with_fb, dg, softness, "frames 1-3 NaN, radius 1, a fallback")
    alone = M.signed_distance(fb.astype(np.float64), *M.centres(*c["size"])) + c["grow"]
    assert np.array_equal(dg[2], alone) and with_fb[2].any()
    assert torch.equal(with_fb, run(pkg, dev, c, pts=pts, smooth=1, fallback=torch.from_numpy(fb).to(dev)))       # a device fallback
    without = run(pkg, dev, c, pts=pts, smooth=1)
    dg, softness = model(c, pts=pts, radius=1)
    assert np.isinf(dg[2]).all() and np.isfinite(dg[[0, 1, 3, 4]]).all()
    check(without, dg, softness, "frames 1-3 NaN, radius 1, no fallback", populated=False)
    assert not without[2].any() and without[1].any() and torch.equal(without[[0, 1, 3, 4]], with_fb[[0, 1, 3, 4]])
    # one landmark without a window: that frame is zeros without a fallback, and takes that one point from it with one
    pts = c["pts"].copy()
    pts[3, c["contour"][0], 0] = np.nan
    one = run(pkg, dev, c, pts=pts, smooth=0)
    assert not one[3].any() and one[2].any()
    check(run(pkg, dev, c, pts=pts, smooth=0, fallback=fb.tolist()), *model(c, pts=pts, radius=0, fallback=fb), "one point from the fallback")
    # a frame with an invalid row (a scale outside [1/16, 16]; NaNs) contributes nothing to its neighbours' windows
    for bad in ([0.01, 0.0, 5.0, 5.0], [np.nan] * 4, [20.0, 0.0, 1.0, 1.0], [1.0, 0.0, np.inf, 0.0]):
        sim = c["sim"].copy()
        sim[1] = bad
        got = run(pkg, dev, c, sim=sim, smooth=1, fallback=torch.from_numpy(fb))
        dg, softness = model(c, sim=sim, radius=1, fallback=fb)
        check(got, dg, softness, f"row 1 = {bad}, radius 1")
        pts = c["pts"].copy()
        pts[1] = np.nan                                                    # the same as if the frame had no landmarks at all
        assert torch.equal(got, run(pkg, dev, c, pts=pts, smooth=1, fallback=torch.from_numpy(fb)))


def test_a_frame_does_not_depend_on_its_batch(pkg, dev):
    """At radius = 0 frame 2 alone and in the batch give the same bits; many frames (more bands than the grid holds) repeat them."""
    for name in ("star 16x16", "star 12x20 shrunk"):
        c = M.case(name)
        batch = run(pkg, dev, c, smooth=0)
        assert torch.equal(run(pkg, dev, c, pts=c["pts"][2:3], sim=c["sim"][2:3], smooth=0), batch[2:3])
    many = run(pkg, dev, c, pts=np.tile(c["pts"], (500, 1, 1)), sim=np.tile(c["sim"], (500, 1)), smooth=0)    # 2500 bands, a grid of 2048
    assert torch.equal(many, batch.repeat(500, 1, 1))


# ---- through the paste ------------------------------------------------------------------------------------------------------------
def test_the_paste_leaves_every_byte_outside_the_outline_alone(pkg, dev):
    """``frames_paste_u8_aligned(matte=matte_from_landmarks(...))`` on 40 x 56 frames.  A frame pixel samples the matte with a
    triangle of half-width r = max(1, 1 / s) around (u, v) = sim^-1 of its centre: every matte pixel it can reach is within
    r sqrt(2) of (u, v), and the signed distance changes by at most the distance moved, so where the model's
    d(u, v) + grow <= -r sqrt(2) every sample is 0 and the byte must stay.  Well inside the outline the generated face lands."""
    ops = pkg.ops
    Hs = Ws = 16
    rows = ops.similarity_rows([(20.0, 28.0), (17.5, 30.2), (22.0, 25.0)], [30.0, 12.0, 36.0], [0.0, 0.5, -0.8], Hs).numpy()
    g = M.base_points(Hs, Ws)[None] + 0.3 * np.random.default_rng(3).standard_normal((3, M.K, 2))
    pts = np.stack([LR.apply(rows[n:n + 1], g[n])[0] for n in range(3)]).astype(np.float32)
    frames = torch.randint(0, 256, (3, 40, 56, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8)
    x = torch.full((3, 3, Hs, Ws), 0.25)                                   # quantises to 159 or 160: a change shows wherever it lands
    frames[frames == 159] = 7
    frames[frames == 160] = 9
    for grow in (0.0, 1.5):
        matte = ops.matte_from_landmarks(torch.from_numpy(pts).to(dev), torch.from_numpy(rows).to(dev), (Hs, Ws), M.STAR, softness=1.5,
                                         grow=grow)
        got = ops.frames_paste_u8_aligned(x.to(dev), frames.to(dev), torch.from_numpy(rows).to(dev), matte=matte).cpu()
        P, hole = M.outline(pts, rows, M.STAR)
        X, Y = M.centres(40, 56)
        stay, land = 0, 0
        for n in range(3):
            a, c, tx, ty = rows[n].astype(np.float64)
            s2 = a * a + c * c
            u, v = (a * (X - tx) + c * (Y - ty)) / s2, (-c * (X - tx) + a * (Y - ty)) / s2
            d = M.signed_distance(P[n], u, v)
            r = max(1.0, 1.0 / np.sqrt(s2))
            outside = torch.from_numpy(d + grow <= -r * np.sqrt(2.0) - 1e-9)
            inside = torch.from_numpy(d + grow >= 1.5 + r * np.sqrt(2.0) + 1e-9)
            assert torch.equal(got[n][outside], frames[n][outside]), (grow, n)
            assert bool(((got[n][inside] == 159) | (got[n][inside] == 160)).all()), (grow, n)
            stay, land = stay + int(outside.sum()), land + int(inside.sum())
        print(f"paste, grow = {grow}: {stay} frame pixels outside the outline untouched, {land} pixels well inside replaced")
        assert stay >= 3 * 1200 and land >= 20 and not torch.equal(got, frames)


# ---- the public interface ---------------------------------------------------------------------------------------------------------
SIZE = 128          # encoder input of the model-level case, as tests/test_landmark_gpu.py
TEMPLATE5 = [(44.0, 52.0), (84.0, 52.0), (64.0, 74.0), (48.0, 96.0), (80.0, 96.0)]      # eyes, nose, mouth corners in the 128 image
CONTOUR = [0, 1, 4, 3]                                                    # eyes and mouth corners, in outline order


def frames(seed, *shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.fixture(scope="module")
def irfd(dev):
    import model as model_py
    m = model_py.IRFD()
    sd = IR.irfd_recipe_state_dict()
    sd.update({"Gd." + k: v for k, v in fill_state_dict(m.Gd.state_dict(), prefix="Gd.").items()})
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("D.") for k in missing)
    return m.to(dev).eval()


def test_reenact_video_landmark_matte_is_its_hand_composition(irfd, pkg, dev, monkeypatch):
    """The small clip of tests/test_landmark_gpu.py (T = 3 BGR frames of 64 x 80, five landmarks): ``matte=LandmarkMatte(contour)``
    is ``matte=`` the tensor ``matte_from_landmarks`` makes from the rows the paste uses, bit for bit, for ``chunk=1`` as for
    ``chunk=T``, with one launch of the matte per call."""
    ops, T = pkg.ops, 3
    true = ops.similarity_rows([(30.3, 41.6), (33.9, 38.2), (28.4, 44.1)], [44.0, 52.0, 36.0], [0.2, -0.3, 0.1], SIZE)
    rng = np.random.default_rng(9)
    lm = torch.from_numpy((LR.apply(true.numpy(), TEMPLATE5) + rng.standard_normal((T, 5, 2)) / 3).astype(np.float32)).to(dev)
    ident, pose = frames(31, 56, 72, 3).to(dev), frames(32, T, 64, 80, 3).to(dev)
    noises = [n.to(dev) for n in recipe_noises("frame_io", T, 256)]
    kw = dict(size=SIZE, channel_order="bgr", noises=noises, paste=True, feather=2)
    la = ops.LandmarkAlign(lm, TEMPLATE5, offset=0.25, smooth=1)
    # by hand: the rows of the clip, (a, c) scaled by size / R in fp32 as the paste scales them; the template's contour scaled by R / size
    R = 256
    rows = ops.smooth_similarity_rows(ops.similarity_from_landmarks(lm, TEMPLATE5, offset=0.25), 1)
    rows_R = rows * torch.tensor([SIZE / R, SIZE / R, 1.0, 1.0], dtype=torch.float32, device=dev)
    fallback = torch.tensor(TEMPLATE5, dtype=torch.float32)[CONTOUR] * torch.tensor(R / SIZE, dtype=torch.float32)
    matte = ops.matte_from_landmarks(lm, rows_R, R, CONTOUR, softness=6.0, grow=3.0, offset=0.25, fallback=fallback, smooth=1, sigma=la.sigma)
    dg = M.matte64(lm.cpu().numpy(), rows_R.cpu().numpy(), (R, R), CONTOUR, 6.0, grow=3.0, offset=0.25, radius=1, sigma=la.sigma)[0]
    check(matte, dg, 6.0, "the clip's matte, 256 x 256", populated=False)
    assert int((matte == 1).sum()) > 3 * 2000 and int((matte == 0).sum()) > 3 * 30000
    want = irfd.reenact_video(ident, pose, align=la, matte=matte, chunk=2, **kw)
    assert not torch.equal(want, irfd.reenact_video(ident, pose, align=la, chunk=2, **kw)) and not torch.equal(want, pose)
    lib = pkg._lib.lib()
    real, calls = lib.spk_matte_from_landmarks, []
    monkeypatch.setattr(lib, "spk_matte_from_landmarks", lambda *a: calls.append(a[1]) or real(*a))
    for chunk in (1, 2, T):
        got = irfd.reenact_video(ident, pose, align=la, matte=ops.LandmarkMatte(CONTOUR, softness=6.0, grow=3.0), chunk=chunk, **kw)
        assert calls == [T], (chunk, calls)                                # one launch, over the whole clip
        calls.clear()
        assert torch.equal(got, want), chunk
    # landmarks of its own (the same ones), every argument spelled out, a colour match on top: the tensor's path again
    own = ops.LandmarkMatte(CONTOUR, landmarks=lm, softness=6.0, grow=3.0, offset=0.25, fallback=fallback / 2, smooth=1, sigma=la.sigma)
    got = irfd.reenact_video(ident, pose, align=rows, matte=own, chunk=1, colour_match=True, **kw)
    monkeypatch.undo()
    assert torch.equal(got, irfd.reenact_video(ident, pose, align=rows, matte=matte, chunk=T, colour_match=True, **kw))
    # a drop-out at frame 1 with smooth=0: the matte of that frame is the template's outline, not a hole
    lm_bad = lm.clone()
    lm_bad[1, 3] = float("nan")
    rows0 = ops.similarity_from_landmarks(lm, TEMPLATE5) * torch.tensor([0.5, 0.5, 1.0, 1.0], device=dev)
    made = ops.LandmarkMatte(CONTOUR, landmarks=lm_bad).bind(ops.LandmarkAlign(lm, TEMPLATE5), T)(pkg.frames.Aligned(rows0, (R, R)), (SIZE, SIZE))
    assert made[1].any() and torch.equal(made, ops.matte_from_landmarks(lm_bad, rows0, R, CONTOUR, fallback=fallback))
