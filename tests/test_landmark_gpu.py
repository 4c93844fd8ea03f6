"""GPU checks of landmarks -> rows (csrc/landmark_sim.hip): ``ops.similarity_from_landmarks`` and ``ops.smooth_similarity_rows``
against the numpy fp64 model tests/landmark_ref.py (written from the definitions in include/spk.h), and ``ops.LandmarkAlign`` /
``identity_align`` through ``IRFD.reenact_video`` against their hand compositions.

Bound, on every number of every row: ``|got - want| <= spacing(float32(|want|)) + 1e-9`` -- one rounding to fp32 (half a
spacing), a tie the model rounds the other way (the other half), and the order of the fp64 sums (a 64-lane strided sum plus a
butterfly against ``np.sum``: <= 2e-12 on these cases).  The NaN pattern must be the model's exactly.  Each case prints its
largest ratio to the bound."""
import importlib

import numpy as np
import pytest
import torch

import landmark_ref as R
from oracle import irfd_ref as IR
from oracle.weights_recipe import fill_state_dict, recipe_noises

pytestmark = pytest.mark.gpu
N = 6
KS = [2, 5, 68, 130]                            # K = 130: a lane takes three landmarks


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


def bits(t):
    """float32 rows as their bit patterns: what ``bit for bit`` compares, NaNs included"""
    return t.detach().cpu().contiguous().view(torch.int32)


def check(got, want, what):
    ratio = R.compare(got.cpu().numpy(), want)
    print(f"{what}: largest |got - model| / bound = {ratio:.3e}; NaN rows {int(np.isnan(want).all(axis=1).sum())} of {len(want)}")
    assert ratio <= 1.0
    return ratio


# ---- the fit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_fit_against_the_model(pkg, dev, K):
    """No weights, one broadcast set and a set per frame; NaN / Inf coordinates, zero / negative / NaN / Inf weights; offset 0.5."""
    f = pkg.ops.similarity_from_landmarks
    c = R.case(K, N)
    pts, tmpl = torch.from_numpy(c["pts"]).to(dev), torch.from_numpy(c["tmpl"])
    wb, wf = torch.from_numpy(c["w_bcast"]), torch.from_numpy(c["w_frames"])
    valid = 0
    for name, weights, model_weights, offset in (("no weights", None, None, 0.0), ("no weights, offset 0.5", None, None, 0.5),
                                                 ("broadcast weights", wb.to(dev), c["w_bcast"], 0.0),
                                                 ("weights per frame, offset 0.5", wf.to(dev), c["w_frames"], 0.5)):
        got = f(pts, tmpl, weights=weights, offset=offset)
        assert got.dtype == torch.float32 and got.shape == (N, 4) and got.device == pts.device
        want = R.fit(c["pts"], c["tmpl"], model_weights, offset)
        check(got, want, f"fit, K = {K}, {name}")
        valid += int((~np.isnan(want)).all(axis=1).sum())
    assert valid >= (8 if K == 2 else 20)
    # one set of weights: from the host, from the device, and expanded to a copy per frame -- the same bits
    a = f(pts, tmpl, weights=wb.to(dev))
    assert torch.equal(bits(f(pts, tmpl, weights=wb)), bits(a)) and torch.equal(bits(f(pts, tmpl, weights=wb.tolist())), bits(a))
    assert torch.equal(bits(f(pts, tmpl, weights=wb.to(dev).expand(N, K).contiguous())), bits(a))
    # a device template is the host template; landmarks that are not contiguous are made so
    assert torch.equal(bits(f(pts, tmpl.to(dev), weights=wb.to(dev))), bits(a))
    wide = torch.zeros(N, K, 3, device=dev)
    wide[:, :, :2] = pts
    assert not wide[:, :, :2].is_contiguous() and torch.equal(bits(f(wide[:, :, :2], tmpl, weights=wb.to(dev))), bits(a))


@pytest.mark.parametrize("K", KS)
def test_fit_of_a_frame_does_not_depend_on_its_batch(pkg, dev, K):
    f = pkg.ops.similarity_from_landmarks
    c = R.case(K, N, seed=1, bad=False)
    pts, tmpl, wf = torch.from_numpy(c["pts"]).to(dev), torch.from_numpy(c["tmpl"]), torch.from_numpy(c["w_frames"]).to(dev)
    batch, batch_w = f(pts, tmpl), f(pts, tmpl, weights=wf)
    assert not torch.isnan(batch).any() and not torch.isnan(batch_w).any()
    assert torch.equal(bits(f(pts[2:3], tmpl)), bits(batch[2:3]))
    assert torch.equal(bits(f(pts[2:3], tmpl, weights=wf[2:3])), bits(batch_w[2:3]))
    many = f(pts.repeat(1400, 1, 1), tmpl)                                # 8400 frames: more than the grid holds, a second trip
    assert torch.equal(bits(many), bits(batch.repeat(1400, 1)))


def test_drop_out_frames_are_nan_rows_and_give_frames_of_shift(pkg, dev):
    """One participant; all weights zero; participants on one template point: four NaNs each, and the way in then writes shift_c."""
    ops = pkg.ops
    tmpl = torch.tensor([(5.0, 6.0), (5.0, 6.0), (5.0, 6.0), (12.0, 13.0), (15.0, 9.0)])
    pts = torch.from_numpy(R.apply([[1.5, 0.2, 10, 8]] * 3, tmpl.numpy()).astype(np.float32))
    w = torch.tensor([[0.0, 0, 0, 1, 0], [0.0, 0, 0, 0, 0], [1.0, 1, 1, 0, 0]])
    rows = ops.similarity_from_landmarks(pts.to(dev), tmpl, weights=w.to(dev))
    assert np.isnan(R.fit(pts.numpy(), tmpl.numpy(), w.numpy())).all() and bool(torch.isnan(rows).all())
    u8 = torch.randint(0, 256, (3, 40, 56, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    mean, std = (0.4, 0.5, 0.6), (0.2, 0.25, 0.5)
    got = ops.frames_from_u8_aligned(u8.to(dev), 16, rows, mean=mean, std=std)
    shift = torch.tensor([np.float32(-m / s) for m, s in zip(mean, std)], dtype=torch.float32).view(1, 3, 1, 1)
    assert torch.equal(got.cpu(), shift.expand(3, 3, 16, 16))
    full = ops.similarity_from_landmarks(pts.to(dev), tmpl)               # with every landmark the rows are there
    check(full, R.fit(pts.numpy(), tmpl.numpy()), "fit, all five landmarks of the drop-out clip")
    assert not torch.isnan(full).any()


# ---- the smoothing ----------------------------------------------------------------------------------------------------------------
def some_rows(n, seed=0):
    rng = np.random.default_rng(seed)
    s, th = rng.uniform(0.3, 3.0, n), rng.uniform(-0.5, 0.5, n)
    return np.stack([s * np.cos(th), s * np.sin(th), rng.uniform(-500, 4000, n), rng.uniform(-500, 4000, n)], axis=1).astype(np.float32)


def test_smooth_against_the_model(pkg, dev):
    f = pkg.ops.smooth_similarity_rows
    rows = some_rows(12)
    rows[0] = rows[4] = np.nan
    check(f(torch.from_numpy(rows).to(dev), 2, 1.0), R.smooth(rows, 2, 1.0), "smooth, N = 12, radius 2, NaN rows at 0 and 4")
    rows = some_rows(12, 1)
    rows[5:10] = np.nan                                                    # 2 * radius + 1 frames: the middle one has no neighbour
    rows[2, 3], rows[11, 0] = np.nan, np.inf                               # a row with one number that is not finite takes no part
    got = f(torch.from_numpy(rows).to(dev), 2, 1.0)
    check(got, R.smooth(rows, 2, 1.0), "smooth, N = 12, radius 2, a run of five NaN rows")
    assert bool(torch.isnan(got[7]).all()) and int(torch.isnan(got).any(dim=1).sum()) == 1
    host = f(rows.tolist(), 2, 1.0)                                        # host rows are uploaded unchecked
    assert host.is_cuda and torch.equal(bits(host), bits(got))
    rows = some_rows(5, 2)
    rows[1] = np.nan
    check(f(torch.from_numpy(rows).to(dev), 64, 7.5), R.smooth(rows, 64, 7.5), "smooth, N = 5, radius 64")
    check(f(torch.from_numpy(rows).to(dev), 3), R.smooth(rows, 3, 1.5), "smooth, N = 5, radius 3, the default sigma")
    big = some_rows(3000, 3)                                               # more than one workgroup
    check(f(torch.from_numpy(big).to(dev), 5, 2.0), R.smooth(big, 5, 2.0), "smooth, N = 3000, radius 5")


def test_smooth_copies_at_radius_zero_and_keeps_constant_rows(pkg, dev):
    f = pkg.ops.smooth_similarity_rows
    rows = some_rows(9, 4)
    rows[2, 3], rows[5], rows[1, 1], rows[7] = np.nan, np.inf, -0.0, np.nan
    src = torch.from_numpy(rows).to(dev)
    got = f(src, 0)
    part = torch.from_numpy(np.isfinite(rows).all(axis=1))
    assert got.data_ptr() != src.data_ptr() and int(part.sum()) == 6
    assert torch.equal(bits(got)[part], bits(src)[part]) and bool(torch.isnan(got.cpu()[~part]).all())
    row = np.array([0.8125, -0.3333, 412.75, 96.1], dtype=np.float32)
    const = np.tile(row, (9, 1))
    const[3] = np.nan                                                      # bridged from its neighbours
    for radius, sigma in ((2, 1.0), (64, 3.3), (1, None)):
        got = f(torch.from_numpy(const).to(dev), radius, sigma)
        assert torch.equal(bits(got), bits(torch.from_numpy(np.tile(row, (9, 1))))), (radius, sigma)


# ---- the public interface ---------------------------------------------------------------------------------------------------------
SIZE = 128          # encoder input of the model-level cases, as tests/test_align_gpu.py
TEMPLATE5 = [(44.0, 52.0), (84.0, 52.0), (64.0, 74.0), (48.0, 96.0), (80.0, 96.0)]      # eyes, nose, mouth corners in the 128 image


def frames(seed, *shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.fixture(scope="module")
def irfd(dev):
    import model
    m = model.IRFD()
    sd = IR.irfd_recipe_state_dict()
    sd.update({"Gd." + k: v for k, v in fill_state_dict(m.Gd.state_dict(), prefix="Gd.").items()})
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("D.") for k in missing)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def clip(pkg, dev):
    """Identity photo, T = 3 BGR video frames of 64 x 80, five landmarks per frame made from three known transforms plus a third
    of a pixel of noise, the identity's landmarks and its row, explicit noise."""
    T = 3
    true = pkg.ops.similarity_rows([(30.3, 41.6), (33.9, 38.2), (28.4, 44.1)], [44.0, 52.0, 36.0], [0.2, -0.3, 0.1], SIZE)
    rng = np.random.default_rng(9)
    lm = torch.from_numpy((R.apply(true.numpy(), TEMPLATE5) + rng.standard_normal((T, 5, 2)) / 3).astype(np.float32)).to(dev)
    rows1 = pkg.ops.similarity_rows([(27.2, 35.1)], [40.0], [-0.15], SIZE)
    lm1 = torch.from_numpy(R.apply(rows1.numpy(), TEMPLATE5).astype(np.float32)).to(dev)
    return dict(T=T, ident_u8=frames(31, 56, 72, 3).to(dev), pose_u8=frames(32, T, 64, 80, 3).to(dev), emo_u8=frames(33, T, 64, 80, 3).to(dev),
                lm=lm, lm1=lm1, rows1=rows1, noises=[n.to(dev) for n in recipe_noises("frame_io", T, 256)])


def test_reenact_video_landmark_align_is_align_with_its_rows(irfd, pkg, clip, dev, monkeypatch):
    """``align=LandmarkAlign(..., smooth=1)`` is ``align=`` the smoothed fit, bit for bit, whatever the chunk; one fit launch and one
    smoothing launch per call, and no smoothing launch with ``smooth=0``."""
    c, ops = clip, pkg.ops
    raw = ops.similarity_from_landmarks(c["lm"], TEMPLATE5)
    rows = ops.smooth_similarity_rows(raw, 1)
    check(raw, R.fit(c["lm"].cpu().numpy(), TEMPLATE5), "the clip's rows: fit")
    check(rows, R.smooth(raw.cpu().numpy(), 1, 0.5), "the clip's rows: smooth")
    assert not torch.equal(rows, raw)
    lib = pkg._lib.lib()
    names = ("spk_sim_fit_landmarks", "spk_sim_smooth")
    real = {n: getattr(lib, n) for n in names}
    calls = dict.fromkeys(names, 0)

    def counting(name):
        def f(*args):
            calls[name] += 1
            return real[name](*args)
        return f

    for n in names:
        monkeypatch.setattr(lib, n, counting(n))
    kw = dict(size=SIZE, channel_order="bgr", noises=c["noises"])
    for paste in (dict(), dict(paste=True, feather=4)):
        want = irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], align=rows, chunk=2, **kw, **paste)
        assert calls == {"spk_sim_fit_landmarks": 0, "spk_sim_smooth": 0}
        for chunk in (1, 2):
            la = ops.LandmarkAlign(c["lm"], TEMPLATE5, smooth=1)
            got = irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], align=la, chunk=chunk, **kw, **paste)
            assert calls == {"spk_sim_fit_landmarks": 1, "spk_sim_smooth": 1}, calls
            calls.update(dict.fromkeys(names, 0))
            assert got.shape == ((c["T"], 64, 80, 3) if paste else (c["T"], 256, 256, 3)) and torch.equal(got, want), (paste, chunk)
    # smooth=0: the raw fit, one launch
    want = irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], align=raw, chunk=2, paste=True, feather=4, **kw)
    got = irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], align=ops.LandmarkAlign(c["lm"], TEMPLATE5), chunk=2, paste=True,
                             feather=4, **kw)
    assert calls == {"spk_sim_fit_landmarks": 1, "spk_sim_smooth": 0}, calls
    monkeypatch.undo()
    assert torch.equal(got, want) and not torch.equal(got, c["pose_u8"])
    assert not torch.equal(got, irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], align=rows, chunk=2, paste=True, feather=4, **kw))


def test_reenact_video_identity_align_is_its_hand_composition(irfd, pkg, clip, dev):
    c, ops = clip, pkg.ops
    rows = ops.similarity_from_landmarks(c["lm"], TEMPLATE5)
    pose, emo = (ops.frames_from_u8_aligned(c[k], SIZE, rows, channel_order="bgr") for k in ("pose_u8", "emo_u8"))
    kw = dict(size=SIZE, align=rows, channel_order="bgr", noises=c["noises"], chunk=2)
    run = lambda ident: irfd.reenact(ident, pose, emo, noises=c["noises"], chunk=2, output="uint8", channel_order="bgr")   # noqa: E731
    whole = run(ops.frames_from_u8(c["ident_u8"], SIZE, channel_order="bgr"))
    # None: today's call
    assert torch.equal(irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], identity_align=None, **kw), whole)
    assert torch.equal(irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], **kw), whole)
    # rows, from the host and from the device
    want = run(ops.frames_from_u8_aligned(c["ident_u8"], SIZE, c["rows1"], channel_order="bgr"))
    assert not torch.equal(want, whole)
    for form in (c["rows1"], c["rows1"].tolist(), c["rows1"].to(dev)):
        assert torch.equal(irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], identity_align=form, **kw), want)
    assert torch.equal(irfd.reenact_video(c["ident_u8"][None], c["pose_u8"], c["emo_u8"], identity_align=c["rows1"], **kw), want)
    # landmarks over one frame
    fitted = ops.similarity_from_landmarks(c["lm1"], TEMPLATE5)
    check(fitted, R.fit(c["lm1"].cpu().numpy(), TEMPLATE5), "the identity's row")
    want = run(ops.frames_from_u8_aligned(c["ident_u8"], SIZE, fitted, channel_order="bgr"))
    got = irfd.reenact_video(c["ident_u8"], c["pose_u8"], c["emo_u8"], identity_align=ops.LandmarkAlign(c["lm1"], TEMPLATE5), **kw)
    assert torch.equal(got, want) and not torch.equal(got, whole)
    # NV12 video frames: the identity is a packed photo there too
    surf = frames(34, c["T"], 96, 80).to(dev)
    ident = ops.frames_from_u8_aligned(c["ident_u8"], SIZE, c["rows1"], channel_order="bgr")
    want = irfd.reenact(ident, ops.frames_from_nv12(surf, SIZE), None, noises=c["noises"], chunk=2, output="nv12")
    got = irfd.reenact_video(c["ident_u8"], surf, size=SIZE, channel_order="bgr", noises=c["noises"], chunk=2, pixel_format="nv12",
                             identity_align=c["rows1"])
    assert torch.equal(got, want)
    assert not torch.equal(got, irfd.reenact_video(c["ident_u8"], surf, size=SIZE, channel_order="bgr", noises=c["noises"], chunk=2,
                                                   pixel_format="nv12"))
