"""CPU checks of the causal filters: the numpy model of tests/causal_ref.py against the properties include/spk.h states (split
invariance, hold and expiry, what the filter is for: less jitter on a still point, little lag after a jump), and every host refusal of
``ops.causal_filter`` / ``ops.causal_filter_state`` / ``ops.colour_rows_causal`` / ``IRFD.live`` / ``LiveSession.step``, which come
before a device is touched."""
import importlib

import numpy as np
import pytest
import torch

import causal_ref as CR
import colour_window_ref as CW

TEMPLATE5 = [(44.0, 52.0), (84.0, 52.0), (64.0, 74.0), (48.0, 96.0), (80.0, 96.0)]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("speak-hack_amd")


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["landmarks", "features", "triples"])
def test_model_is_split_invariant(name):
    x, w, group = CR.series(name)
    kw = dict(group=group, hold=2)
    results = []
    for split in ([9], [4, 5], [1] * 9):
        state, ys, wys, n0 = CR.empty_state(x.shape[1], group), [], [], 0
        for n in split:
            y, wy = CR.causal_filter(x[n0:n0 + n], state, None if w is None else w[n0:n0 + n], **kw)
            ys.append(y), wys.append(wy)
            n0 += n
        results.append((np.concatenate(ys), np.concatenate(wys), state))
    for y, wy, state in results[1:]:
        assert CR.same(y, results[0][0]) and CR.same(wy, results[0][1]) and CR.same(state, results[0][2])
    assert np.isnan(results[0][0]).any() and np.isfinite(results[0][0]).any()


def test_model_colour_rows_are_split_invariant_and_keep_the_row_of_a_frame_without_statistics():
    sums = np.array(CW.window_clip("holes"))                                # frame 2: NaN S0, frame 3: zeros, frame 5: a NaN Sq
    whole_state = np.zeros(13)
    whole = CR.colour_rows_causal(sums, whole_state, 0.8)
    assert whole["part"].tolist() == [True, True, False, False, True, False, True]
    for split in ([3, 4], [1] * 7):
        state, rows, n0 = np.zeros(13), [], 0
        for n in split:
            rows.append(CR.colour_rows_causal(sums[n0:n0 + n], state, 0.8)["rows"])
            n0 += n
        assert CR.same(np.concatenate(rows), whole["rows"]) and CR.same(state, whole_state)
    for n in (2, 3, 5):
        assert CR.same(whole["rows"][n], whole["rows"][n - 1])
    # decay = 0: the frame's own sums, i.e. the window model at radius 0 on the frames that take part
    per_frame = CW.window_rows(sums, 0)["rows"]
    got = CR.colour_rows_causal(sums, np.zeros(13), 0.0)["rows"]
    for n in (0, 1, 4, 6):
        assert CR.same(got[n], per_frame[n])
    # nothing yet: (1, 0) by rule
    assert CR.colour_rows_causal(sums[2:4], np.zeros(13), 0.5)["rows"].tolist() == [[[1.0, 0.0]] * 3] * 2


def test_hold_and_expiry():
    rate, hold = 30.0, 2
    kw = dict(group=1, rate=rate, hold=hold)
    nan = np.nan
    # a 2-frame gap: bridged with the held value, and the recursion goes on with Te = 3 / rate
    x = np.array([[1.0], [2.0], [nan], [nan], [5.0]])
    state = CR.empty_state(1, 1)
    y, wy = CR.causal_filter(x, state, np.array([[0.5], [0.7], [0.9], [0.9], [0.3]]), **kw)
    assert y[0, 0] == 1.0 and y[2, 0] == y[1, 0] and y[3, 0] == y[1, 0] and 1.0 < y[1, 0] < 2.0
    assert wy[:, 0].tolist() == [0.5, 0.7, 0.7, 0.7, 0.3]                  # held: the weight it last had
    Te = 3.0 / rate
    xh, dh = y[1, 0], CR.alpha(1.0, 1.0 / rate) * ((2.0 - 1.0) / (1.0 / rate))
    dh3 = CR.alpha(1.0, Te) * ((5.0 - xh) / Te) + (1.0 - CR.alpha(1.0, Te)) * dh
    a = CR.alpha(1.0 + 0.05 * abs(dh3), Te)
    assert y[4, 0] == a * 5.0 + (1.0 - a) * xh
    assert state[0].tolist() == [1.0, 0.3, y[4, 0], dh3]
    # a 4-frame gap: held, held, NaN, NaN, then the sample itself
    x = np.array([[1.0], [2.0], [nan], [nan], [nan], [nan], [7.0], [8.0]])
    state = CR.empty_state(1, 1)
    y, wy = CR.causal_filter(x, state, **kw)
    assert y[2, 0] == y[1, 0] and y[3, 0] == y[1, 0] and np.isnan(y[4:6, 0]).all() and y[6, 0] == 7.0 and 7.0 < y[7, 0] < 8.0
    assert wy[:, 0].tolist() == [1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0]
    # exactly hold + 1 frames: the estimate has expired, and the sample restarts it (k - 1 = 3 > hold)
    y, _ = CR.causal_filter(np.array([[1.0], [nan], [nan], [nan], [9.0]]), CR.empty_state(1, 1), **kw)
    assert np.isnan(y[3, 0]) and y[4, 0] == 9.0
    # never valid: NaN throughout, k = 0
    state = CR.empty_state(2, 2)
    y, wy = CR.causal_filter(np.array([[1.0, nan]] * 4), state, **dict(kw, group=2))
    assert np.isnan(y).all() and (wy == 0).all() and (state == 0).all()
    y, wy = CR.causal_filter(np.ones((3, 1)), state[:1, :4].copy(), np.array([0.0]), **kw)                  # a zero weight
    assert np.isnan(y).all() and (wy == 0).all()
    # hold = 0: nothing is bridged
    y, _ = CR.causal_filter(np.array([[1.0], [nan], [3.0]]), CR.empty_state(1, 1), group=1, hold=0)
    assert np.isnan(y[1, 0]) and y[2, 0] == 3.0


def test_a_still_point_is_steadied_and_a_jump_is_followed():
    x = CR.still_point()                                                    # 200 frames, N(0, 0.5) noise, 30 fps, the defaults
    y, _ = CR.causal_filter(x, CR.empty_state(2, 2))
    ratio = x.astype(np.float64).std(0) / y.std(0)
    print(f"still point: the standard deviation falls by {ratio[0]:.2f}x / {ratio[1]:.2f}x")
    assert (ratio > 2.0).all()
    jump = np.concatenate([np.zeros((30, 2)), np.tile(np.array([[40.0, 0.0]]), (6, 1))])
    y, _ = CR.causal_filter(jump, CR.empty_state(2, 2))
    lag = 40.0 - y[30:, 0]
    print(f"40-pixel jump: lag {lag.round(3).tolist()}")
    assert lag[2] < 1.0 and (np.diff(lag) <= 0).all() and (lag >= 0).all()


# ---- the host refusals -------------------------------------------------------------------------------------------------------------------
def test_launchers_refuse_on_the_host(pkg):
    ops = pkg.ops
    x, state = torch.zeros(3, 5, 2), torch.zeros(5, 6, dtype=torch.float64)
    for kw, match in ((dict(group=0), "group"), (dict(group=5), "group"), (dict(group=True), "group"), (dict(group=2.0), "group"),
                      (dict(group=3), "does not divide"), (dict(group=4), "does not divide"),
                      (dict(rate=0.0), "rate"), (dict(rate=-30.0), "rate"), (dict(rate=float("nan")), "rate"), (dict(rate=float("inf")), "rate"),
                      (dict(min_cutoff=0.0), "min_cutoff"), (dict(d_cutoff=float("nan")), "d_cutoff"), (dict(beta=-0.1), "beta"),
                      (dict(beta=float("inf")), "beta"), (dict(hold=-1), "hold"), (dict(hold=1.5), "hold"), (dict(hold=True), "hold"),
                      (dict(weights=[1.0] * 4), "weights"), (dict(weights="no"), "weights"), (dict(out=torch.zeros(3, 10)), "out")):
        with pytest.raises(ValueError, match=match):
            ops.causal_filter(x, state, **kw)
    for bad in (torch.zeros(5, 5, dtype=torch.float64), torch.zeros(5, 6), torch.zeros(6, 5, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="state"):
            ops.causal_filter(x, bad)
    for bad in (torch.zeros(10), torch.zeros(0, 5, 2), [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="x must be"):
            ops.causal_filter(bad, state)
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):          # the arguments are in order: what is left is the device
        ops.causal_filter(x, state)
    for D, group in ((10, 0), (10, 5), (10, 3), (0, 1), (-2, 2), (2.0, 2)):
        with pytest.raises(ValueError):
            ops.causal_filter_state(D, group, "cuda")
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        ops.causal_filter_state(10, 2, "cpu")
    sums, P = torch.zeros(4, 13, dtype=torch.float64), torch.zeros(13, dtype=torch.float64)
    for decay in (-0.01, 1.01, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="decay"):
            ops.colour_rows_causal(sums, P, decay)
    for kw, match in ((dict(max_gain=0.5), "max_gain"), (dict(min_sigma=-1.0), "min_sigma"), (dict(min_weight=float("nan")), "min_weight")):
        with pytest.raises(ValueError, match=match):
            ops.colour_rows_causal(sums, P, 0.9, **kw)
    for bad in (torch.zeros(4, 13), torch.zeros(4, 12, dtype=torch.float64), torch.zeros(0, 13, dtype=torch.float64), torch.zeros(13, dtype=torch.float64)):
        with pytest.raises(ValueError, match="sums"):
            ops.colour_rows_causal(bad, P, 0.9)
    for bad in (torch.zeros(13), torch.zeros(1, 13, dtype=torch.float64), torch.zeros(12, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="state"):
            ops.colour_rows_causal(sums, bad, 0.9)
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        ops.colour_rows_causal(sums, P, 0.9)


def test_live_refuses_on_the_host(pkg, monkeypatch):
    import model
    m = model.IRFD()
    ident = torch.zeros(48, 64, 3, dtype=torch.uint8)
    good = dict(template=TEMPLATE5, size=128)
    for kw, match in ((dict(template=None), "template"), (dict(template=None, contour=[0, 1, 4, 3]), "contour= takes its fallback"),
                      (dict(template=[(1.0, 2.0)]), "template"), (dict(template=[(1.0, 2.0)] * 3), "distinct"), (dict(template=7), "template"),
                      (dict(contour=[0, 1, 5]), "contour"), (dict(contour=[0, 1]), "contour"),
                      (dict(rate=0.0), "rate"), (dict(rate=float("nan")), "rate"),
                      (dict(track=dict(hold=-1)), "hold"), (dict(track=dict(min_cutoff=0.0)), "min_cutoff"), (dict(track=dict(radius=3)), "track"),
                      (dict(track=3), "track"), (dict(features=dict(beta=-1.0)), "beta"), (dict(features=True), "features"),
                      (dict(feather=-1.0), "feather"), (dict(matte_softness=0.0), "matte_softness"), (dict(matte_grow=float("inf")), "matte_grow"),
                      (dict(colour_match=1), "colour_match"), (dict(colour_decay=1.5), "colour_decay"), (dict(colour_decay=float("nan")), "colour_decay"),
                      (dict(noise="fixed"), "needs a seed"), (dict(noise="pink"), "noise"), (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"),
                      (dict(channel_order="gbr"), "channel_order"), (dict(offset=float("nan")), "offset"), (dict(size=0), "size"),
                      (dict(identity_align=[[0.0, 0.0, 1.0, 1.0]]), "identity_align")):
        with pytest.raises(ValueError, match=match):
            m.live(ident, **dict(good, **kw))
    with pytest.raises(ValueError, match="identity_u8"):
        m.live(torch.zeros(2, 48, 64, 3, dtype=torch.uint8), **good)
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):          # the arguments are in order: what is left is the device
        m.live(ident, contour=[0, 1, 4, 3], colour_match=True, seed=3, **good)

    # a session without a device, to reach ``step``'s own checks: Ei and the crop of the photo stand in as functions that return
    # CPU tensors; nothing of ``step`` may run before its arguments are in order
    monkeypatch.setattr(pkg.frames, "frames_from_u8", lambda u8, size, **kw: torch.zeros(1, 3, 128, 128))
    monkeypatch.setattr(model.IRFD, "encode", lambda self, images, which: torch.zeros(images.size(0), 2048, 1, 1))
    monkeypatch.setattr(pkg.frames, "causal_filter_state", lambda D, group, device: torch.zeros(D // group, 2 + 2 * group, dtype=torch.float64))
    s = m.live(ident, contour=[0, 1, 4, 3], features={}, colour_match=True, seed=3, **good)
    assert s.frames == 0 and tuple(s.fi.shape) == (1, 2048, 1, 1) and tuple(s.lm_state.shape) == (5, 6) and tuple(s.feature_state.shape) == (4096, 4)
    assert s.track == dict(group=2, rate=30.0, min_cutoff=1.0, beta=0.05, d_cutoff=1.0, hold=5) and s.features["group"] == 1
    video, lm = torch.zeros(3, 48, 64, 3, dtype=torch.uint8), torch.zeros(3, 5, 2)
    for args, kw, match in (((video[0], lm), {}, "frames must be"), ((video, torch.zeros(3, 6, 2)), {}, "5 points per frame as the template has"),
                            ((video, torch.zeros(2, 5, 2)), {}, "landmarks must be"), ((video, lm), dict(emotion_u8=video[:2]), "emotion_u8"),
                            ((video, lm), dict(inplace=1), "inplace"), ((video, lm), dict(weights=[1.0] * 4), "weights"),
                            ((video, lm), dict(weights=torch.zeros(3, 4)), "weights")):
        with pytest.raises(ValueError, match=match):
            s.step(*args, **kw)
    raw = m.live(ident, track=None, **good)                                 # without the filter the fit's own check of the weights
    with pytest.raises(ValueError, match="weights"):
        raw.step(video, lm, weights=[1.0] * 4)
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        s.step(video, lm)
    assert s.frames == 0
    s.frames = 4
    s.lm_state += 1.0
    s.reset()
    assert s.frames == 0 and not s.lm_state.any() and tuple(s.fi.shape) == (1, 2048, 1, 1)
