"""CPU checks of the live room (speak-hack_amd/live.py: ``LiveRoom``; ``ops.noise_fill_rows``, ``ops.colour_rows_causal_feeds``): the
numpy model of the feeds' colour rows (tests/live_room_ref.py) is the single-feed model of tests/causal_ref.py column by column,
and the host checks of the two launchers, of ``IRFD.live_room`` and of the room's methods raise ``ValueError`` before a device is
touched."""
import importlib

import numpy as np
import pytest
import torch

import causal_ref as CR
import live_room_ref as RR

TEMPLATE5 = [(44.0, 52.0), (84.0, 52.0), (64.0, 74.0), (48.0, 96.0), (80.0, 96.0)]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("speak-hack_amd")


@pytest.mark.parametrize("S", [1, 4, 22])
def test_feeds_model_is_the_single_feed_model_column_by_column(S):
    sums = RR.spoil(RR.synthetic_sums(S))
    assert sums.shape == (RR.N, S, 13)
    for decay in RR.DECAYS:
        state = np.zeros((S, 13))
        got = RR.colour_rows_feeds(sums, state, decay)
        assert np.array_equal(got["part"], RR.takes_part(S)) and not got["part"].all()
        for s in range(S):
            one_state = np.zeros(13)
            one = CR.colour_rows_causal(sums[:, s], one_state, decay)
            assert CR.same(got["rows"][:, s], one["rows"]) and CR.same(got["P"][:, s], one["P"]) and CR.same(state[s], one_state), (decay, s)
            assert np.array_equal(got["part"][:, s], one["part"])
        # any split of the frames: the same numbers
        state2, parts = np.zeros((S, 13)), []
        for n0, n1 in ((0, 3), (3, 7)):
            parts.append(RR.colour_rows_feeds(sums[n0:n1], state2, decay)["rows"])
        assert CR.same(np.concatenate(parts), got["rows"]) and CR.same(state2, state)
    low, nan, clean = RR.pattern(S)
    rows = RR.colour_rows_feeds(sums, np.zeros((S, 13)), 0.8)["rows"]
    assert CR.same(rows[2, low], rows[1, low]) and CR.same(rows[5, nan], rows[4, nan])      # a rejected frame repeats the previous row
    assert not CR.same(rows[2, clean], rows[1, clean]) or S == 1


def test_noise_rows_model_is_the_stepped_model_row_by_row():
    import philox_ref as PR
    hw, seeds, frames = (16, 6), (7, 7, 2 ** 63 + 3), (0, 5, 2 ** 32 + 1)
    rows = RR.noise_rows(seeds, frames, hw)
    for b, (s, f) in enumerate(zip(seeds, frames)):
        for l, plane in enumerate(PR.noise_layers(s, f, hw, 1)):
            assert np.array_equal(rows[l][b], plane[0])
    same = RR.noise_rows((9, 9, 9), (4, 5, 6), hw)
    assert all(np.array_equal(a, b) for a, b in zip(same, PR.noise_layers(9, 4, hw, 3)))


def test_launchers_refuse_on_the_host(pkg):
    ops = pkg.ops
    sums, P = torch.zeros(7, 4, 13, dtype=torch.float64), torch.zeros(4, 13, dtype=torch.float64)
    for decay in (-0.01, 1.01, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="decay"):
            ops.colour_rows_causal_feeds(sums, P, decay)
    for kw, match in ((dict(max_gain=0.5), "max_gain"), (dict(min_sigma=-1.0), "min_sigma"), (dict(min_weight=float("nan")), "min_weight")):
        with pytest.raises(ValueError, match=match):
            ops.colour_rows_causal_feeds(sums, P, 0.9, **kw)
    for bad in (torch.zeros(7, 4, 13), torch.zeros(7, 4, 12, dtype=torch.float64), torch.zeros(0, 4, 13, dtype=torch.float64),
                torch.zeros(7, 0, 13, dtype=torch.float64), torch.zeros(7, 13, dtype=torch.float64), None):                      # bad S among them
        with pytest.raises(ValueError, match="sums"):
            ops.colour_rows_causal_feeds(bad, P, 0.9)
    for bad in (torch.zeros(4, 13), torch.zeros(3, 13, dtype=torch.float64), torch.zeros(5, 13, dtype=torch.float64),
                torch.zeros(13, dtype=torch.float64), torch.zeros(4, 12, dtype=torch.float64), None):                            # [N,S,13] against [S',13]
        with pytest.raises(ValueError, match="state"):
            ops.colour_rows_causal_feeds(sums, bad, 0.9)
    with pytest.raises(ValueError, match="out"):
        ops.colour_rows_causal_feeds(sums, P, 0.9, out=torch.zeros(7, 3, 3, 2))
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):          # the arguments are in order: what is left is the device
        ops.colour_rows_causal_feeds(sums, P, 0.9)
    # the rows noise: the tables
    dst, seeds, frames = torch.zeros(3 * 80), torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    for s, f, match in ((seeds[:2], frames, "seed_rows"), (seeds, frames[:2], "frame_rows"), (seeds.to(torch.int32), frames, "seed_rows"),
                        (seeds, frames.double(), "frame_rows"), ([7, 7, 7], frames, "seed_rows"), (seeds, None, "frame_rows"),
                        (seeds.view(3, 1), frames, "seed_rows")):
        with pytest.raises(ValueError, match=match):
            ops.noise_fill_rows(dst, (16, 64), 3, s, f)
        with pytest.raises(ValueError, match=match):
            ops.decoder_noise_rows([(3, 1, 4, 4), (3, 1, 8, 8)], s, f)
    with pytest.raises(ValueError, match="shapes"):
        ops.decoder_noise_rows([(3, 1, 4, 4), (2, 1, 8, 8)], seeds, frames)
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        ops.noise_fill_rows(dst, (16, 64), 3, seeds, frames)
    for bad in ([], 7, [7, -1], [7, 2 ** 64], [7, 1.5], [True]):
        with pytest.raises(ValueError, match="seed"):
            ops.seed_rows(bad)
    assert ops.seed_rows([7, 2 ** 63 + 3, 2 ** 64 - 1]).tolist() == [7, -2 ** 63 + 3, -1]      # the 64-bit patterns


def test_live_room_refuses_on_the_host(pkg, monkeypatch):
    import model
    m = model.IRFD()
    photos = [torch.zeros(48, 64, 3, dtype=torch.uint8), torch.zeros(1, 30, 40, 3, dtype=torch.uint8), torch.zeros(56, 72, 3, dtype=torch.uint8)]
    good = dict(template=TEMPLATE5, size=128)
    for kw, match in ((dict(template=None), "template"), (dict(contour=[0, 1, 5]), "contour"), (dict(rate=0.0), "rate"),
                      (dict(track=dict(hold=-1)), "hold"), (dict(features=True), "features"), (dict(colour_match=1), "colour_match"),
                      (dict(colour_decay=1.5), "colour_decay"), (dict(colour_decay=-0.1), "colour_decay"), (dict(colour_decay=float("nan")), "colour_decay"),
                      (dict(noise="fixed"), "needs a seed"), (dict(noise="pink"), "noise"), (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"),
                      (dict(seed=[1, 2]), "one per feed"), (dict(seed=[1, 2, 3, 4]), "one per feed"), (dict(seed=[1, 2, -3]), "seed"),
                      (dict(seed=[1, None, 3]), "seed"), (dict(seed=1.5), "seed"),
                      (dict(identity_align=[None, None]), "identity_align"), (dict(identity_align=[None, [[0.0, 0.0, 1.0, 1.0]], None]), "identity_align"),
                      (dict(identity_align=3), "identity_align"), (dict(size=0), "size")):
        with pytest.raises(ValueError, match=match):
            m.live_room(photos, **dict(good, **kw))
    for bad, match in (([], "at least one feed"), (torch.zeros(0, 48, 64, 3, dtype=torch.uint8), "at least one feed"),
                       (torch.zeros(48, 64, 3, dtype=torch.uint8), "identities_u8"), (7, "identities_u8"),
                       ([photos[0], torch.zeros(2, 48, 64, 3, dtype=torch.uint8)], r"identities_u8\[1\]"), ([photos[0], None], r"identities_u8\[1\]")):
        with pytest.raises(ValueError, match=match):                        # bad S among them
            m.live_room(bad, **good)
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):          # the arguments are in order: what is left is the device
        m.live_room(photos, contour=[0, 1, 4, 3], colour_match=True, seed=[3, 4, 2 ** 63 + 5], **good)

    # a room without a device, to reach the checks of its methods: Ei and the crop of a photo stand in as functions that return CPU
    # tensors; nothing of ``step`` may run before its arguments are in order
    monkeypatch.setattr(pkg.frames, "frames_from_u8", lambda u8, size, **kw: torch.zeros(1, 3, 128, 128))
    monkeypatch.setattr(model.IRFD, "encode", lambda self, images, which: torch.full((images.size(0), 2048, 1, 1), 1.0))
    monkeypatch.setattr(pkg.frames, "causal_filter_state", lambda D, group, device: torch.zeros(D // group, 2 + 2 * group, dtype=torch.float64))
    room = m.live_room(photos, contour=[0, 1, 4, 3], features={}, colour_match=True, seed=[3, 4, 2 ** 63 + 5], **good)
    assert room.S == 3 and tuple(room.fi.shape) == (3, 2048, 1, 1) and tuple(room.lm_state.shape) == (15, 6)
    assert tuple(room.feature_state.shape) == (3 * 4096, 4) and tuple(room.colour_state.shape) == (3, 13)
    assert room.frames.dtype == torch.int64 and room.frames.tolist() == [0, 0, 0] and room.seeds.tolist() == [3, 4, -2 ** 63 + 5]
    assert m.live_room(torch.zeros(2, 48, 64, 3, dtype=torch.uint8), seed=9, **good).seeds.tolist() == [9, 9]
    assert m.live_room(photos[:1], **good).seeds is None
    tick, lm = torch.zeros(3, 48, 64, 3, dtype=torch.uint8), torch.zeros(3, 5, 2)
    for args, kw, match in (((tick[0], lm), {}, "frames must be"), ((tick[:2], lm[:2]), {}, "one frame per feed"),
                            ((tick, torch.zeros(3, 6, 2)), {}, "5 points per feed as the template has"),       # landmarks [S,K',2]
                            ((tick, torch.zeros(2, 5, 2)), {}, "landmarks must be"), ((tick, lm), dict(emotion_u8=tick[:2]), "emotion_u8"),
                            ((tick, lm), dict(inplace=1), "inplace"), ((tick, lm), dict(weights=[1.0] * 4), "weights"),
                            ((tick, lm), dict(weights=torch.zeros(3, 4)), "weights"), ((tick, lm), dict(weights=torch.zeros(2, 5)), "weights"),
                            ((tick, lm), dict(weights=[[1.0] * 5] * 4), "weights"), ((tick, lm), dict(weights="no"), "weights")):
        with pytest.raises(ValueError, match=match):
            room.step(*args, **kw)
    raw = m.live_room(photos, track=None, **good)                           # the same checks without the filter
    with pytest.raises(ValueError, match="weights"):
        raw.step(tick, lm, weights=[1.0] * 4)
    for kw in ({}, dict(weights=[1.0] * 5), dict(weights=torch.ones(3, 5))):
        with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
            room.step(tick, lm, **kw)
    assert room.frames.tolist() == [0, 0, 0]
    for slot in (-1, 3, 1.0, True, "0"):                                   # slot out of range
        with pytest.raises(ValueError, match="slot"):
            room.reset(slot)
        with pytest.raises(ValueError, match="slot"):
            room.set_identity(slot, photos[0])
    with pytest.raises(ValueError, match="identity_u8"):
        room.set_identity(1, torch.zeros(2, 48, 64, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="identity_align"):
        room.set_identity(1, photos[0], identity_align=[[0.0, 0.0, 1.0, 1.0]])

    # reset and set_identity touch their slot alone
    def dirty():
        room.frames += torch.tensor([4, 5, 6])
        for t in (room.lm_state, room.feature_state, room.colour_state):
            t += 1.0

    dirty()
    room.reset(1)
    assert room.frames.tolist() == [4, 0, 6]
    for t in (room.lm_state, room.feature_state, room.colour_state):
        per_slot = t.view(3, -1)
        assert not per_slot[1].any() and (per_slot[0] == 1.0).all() and (per_slot[2] == 1.0).all()
    monkeypatch.setattr(model.IRFD, "encode", lambda self, images, which: torch.full((images.size(0), 2048, 1, 1), 2.0))
    room.set_identity(2, photos[1])
    assert room.frames.tolist() == [4, 0, 0] and (room.fi[2] == 2.0).all() and (room.fi[:2] == 1.0).all()
    assert not room.lm_state.view(3, -1)[2].any() and (room.lm_state.view(3, -1)[0] == 1.0).all()
    room.reset()
    assert room.frames.tolist() == [0, 0, 0] and not room.lm_state.any() and not room.feature_state.any() and not room.colour_state.any()
    assert (room.fi[2] == 2.0).all()
