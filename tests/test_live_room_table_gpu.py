"""GPU checks of ``LiveRoom.step`` over feeds in buffers of their own (speak-hack_amd/live.py over csrc/frame_table.hip): a list of
separately allocated frames of one size gives the bytes and the states of the step on their stack; feeds of three sizes -- one of
them a view with a pitch -- give, slot by slot, what a ``LiveSession`` gives on that feed alone; a tick makes today's library calls
with the three ``_table`` entry points in place of the strided three; and every refusal comes before a launch.  Model, template and
settings are those of tests/test_live_room_gpu.py; S = 3 feeds, T = 3 ticks, ``features`` on."""
import importlib

import numpy as np
import pytest
import torch

import blend_cases as BC
import landmark_ref as LR
from oracle import irfd_ref as IR
from oracle.weights_recipe import fill_state_dict

pytestmark = pytest.mark.gpu
SIZE, T, S = 128, 3, 3
TEMPLATE5 = [(44.0, 52.0), (84.0, 52.0), (64.0, 74.0), (48.0, 96.0), (80.0, 96.0)]
CONTOUR = [0, 1, 4, 3]
SEEDS = [7, 11, 2 ** 63 + 3]
TRACK, FEATS = dict(hold=2, beta=0.1), dict(hold=2, min_cutoff=2.0)
COMMON = dict(size=SIZE, template=TEMPLATE5, contour=CONTOUR, channel_order="bgr", track=TRACK, feather=4, colour_match=True, colour_decay=0.8,
              matte_softness=6.0, matte_grow=3.0)
# per feed: (buffer H, W, view offset y, x, frame H, W); feed 1 is a view with pitch 180 of a 44 x 60 surface
LAYOUT = [(48, 64, 0, 0, 48, 64), (44, 60, 2, 4, 40, 52), (56, 72, 0, 0, 56, 72)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


@pytest.fixture(scope="module")
def irfd(dev):
    import model
    m = model.IRFD()
    sd = IR.irfd_recipe_state_dict()
    sd.update({"Gd." + k: v for k, v in fill_state_dict(m.Gd.state_dict(), prefix="Gd.").items()})
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("D.") for k in missing)
    return m.to(dev).eval()


def tracked(pkg, rng, h, w):
    """T landmark sets [T,5,2] of a face that drifts over an h x w frame, in that frame's coordinates"""
    true = pkg.ops.similarity_rows([(0.48 * h + 0.7 * t, 0.51 * w - 0.5 * t) for t in range(T)], [0.7 * h + 1.5 * t for t in range(T)],
                                   [0.2 - 0.07 * t for t in range(T)], SIZE)
    return torch.from_numpy((LR.apply(true.numpy(), TEMPLATE5) + rng.standard_normal((T, 5, 2)) / 3).astype(np.float32))


@pytest.fixture(scope="module")
def feeds(pkg, dev):
    """Three identity photos; same-size feeds (48 x 64) and mixed-size feeds (LAYOUT), T frames each, with their landmarks [T,S,5,2];
    feed 1 loses a whole frame in tick 1"""
    rng = np.random.default_rng(29)
    photos = [BC.frames(31, 56, 72, 3).to(dev), BC.frames(41, 40, 52, 3).to(dev), BC.frames(42, 1, 64, 48, 3).to(dev)]
    same = BC.frames(33, T, S, 48, 64, 3).to(dev)
    same_lm = torch.stack([tracked(pkg, rng, 48, 64) for _ in range(S)], 1).to(dev)
    mixed = [BC.frames(50 + s, T, bh, bw, 3).to(dev) for s, (bh, bw, *_) in enumerate(LAYOUT)]          # whole surfaces, per feed [T,bh,bw,3]
    mixed_lm = torch.stack([tracked(pkg, rng, h, w) for *_, h, w in LAYOUT], 1).to(dev)
    same_lm[1, 1] = float("nan")
    mixed_lm[1, 1] = float("nan")
    return dict(photos=photos, same=same, same_lm=same_lm, mixed=mixed, mixed_lm=mixed_lm)


def states(room):
    return [t.clone() for t in (room.lm_state, room.feature_state, room.colour_state, room.frames)]


def same_states(a, b):
    return len(a) == len(b) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))


def view(surface, s):
    _, _, y0, x0, h, w = LAYOUT[s]
    return surface[y0:y0 + h, x0:x0 + w]


@pytest.mark.parametrize("inplace", [False, True], ids=["cloned", "in place"])
def test_a_list_of_one_size_is_the_stack(irfd, feeds, inplace):
    c = feeds
    stacked = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **COMMON)
    listed = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **COMMON)
    for t in range(T):
        frames = [c["same"][t, s].clone() for s in range(S)]               # three allocations
        keep = [f.clone() for f in frames]
        want = stacked.step(torch.stack(frames), c["same_lm"][t], inplace=inplace)
        got = listed.step(frames, c["same_lm"][t], inplace=inplace)
        assert isinstance(got, list) and len(got) == S and torch.equal(torch.stack(got), want), t
        assert same_states(states(listed), states(stacked)), t
        if inplace:
            assert got is frames and all(a is b for a, b in zip(got, frames))
        else:
            assert all(a is not b and torch.equal(b, k) for a, b, k in zip(got, frames, keep))      # new tensors, the caller's untouched
        assert not torch.equal(want, torch.stack(keep))
    assert listed.frames.tolist() == [T] * S


def test_feeds_of_three_sizes_are_three_sessions(irfd, feeds):
    c = feeds
    room = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **COMMON)
    sessions = [irfd.live(c["photos"][s], features=FEATS, seed=SEEDS[s], **COMMON) for s in range(S)]
    for t in range(T):
        surfaces = [c["mixed"][s][t].clone() for s in range(S)]
        before = [f.clone() for f in surfaces]
        frames = [view(surfaces[s], s) for s in range(S)]
        assert frames[1].stride(0) == 180 and not frames[1].is_contiguous()
        got = room.step(frames, c["mixed_lm"][t], inplace=True)
        assert got is frames
        for s in range(S):
            own = view(before[s], s).unsqueeze(0).contiguous()
            want = sessions[s].step(own, c["mixed_lm"][t, s:s + 1])[0]
            K = room.K
            assert torch.equal(frames[s], want), (t, s)                      # to the byte
            assert torch.equal(room.lm_state.view(S, K, 6)[s], sessions[s].lm_state.view(K, 6)), (t, s)
            assert torch.equal(room.colour_state[s], sessions[s].colour_state), (t, s)
            assert not torch.equal(frames[s], view(before[s], s)), (t, s)   # pasted in every tick: the lost frame of feed 1 is held
            rest = surfaces[s].clone()                                      # the padding of the surface is untouched
            view(rest, s).copy_(view(before[s], s))
            assert torch.equal(rest, before[s]), (t, s)
    assert room.frames.tolist() == [T] * S and [x.frames for x in sessions] == [T] * S


def test_a_tick_makes_todays_calls_with_the_table_entry_points(irfd, pkg, feeds, monkeypatch):
    c, lib = feeds, pkg._lib.lib()
    strided = ("spk_frames_paste_u8_sim_blend", "spk_frames_paste_u8_sim", "spk_paste_colour_sums_sim", "spk_paste_colour_match_sim",
               "spk_frames_u8_to_f32_sim")
    names = ("spk_launch_list", "spk_causal_filter", "spk_sim_fit_landmarks", "spk_matte_from_landmarks", "spk_colour_rows_causal",
             "spk_colour_rows_causal_feeds", "spk_noise_fill", "spk_noise_fill_rows", "spk_sim_smooth", "spk_colour_rows_window", "spk_conv2d_fwd",
             "spk_frames_u8_to_f32_sim_table", "spk_frames_paste_u8_sim_table", "spk_paste_colour_sums_sim_table",
             "spk_paste_colour_match_sim_table") + strided

    def counted(run):
        real = {n: getattr(lib, n) for n in names}
        calls = dict.fromkeys(names, 0)

        def counting(n):
            def f(*a):
                calls[n] += 1
                return real[n](*a)
            return f

        for n in names:
            monkeypatch.setattr(lib, n, counting(n))
        out = run()
        monkeypatch.undo()
        return out, {n: k for n, k in calls.items() if k}

    kw = dict(COMMON, seed=7)
    per_step = {"spk_launch_list": 3, "spk_causal_filter": 1, "spk_sim_fit_landmarks": 1, "spk_frames_u8_to_f32_sim_table": 1,
                "spk_matte_from_landmarks": 1, "spk_paste_colour_sums_sim_table": 1, "spk_colour_rows_causal_feeds": 1,
                "spk_frames_paste_u8_sim_table": 1}
    assert not set(per_step) & set(strided)

    def tick(t, n_feeds):
        return [view(c["mixed"][s][t].clone(), s) for s in range(n_feeds)]

    for n_feeds in (1, S):
        photos = c["photos"][:n_feeds]
        room = irfd.live_room(photos, **kw)
        room.step(tick(0, n_feeds), c["mixed_lm"][0, :n_feeds], inplace=True)      # the plans of this batch exist from here on
        for t in (1, 2):
            _, calls = counted(lambda: room.step(tick(t, n_feeds), c["mixed_lm"][t, :n_feeds], inplace=True))
            assert calls == per_step, (n_feeds, calls)
        both = irfd.live_room(photos, features={}, **kw)
        both.step(tick(0, n_feeds), c["mixed_lm"][0, :n_feeds], inplace=True)
        _, calls = counted(lambda: both.step(tick(1, n_feeds), c["mixed_lm"][1, :n_feeds], emotion_u8=tick(2, n_feeds), inplace=True))
        assert calls == dict(per_step, spk_causal_filter=2, spk_frames_u8_to_f32_sim_table=2), (n_feeds, calls)


def test_refusals_leave_the_room_as_it_was(irfd, pkg, feeds, dev):
    c, L = feeds, pkg._lib
    room = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **COMMON)
    lm = c["mixed_lm"][0]
    surfaces = [c["mixed"][s][0].clone() for s in range(S)]
    frames = [view(surfaces[s], s) for s in range(S)]
    room.step(frames, lm, inplace=True)                                     # a room in mid-call: its states are not empty
    surfaces = [c["mixed"][s][1].clone() for s in range(S)]
    frames = [view(surfaces[s], s) for s in range(S)]
    before, was = [f.clone() for f in surfaces], states(room)
    assert all(bool(t.any()) for t in was)
    wide = torch.zeros(40, 104, 3, dtype=torch.uint8, device=dev)
    refused = [(ValueError, dict(frames_u8=frames[:2])),                                        # wrong list length
               (ValueError, dict(frames_u8=frames + frames[:1])),
               (ValueError, dict(frames_u8=[frames[0], None, frames[2]])),                      # a None element
               (ValueError, dict(frames_u8=[frames[0], frames[1].float(), frames[2]])),         # wrong dtype
               (L.SpkError, dict(frames_u8=[frames[0], frames[1].cpu(), frames[2]])),           # wrong device
               (ValueError, dict(frames_u8=[frames[0], wide[:, ::2], frames[2]])),              # pixels that are not packed
               (ValueError, dict(frames_u8=frames, emotion_u8=[frames[0], frames[2], frames[1]])),          # sizes differ feed by feed
               (ValueError, dict(frames_u8=frames, emotion_u8=frames[:2])),
               (L.SpkError, dict(frames_u8=[frames[0], frames[1], frames[1][4:30, 3:40]], inplace=True)),   # two elements in one buffer
               (L.SpkError, dict(frames_u8=[frames[0], frames[0], frames[2]], inplace=True))]
    for n, (error, kw) in enumerate(refused):
        with pytest.raises(error):
            room.step(landmarks=lm, **kw)
        assert same_states(states(room), was), n
    assert all(torch.equal(a, b) for a, b in zip(surfaces, before))
    # what was refused in place is fine where every frame is cloned first, and the room goes on
    out = room.step([frames[0], frames[0], frames[2]], lm)
    assert len(out) == S and out[0] is not out[1] and all(torch.equal(a, b) for a, b in zip(surfaces, before))
    assert not same_states(states(room), was)
