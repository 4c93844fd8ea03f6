"""GPU checks of ``IRFD.live_room`` / ``LiveRoom`` (speak-hack_amd/live.py): a tick is the explicit composition of ``ops.*`` calls at
batch S; slot ``s`` is a ``LiveSession`` of its own -- its landmark state to the bit, its ``fi`` to the bit, its frames to the byte;
``reset`` and ``set_identity`` touch one slot; a step makes the same library calls whatever S is; and a room of one is a session.  The
model and clip are those of the live-session tests: recipe weights, 128 -> 256 pixels, T = 5 BGR frames of 48 x 64, five tracked
landmarks.  S = 3 feeds over T = 5 ticks: feed ``s`` shows frame ``(t + s) % T`` in tick ``t``; feed 1 loses a whole frame (tick 1), feed
2 one point for two ticks (3 and 4).

Slot against session compares frames made at batch 3 with frames made at batch 1: equal once quantised, as the session tests find
for the same clip and sizes in every split of it; the fp32 images before the quantisation are not compared."""
import importlib

import numpy as np
import pytest
import torch

import blend_cases as BC
import landmark_ref as LR
from oracle import irfd_ref as IR
from oracle.weights_recipe import fill_state_dict

pytestmark = pytest.mark.gpu
SIZE, R, T, S = 128, 256, 5, 3
TEMPLATE5 = [(44.0, 52.0), (84.0, 52.0), (64.0, 74.0), (48.0, 96.0), (80.0, 96.0)]
CONTOUR = [0, 1, 4, 3]
MATTE = dict(matte_softness=6.0, matte_grow=3.0)
SEEDS = [7, 11, 2 ** 63 + 3]
TRACK, FEATS = dict(hold=2, beta=0.1), dict(hold=2, min_cutoff=2.0)
COMMON = dict(size=SIZE, template=TEMPLATE5, contour=CONTOUR, channel_order="bgr", track=TRACK, feather=4, colour_match=True, colour_decay=0.8,
              **MATTE)


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


@pytest.fixture(scope="module")
def feeds(pkg, dev):
    """Three identity photos of three sizes; per tick and feed a frame [T,S,48,64,3] and its landmarks [T,S,5,2], with the drop-outs"""
    ops = pkg.ops
    rng = np.random.default_rng(23)
    true = ops.similarity_rows([(23.3 + 0.7 * t, 32.6 - 0.5 * t) for t in range(T)], [34.0 + 1.5 * t for t in range(T)],
                               [0.2 - 0.07 * t for t in range(T)], SIZE)
    lm = torch.from_numpy((LR.apply(true.numpy(), TEMPLATE5) + rng.standard_normal((T, 5, 2)) / 3).astype(np.float32)).to(dev)
    pose = BC.frames(32, T, 48, 64, 3).to(dev)
    show = torch.tensor([[(t + s) % T for s in range(S)] for t in range(T)], device=dev)
    frames, lms = pose[show].contiguous(), lm[show].clone()
    lms[1, 1] = float("nan")                                                # feed 1: the tracker lost the face for a tick (held)
    lms[3:5, 2, 3] = float("nan")                                           # feed 2: and one point for two ticks
    photos = [BC.frames(31, 56, 72, 3).to(dev), BC.frames(41, 40, 52, 3).to(dev), BC.frames(42, 1, 64, 48, 3).to(dev)]
    return dict(photos=photos, frames=frames, lm=lms)


def run_room(room, feeds, before=None):
    """All T ticks -> (frames [T,S,48,64,3], the landmark state after every tick [T,S,5,6]); ``before(t)`` runs ahead of tick t"""
    outs, states = [], []
    for t in range(T):
        if before is not None:
            before(t)
        outs.append(room.step(feeds["frames"][t], feeds["lm"][t]))
        states.append(room.lm_state.view(S, 5, 6).clone())
    return torch.stack(outs), torch.stack(states)


def run_session(session, feeds, s, ticks=range(T)):
    """Feed ``s`` through a session, one frame per step -> (frames [len(ticks),48,64,3], its landmark state after every step)"""
    outs, states = [], []
    for t in ticks:
        outs.append(session.step(feeds["frames"][t, s:s + 1], feeds["lm"][t, s:s + 1])[0])
        states.append(session.lm_state.clone())
    return torch.stack(outs), torch.stack(states)


@pytest.fixture(scope="module")
def base(irfd, feeds):
    """The room with the filters on (``features`` on), run once over the T ticks: what the other runs are compared with"""
    room = irfd.live_room(feeds["photos"], features=FEATS, seed=SEEDS, **COMMON)
    outs, states = run_room(room, feeds)
    assert outs.dtype == torch.uint8 and outs.shape == (T, S, 48, 64, 3) and room.frames.tolist() == [T] * S
    assert not torch.equal(outs, feeds["frames"])
    return dict(room=room, outs=outs, states=states)


def test_a_tick_is_the_composition_of_ops_at_batch_s(irfd, pkg, feeds, base, dev):
    ops, c = pkg.ops, feeds
    fi = torch.cat([irfd.encode(ops.frames_from_u8(p, SIZE, channel_order="bgr"), "Ei") for p in c["photos"]])
    assert torch.equal(fi, base["room"].fi)
    lm_state, f_state = ops.causal_filter_state(S * 10, 2, dev), ops.causal_filter_state(S * 4096, 1, dev)
    c_state = torch.zeros(S, 13, dtype=torch.float64, device=dev)
    seeds, counters = ops.seed_rows(SEEDS, dev), torch.zeros(S, dtype=torch.int64, device=dev)
    nan = torch.full((), float("nan"), device=dev)
    for t in range(T):
        frames = c["frames"][t]
        y_lm, wy = ops.causal_filter(c["lm"][t].reshape(1, S * 10), lm_state, **TRACK)
        y_lm, wy = y_lm.view(S, 5, 2), wy.view(S, 5)
        assert torch.isfinite(y_lm).all()                                   # every drop-out is bridged: hold = 2
        rows = ops.similarity_from_landmarks(y_lm, TEMPLATE5, weights=wy)
        pose = ops.frames_from_u8_aligned(frames, SIZE, rows, channel_order="bgr")
        f = torch.cat([irfd.encode(pose, "Ee").view(S, -1), irfd.encode(pose, "Ep").view(S, -1)], 1)
        f = torch.where(torch.isfinite(rows).all(1, keepdim=True), f, nan)
        ops.causal_filter(f.view(1, -1), f_state, group=1, out=f.view(1, -1), **FEATS)
        y = irfd._decode_eval(torch.cat([fi.view(S, -1), f], 1), None, "f32", "rgb", dict(seed_rows=seeds, frame_rows=counters))
        half = rows * torch.tensor([0.5, 0.5, 1.0, 1.0], device=dev)
        matte = ops.matte_from_landmarks(y_lm, half, R, CONTOUR, softness=6.0, grow=3.0, fallback=[tuple(2.0 * v for v in TEMPLATE5[i]) for i in CONTOUR])
        sums = ops.paste_colour_sums(y, frames, half, matte=matte, feather=4, channel_order="bgr")
        colour = ops.colour_rows_causal_feeds(sums.view(1, S, 13), c_state, 0.8).view(S, 3, 2)
        want = ops.frames_paste_u8_aligned(y, frames, half, matte=matte, colour=colour, feather=4, channel_order="bgr")
        assert torch.equal(base["outs"][t], want), t
        counters += 1
    room = base["room"]
    assert torch.equal(room.lm_state, lm_state) and torch.equal(room.feature_state, f_state) and torch.equal(room.colour_state, c_state)
    assert torch.equal(room.frames, counters) and torch.equal(room.seeds, seeds)
    # the held tick of feed 1 is pasted (not passed through), and the three feeds differ where they show the same frame
    assert not torch.equal(base["outs"][1, 1], c["frames"][1, 1]) and not torch.equal(base["outs"][1, 0], base["outs"][0, 1])


@pytest.mark.parametrize("features", [None, FEATS], ids=["features off", "features on"])
def test_a_slot_is_a_session(irfd, feeds, base, features):
    if features is None:
        room = irfd.live_room(feeds["photos"], features=None, seed=SEEDS, **COMMON)
        outs, states = run_room(room, feeds)
    else:
        room, outs, states = base["room"], base["outs"], base["states"]
    for s in range(S):
        session = irfd.live(feeds["photos"][s], features=features, seed=SEEDS[s], **COMMON)
        assert torch.equal(room.fi[s], session.fi[0])
        want, want_states = run_session(session, feeds, s)
        assert torch.equal(states[:, s], want_states), s                     # to the bit, after every tick
        assert torch.equal(outs[:, s], want), s                              # to the byte
        assert session.frames == T == int(room.frames[s])


def test_reset_and_set_identity_touch_one_slot(irfd, feeds, base):
    c = feeds
    # reset(1) ahead of tick 2
    room = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **COMMON)
    outs, _ = run_room(room, c, before=lambda t: room.reset(1) if t == 2 else None)
    assert torch.equal(outs[:, 0], base["outs"][:, 0]) and torch.equal(outs[:, 2], base["outs"][:, 2])
    assert torch.equal(outs[:2, 1], base["outs"][:2, 1]) and not torch.equal(outs[2:, 1], base["outs"][2:, 1])
    fresh = irfd.live(c["photos"][1], features=FEATS, seed=SEEDS[1], **COMMON)
    assert torch.equal(outs[2:, 1], run_session(fresh, c, 1, range(2, T))[0])
    assert room.frames.tolist() == [T, T - 2, T]
    # set_identity(2, another photo) ahead of tick 3: the state of slot 2 starts over with the new fi
    other = BC.frames(43, 44, 60, 3).to(c["frames"].device)
    room = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **COMMON)
    fi_before = room.fi.clone()
    outs, _ = run_room(room, c, before=lambda t: room.set_identity(2, other) if t == 3 else None)
    assert torch.equal(outs[:, :2], base["outs"][:, :2]) and torch.equal(outs[:3, 2], base["outs"][:3, 2])
    assert not torch.equal(outs[3:, 2], base["outs"][3:, 2])
    fresh = irfd.live(other, features=FEATS, seed=SEEDS[2], **COMMON)
    assert torch.equal(room.fi[2], fresh.fi[0]) and torch.equal(room.fi[:2], fi_before[:2]) and not torch.equal(room.fi[2], fi_before[2])
    assert torch.equal(outs[3:, 2], run_session(fresh, c, 2, range(3, T))[0])
    assert room.frames.tolist() == [T, T, T - 3]
    # reset() of every slot: the room runs the clip again, to the byte
    room.set_identity(2, c["photos"][2])
    room.reset()
    assert not room.lm_state.any() and not room.feature_state.any() and not room.colour_state.any() and not room.frames.any()
    assert torch.equal(run_room(room, c)[0], base["outs"])


def test_a_slot_lost_beyond_hold_passes_through_and_restarts_clean(irfd, feeds, dev):
    c = feeds
    lm = c["lm"].clone()
    lm[1:4, 1] = float("nan")                                               # hold = 1: tick 1 is held, ticks 2 and 3 have expired
    kw = dict(COMMON, track=dict(hold=1), features=dict(hold=1), colour_decay=0.0, noise="fixed")
    room = irfd.live_room(c["photos"], seed=SEEDS, **kw)
    outs = torch.stack([room.step(c["frames"][t], lm[t]) for t in range(T)])
    assert torch.equal(outs[2:4, 1], c["frames"][2:4, 1])
    for t in (0, 1, 4):
        assert not torch.equal(outs[t, 1], c["frames"][t, 1]), t
    for s in (0, 2):                                                        # the neighbours are pasted in every tick
        assert all(not torch.equal(outs[t, s], c["frames"][t, s]) for t in range(T))
    assert room.lm_state.view(S, 5, 6)[1, :, 0].tolist() == [1.0] * 5 and room.frames.tolist() == [0] * S      # fixed noise: index 0
    fresh = irfd.live(c["photos"][1], seed=SEEDS[1], **kw)
    assert torch.equal(fresh.step(c["frames"][4, 1:2], lm[4, 1:2])[0], outs[4, 1])
    # a room that never saw a face passes everything through
    blind = irfd.live_room(c["photos"], seed=SEEDS, **kw)
    assert torch.equal(blind.step(c["frames"][0], torch.full_like(lm[0], float("nan"))), c["frames"][0]) and not blind.lm_state.any()


def test_the_launches_of_a_step_do_not_depend_on_s(irfd, pkg, feeds, monkeypatch):
    c, lib = feeds, pkg._lib.lib()
    names = ("spk_launch_list", "spk_causal_filter", "spk_sim_fit_landmarks", "spk_matte_from_landmarks", "spk_colour_rows_causal",
             "spk_colour_rows_causal_feeds", "spk_noise_fill", "spk_noise_fill_rows", "spk_frames_paste_u8_sim_blend", "spk_frames_paste_u8_sim",
             "spk_paste_colour_sums_sim", "spk_paste_colour_match_sim", "spk_frames_u8_to_f32_sim", "spk_sim_smooth", "spk_colour_rows_window",
             "spk_conv2d_fwd")

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
    per_step = {"spk_launch_list": 3, "spk_causal_filter": 1, "spk_sim_fit_landmarks": 1, "spk_frames_u8_to_f32_sim": 1,
                "spk_matte_from_landmarks": 1, "spk_paste_colour_sums_sim": 1, "spk_colour_rows_causal_feeds": 1, "spk_frames_paste_u8_sim_blend": 1}
    for n_feeds in (1, S):
        photos = c["photos"][:n_feeds]
        irfd.live_room(photos, **kw)                                        # Ei's plan for one image exists from here on
        room, calls = counted(lambda: irfd.live_room(photos, **kw))
        assert calls == {"spk_launch_list": n_feeds}, calls                 # Ei, once per photo
        room.step(c["frames"][0, :n_feeds], c["lm"][0, :n_feeds])           # the plans of this batch exist from here on
        for t in (1, 2):
            _, calls = counted(lambda: room.step(c["frames"][t, :n_feeds], c["lm"][t, :n_feeds]))
            assert calls == per_step, (n_feeds, calls)                      # Ee, Ep, Gd with the rows noise inside its list
        both = irfd.live_room(photos, features={}, **kw)
        both.step(c["frames"][0, :n_feeds], c["lm"][0, :n_feeds])
        _, calls = counted(lambda: both.step(c["frames"][1, :n_feeds], c["lm"][1, :n_feeds], emotion_u8=c["frames"][2, :n_feeds]))
        assert calls == dict(per_step, spk_causal_filter=2, spk_frames_u8_to_f32_sim=2), (n_feeds, calls)
        _, calls = counted(lambda: (both.reset(0), both.reset()))
        assert calls == {}, calls


def test_a_room_of_one_is_a_session(irfd, feeds):
    c = feeds
    kw = dict(COMMON, features=FEATS, seed=SEEDS[1])
    room, session = irfd.live_room(c["photos"][1:2], **kw), irfd.live(c["photos"][1], **kw)
    assert room.S == 1 and torch.equal(room.fi, session.fi)
    for t in range(T):
        tick = c["frames"][t, 1:2].clone()
        keep = tick.clone()
        want = session.step(keep, c["lm"][t, 1:2])
        got = room.step(tick, c["lm"][t, 1:2], inplace=True)
        assert got is tick and torch.equal(got, want) and not torch.equal(got, keep), t
        assert torch.equal(room.lm_state, session.lm_state) and torch.equal(room.colour_state[0], session.colour_state)
        assert torch.equal(room.feature_state, session.feature_state)       # one kernel at one batch: these too, to the bit
    # weights per feed or one set for all: the same bytes where they say the same
    w = [1.0, 0.5, 2.0, 1.0, 0.25]
    a, b = irfd.live_room(c["photos"], seed=SEEDS, **COMMON), irfd.live_room(c["photos"], seed=SEEDS, **COMMON)
    wd = torch.tensor([w] * S, device=c["frames"].device)
    assert torch.equal(a.step(c["frames"][0], c["lm"][0], weights=w), b.step(c["frames"][0], c["lm"][0], weights=wd))
    assert torch.equal(a.lm_state, b.lm_state)
    assert not torch.equal(a.step(c["frames"][1], c["lm"][1], weights=w), b.step(c["frames"][1], c["lm"][1]))
