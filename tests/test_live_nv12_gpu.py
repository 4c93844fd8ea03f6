"""GPU checks of ``IRFD.live`` / ``IRFD.live_room`` with ``pixel_format="nv12"`` (speak-hack_amd/live.py over csrc/frame_sim_nv12.hip
and csrc/frame_table_nv12.hip).  A session: with the filters off a step is the composition of the public ``ops`` written out here,
byte for byte; with them on, any split of the frames gives the same bytes and states, the landmark filter is the rgb24 session's to
the bit, a feed lost beyond ``hold`` gets its surface back; cloned and in place agree.  A room: slot ``s`` is an NV12 session on feed
``s`` alone, over one ``[S,3H/2,W]`` tensor and over a list of three surfaces of three sizes (one a region of interest), whose
padding stays untouched; a list of same-size allocations is the step on their stack; a tick on a list makes today's library calls
with the three ``_nv12_sim_table`` entry points; and every refusal comes before a launch.  Model, template, settings and seeds are
those of tests/test_live_room_table_gpu.py; S = 3 feeds, T = 3 ticks, ``features`` on."""
import importlib

import numpy as np
import pytest
import torch

import blend_cases as BC
import landmark_ref as LR
import nv12_sim_cases as NS
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
NV12 = dict(COMMON, pixel_format="nv12")
# per feed: (surface H, W, region offset y, x, H, W); feed 1 is a 40 x 52 region at (2, 4) of a 44 x 60 surface
LAYOUT = [(48, 64, 0, 0, 48, 64), (44, 60, 2, 4, 40, 52), (56, 72, 0, 0, 56, 72)]
PAD = 0xA5


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


def surface(seed, N, h, w, dev, pitch=None):
    """N surfaces from random RGB as one tensor [N,3h/2,w] of row pitch ``pitch`` (the padding is PAD)"""
    y, uv = NS.surface_from_rgb(seed, N, h, w)
    buf = torch.full((N, 3 * h // 2, pitch or w), PAD, dtype=torch.uint8)
    buf[:, :h, :w], buf[:, h:, :w] = y, uv.reshape(N, h // 2, w)
    return buf.to(dev)[:, :, :w]


@pytest.fixture(scope="module")
def feeds(pkg, dev):
    """Three identity photos; a session's feed (T surfaces of 48 x 64 at pitch 80); same-size feeds [T,S,72,64] and mixed-size feeds
    (LAYOUT: whole surfaces [T,3H/2,W] per feed), with their landmarks [T,S,5,2]; feed 1 loses a whole frame in tick 1"""
    rng = np.random.default_rng(29)
    photos = [BC.frames(31, 56, 72, 3).to(dev), BC.frames(41, 40, 52, 3).to(dev), BC.frames(42, 1, 64, 48, 3).to(dev)]
    one = surface(32, T, 48, 64, dev, pitch=80)
    one_lm = tracked(pkg, rng, 48, 64).to(dev)
    same = surface(33, T * S, 48, 64, dev).view(T, S, 72, 64)
    same_lm = torch.stack([tracked(pkg, rng, 48, 64) for _ in range(S)], 1).to(dev)
    mixed = [surface(50 + s, T, bh, bw, dev) for s, (bh, bw, *_) in enumerate(LAYOUT)]
    mixed_lm = torch.stack([tracked(pkg, rng, h, w) for *_, h, w in LAYOUT], 1).to(dev)
    same_lm[1, 1] = float("nan")
    mixed_lm[1, 1] = float("nan")
    return dict(photos=photos, one=one, one_lm=one_lm, same=same, same_lm=same_lm, mixed=mixed, mixed_lm=mixed_lm)


def states(live):
    frames = live.frames if isinstance(live.frames, torch.Tensor) else torch.tensor(live.frames)
    return [t.clone() for t in (live.lm_state, live.feature_state, live.colour_state, frames)]


def same_states(a, b):
    return len(a) == len(b) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))


def view(whole, s):
    """Feed ``s``'s surface for a tick out of its whole surface [3H/2,W]: the region of interest as a pair of plane views"""
    bh, bw, y0, x0, h, w = LAYOUT[s]
    if (y0, x0, h, w) == (0, 0, bh, bw):
        return whole
    return whole[:bh][y0:y0 + h, x0:x0 + w], whole[bh:][y0 // 2:(y0 + h) // 2, x0:x0 + w].unflatten(1, (w // 2, 2))


def planes(pkg, surf):
    return pkg.ops.nv12_planes(surf)


def same_surface(pkg, a, b):
    (ya, ua), (yb, ub) = planes(pkg, a), planes(pkg, b)
    return torch.equal(ya, yb) and torch.equal(ua, ub)


# ---- a session ------------------------------------------------------------------------------------------------------------------
def test_filters_off_is_the_composition_of_ops(irfd, pkg, feeds, dev):
    c, ops = feeds, pkg.ops
    surf, lm = c["one"], c["one_lm"]
    assert surf.stride(1) == 80 and not surf.is_contiguous()
    keep = surf.clone()
    s = irfd.live(c["photos"][0], **dict(NV12, track=None, features=None, colour_decay=0.0), seed=7)
    got = s.step(surf, lm)
    assert got.dtype == torch.uint8 and got.shape == (T, 72, 64) and got.is_contiguous() and s.frames == T and torch.equal(surf, keep)
    rows = ops.similarity_from_landmarks(lm, TEMPLATE5)
    pose = ops.frames_from_nv12_aligned(surf, SIZE, rows)
    fe, fp = irfd.encode(pose, "Ee"), irfd.encode(pose, "Ep")
    gin = irfd._prepare_generator_input(s.fi.expand(T, -1, -1, -1), fe, fp)
    y = irfd._decode_eval(gin, None, "f32", "rgb", dict(seed=7, frame0=0, fixed_noise=False))
    Hs, Ws = y.shape[2:]
    gen = rows * torch.tensor([SIZE / Ws, SIZE / Ws, 1.0, 1.0], device=dev)
    matte = ops.matte_from_landmarks(lm, gen, (Hs, Ws), CONTOUR, softness=6.0, grow=3.0, smooth=0,
                                     fallback=[tuple(Ws / SIZE * v for v in TEMPLATE5[i]) for i in CONTOUR])
    colour = ops.paste_colour_match_nv12(y, surf, gen, matte=matte, feather=4)
    want = ops.frames_paste_nv12_aligned(y, surf, gen, matte=matte, colour=colour, feather=4)
    assert torch.equal(got, want) and not torch.equal(got, keep.contiguous())
    # the same feed as a pair of planes; and another colour is another result
    s.reset()
    assert torch.equal(s.step(ops.nv12_planes(surf), lm), want)
    wide = irfd.live(c["photos"][0], **dict(NV12, track=None, features=None, colour_decay=0.0), seed=7, standard="bt709", full_range=True)
    assert not torch.equal(wide.step(surf, lm), want)


def test_filters_on_any_split_and_the_rgb24_landmark_filter(irfd, pkg, feeds, dev):
    c = feeds
    surf, lm = c["one"], c["one_lm"].clone()
    lm[1, 3] = float("nan")                                                 # one point lost for a frame: held
    s = irfd.live(c["photos"][0], features=FEATS, seed=7, **NV12)
    whole = s.step(surf, lm)
    was = states(s)
    assert s.frames == T and all(bool(t.any()) for t in was)
    s.reset()
    assert not s.lm_state.any() and not s.feature_state.any() and not s.colour_state.any() and s.frames == 0
    split = torch.cat([s.step(surf[:1], lm[:1]), s.step(surf[1:], lm[1:])])
    assert torch.equal(split, whole) and same_states(states(s), was)
    for t in range(T):                                                      # a frame that was pasted differs from its input
        assert not torch.equal(whole[t], surf[t]), t
    # the landmark filter never sees a pixel: its state is the rgb24 session's on the same landmarks, to the bit
    rgb = irfd.live(c["photos"][0], features=FEATS, seed=7, **COMMON)
    rgb.step(BC.frames(34, T, 48, 64, 3).to(dev), lm)
    assert torch.equal(rgb.lm_state, s.lm_state) and rgb.frames == s.frames == T
    # lost for longer than hold: the surface comes back byte for byte; the held frame is pasted
    gone = c["one_lm"].clone()
    gone[1:] = float("nan")
    short = irfd.live(c["photos"][0], seed=7, **dict(NV12, track=dict(hold=1), features=dict(hold=1)))
    out = short.step(surf, gone)
    assert torch.equal(out[2], surf[2]) and not torch.equal(out[1], surf[1]) and not torch.equal(out[0], surf[0])


def test_cloned_and_in_place_give_the_same_bytes(irfd, pkg, feeds, dev):
    c = feeds
    surf, lm = c["one"], c["one_lm"]
    keep = surf.clone()
    s = irfd.live(c["photos"][0], features=FEATS, seed=7, **NV12)
    cloned = s.step(surf, lm)
    assert torch.equal(surf, keep) and cloned.data_ptr() != surf.data_ptr()
    s.reset()
    mine = surface(32, T, 48, 64, dev, pitch=80)
    assert s.step(mine, lm, inplace=True) is mine and torch.equal(mine, cloned)
    assert bool((mine._base[:, :, 64:] == PAD).all())                        # the pitch padding is untouched
    s.reset()
    pair = pkg.ops.nv12_planes(surface(32, T, 48, 64, dev, pitch=80))
    assert s.step(pair, lm, inplace=True) is pair and same_surface(pkg, pair, cloned)
    emo = surface(35, T, 48, 64, dev)
    s.reset()
    assert not torch.equal(s.step(surf, lm, emotion_u8=emo), cloned)


# ---- a room ---------------------------------------------------------------------------------------------------------------------
def test_a_room_over_one_tensor_is_three_sessions(irfd, pkg, feeds):
    c = feeds
    room = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **NV12)
    sessions = [irfd.live(c["photos"][s], features=FEATS, seed=SEEDS[s], **NV12) for s in range(S)]
    K = room.K
    for t in range(T):
        tick = c["same"][t]
        keep = tick.clone()
        got = room.step(tick, c["same_lm"][t])
        assert got.shape == (S, 72, 64) and torch.equal(tick, keep)
        for s in range(S):
            want = sessions[s].step(tick[s:s + 1], c["same_lm"][t, s:s + 1])[0]
            assert torch.equal(got[s], want), (t, s)                        # to the byte
            assert torch.equal(room.lm_state.view(S, K, 6)[s], sessions[s].lm_state.view(K, 6)), (t, s)
            assert torch.equal(room.colour_state[s], sessions[s].colour_state), (t, s)
            assert not torch.equal(got[s], tick[s]), (t, s)                 # pasted in every tick: the lost frame of feed 1 is held
    assert room.frames.tolist() == [T] * S and [x.frames for x in sessions] == [T] * S
    # in place on one tensor returns the tensor; on a pair of planes, the pair
    again = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **NV12)
    tick = c["same"][0].clone()
    first = again.step(c["same"][0], c["same_lm"][0])
    again.reset()
    assert again.step(tick, c["same_lm"][0], inplace=True) is tick and torch.equal(tick, first)


def test_feeds_of_three_sizes_are_three_sessions(irfd, pkg, feeds):
    c = feeds
    room = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **NV12)
    sessions = [irfd.live(c["photos"][s], features=FEATS, seed=SEEDS[s], **NV12) for s in range(S)]
    K = room.K
    for t in range(T):
        wholes = [c["mixed"][s][t].clone() for s in range(S)]
        before = [w.clone() for w in wholes]
        surfaces = [view(wholes[s], s) for s in range(S)]
        assert isinstance(surfaces[1], tuple) and surfaces[1][0].stride(0) == 60 and tuple(surfaces[1][0].shape) == (40, 52)
        got = room.step(surfaces, c["mixed_lm"][t], inplace=True)
        assert got is surfaces
        for s in range(S):
            own = view(before[s], s)
            own = tuple(p.unsqueeze(0) for p in own) if isinstance(own, tuple) else own.unsqueeze(0)
            want = sessions[s].step(own, c["mixed_lm"][t, s:s + 1])
            assert same_surface(pkg, surfaces[s], want[0]), (t, s)           # to the byte
            assert torch.equal(room.lm_state.view(S, K, 6)[s], sessions[s].lm_state.view(K, 6)), (t, s)
            assert torch.equal(room.colour_state[s], sessions[s].colour_state), (t, s)
            assert not same_surface(pkg, surfaces[s], view(before[s], s)), (t, s)
            rest = wholes[s].clone()                                        # the padding of the surface is untouched
            for mine, kept in zip(planes(pkg, view(rest, s)), planes(pkg, view(before[s], s))):
                mine.copy_(kept)
            assert torch.equal(rest, before[s]), (t, s)
    assert room.frames.tolist() == [T] * S and [x.frames for x in sessions] == [T] * S


@pytest.mark.parametrize("inplace", [False, True], ids=["cloned", "in place"])
def test_a_list_of_one_size_is_the_stack(irfd, pkg, feeds, inplace):
    c = feeds
    stacked = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **NV12)
    listed = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **NV12)
    for t in range(T):
        surfaces = [c["same"][t, s].clone() for s in range(S)]              # three allocations
        keep = [f.clone() for f in surfaces]
        want = stacked.step(torch.stack(surfaces), c["same_lm"][t], inplace=inplace)
        got = listed.step(surfaces, c["same_lm"][t], inplace=inplace)
        assert isinstance(got, list) and len(got) == S and torch.equal(torch.stack(got), want), t
        assert same_states(states(listed), states(stacked)), t
        if inplace:
            assert got is surfaces and all(a is b for a, b in zip(got, surfaces))
        else:
            assert all(a is not b and torch.equal(b, k) for a, b, k in zip(got, surfaces, keep))      # new tensors, the caller's untouched
        assert not torch.equal(want, torch.stack(keep))
    assert listed.frames.tolist() == [T] * S
    # a SurfaceTable is taken as the list it was made from
    table = pkg.ops.SurfaceTable([c["same"][0, s].clone() for s in range(S)])
    out = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **NV12).step(table, c["same_lm"][0], inplace=True)
    assert all(a is b for a, b in zip(out, table.surfaces))


def test_a_tick_makes_todays_calls_with_the_table_entry_points(irfd, pkg, feeds, monkeypatch):
    c, lib = feeds, pkg._lib.lib()
    others = ("spk_frames_paste_nv12_sim", "spk_paste_colour_sums_nv12_sim", "spk_paste_colour_match_nv12_sim", "spk_frames_nv12_to_f32_sim",
              "spk_frames_paste_u8_sim_blend", "spk_frames_paste_u8_sim", "spk_paste_colour_sums_sim", "spk_paste_colour_match_sim",
              "spk_frames_u8_to_f32_sim", "spk_frames_u8_to_f32_sim_table", "spk_frames_paste_u8_sim_table", "spk_paste_colour_sums_sim_table",
              "spk_paste_colour_match_sim_table", "spk_frames_nv12_to_f32", "spk_frames_paste_nv12", "spk_frames_f32_to_nv12")
    names = ("spk_launch_list", "spk_causal_filter", "spk_sim_fit_landmarks", "spk_matte_from_landmarks", "spk_colour_rows_causal",
             "spk_colour_rows_causal_feeds", "spk_noise_fill", "spk_noise_fill_rows", "spk_sim_smooth", "spk_colour_rows_window", "spk_conv2d_fwd",
             "spk_frames_nv12_to_f32_sim_table", "spk_frames_paste_nv12_sim_table", "spk_paste_colour_sums_nv12_sim_table",
             "spk_paste_colour_match_nv12_sim_table") + others

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

    kw = dict(NV12, seed=7)
    per_step = {"spk_launch_list": 3, "spk_causal_filter": 1, "spk_sim_fit_landmarks": 1, "spk_frames_nv12_to_f32_sim_table": 1,
                "spk_matte_from_landmarks": 1, "spk_paste_colour_sums_nv12_sim_table": 1, "spk_colour_rows_causal_feeds": 1,
                "spk_frames_paste_nv12_sim_table": 1}
    assert not set(per_step) & set(others)

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
        assert calls == dict(per_step, spk_causal_filter=2, spk_frames_nv12_to_f32_sim_table=2), (n_feeds, calls)


def test_refusals_leave_the_states_and_the_buffers_as_they_were(irfd, pkg, feeds, dev):
    c, L = feeds, pkg._lib
    room = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **NV12)
    lm = c["mixed_lm"][0]
    room.step([view(c["mixed"][s][0].clone(), s) for s in range(S)], lm, inplace=True)    # a room in mid-call: its states are not empty
    wholes = [c["mixed"][s][1].clone() for s in range(S)]
    surfaces = [view(wholes[s], s) for s in range(S)]
    before, was = [w.clone() for w in wholes], states(room)
    assert all(bool(t.any()) for t in was)
    wide = torch.zeros(72, 128, dtype=torch.uint8, device=dev)
    odd = torch.zeros(69, 64, dtype=torch.uint8, device=dev)                # its first 63 columns: 46 x 63
    refused = [(ValueError, dict(frames_u8=surfaces[:2])),                                      # wrong list length
               (ValueError, dict(frames_u8=surfaces + surfaces[:1])),
               (ValueError, dict(frames_u8=[surfaces[0], None, surfaces[2]])),                  # a None element
               (ValueError, dict(frames_u8=[surfaces[0], surfaces[1], odd[:, :63]])),           # an odd size
               (ValueError, dict(frames_u8=[surfaces[0], surfaces[1], surfaces[2].float()])),   # wrong dtype
               (L.SpkError, dict(frames_u8=[surfaces[0].cpu(), surfaces[1], surfaces[2]])),     # wrong device
               (ValueError, dict(frames_u8=[wide[:, ::2], surfaces[1], surfaces[2]])),          # a pixel stride
               (ValueError, dict(frames_u8=surfaces, emotion_u8=[surfaces[2], surfaces[1], surfaces[0]])),  # sizes differ feed by feed
               (ValueError, dict(frames_u8=surfaces, emotion_u8=surfaces[:2])),
               (L.SpkError, dict(frames_u8=[surfaces[0], surfaces[1], (surfaces[1][0][4:30, 4:40], surfaces[1][1][2:15, 2:20])], inplace=True)),
               (L.SpkError, dict(frames_u8=[surfaces[0], surfaces[0], surfaces[2]], inplace=True))]          # elements that share bytes
    for n, (error, kw) in enumerate(refused):
        with pytest.raises(error):
            room.step(landmarks=lm, **kw)
        assert same_states(states(room), was), n
    assert all(torch.equal(a, b) for a, b in zip(wholes, before))
    # what was refused in place is fine where every surface is cloned first, and the room goes on
    out = room.step([surfaces[0], surfaces[0], surfaces[2]], lm)
    assert len(out) == S and out[0] is not out[1] and all(torch.equal(a, b) for a, b in zip(wholes, before))
    assert not same_states(states(room), was)
    # a session, and a room over one tensor: the same kinds, refused before the filters have moved
    s = irfd.live(c["photos"][0], features=FEATS, seed=7, **NV12)
    surf, one_lm = c["one"].clone(), c["one_lm"]
    s.step(surf, one_lm)
    was, keep = states(s), surf.clone()
    stack = torch.zeros(2, 72, 64, dtype=torch.uint8, device=dev)
    refused = [(ValueError, dict(frames_u8=surf[:, :71])),                                      # rows that are not 3H/2
               (ValueError, dict(frames_u8=surf[:, :, :63])),                                   # an odd width
               (ValueError, dict(frames_u8=surf.float())),
               (ValueError, dict(frames_u8=[surf[0], surf[1], surf[2]])),                       # a session takes one tensor or a pair
               (L.SpkError, dict(frames_u8=surf.cpu())),
               (ValueError, dict(frames_u8=torch.zeros(T, 72, 128, dtype=torch.uint8, device=dev)[:, :, ::2])),
               (ValueError, dict(frames_u8=surf, emotion_u8=surf[:2])),
               (ValueError, dict(frames_u8=surf, emotion_u8=torch.zeros(T, 60, 64, dtype=torch.uint8, device=dev))),
               (L.SpkError, dict(frames_u8=surf, emotion_u8=surf.cpu())),
               (L.SpkError, dict(frames_u8=stack[:1].expand(T, 72, 64), inplace=True))]         # frames that share bytes
    for n, (error, kw) in enumerate(refused):
        with pytest.raises(error):
            s.step(landmarks=one_lm, **kw)
        assert same_states(states(s), was), n
    assert torch.equal(surf, keep) and not stack.any()
    one = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **NV12)
    one.step(c["same"][0], c["same_lm"][0])
    was = states(one)
    for error, kw in [(ValueError, dict(frames_u8=c["same"][1][:2])), (L.SpkError, dict(frames_u8=c["same"][1].cpu())),
                      (ValueError, dict(frames_u8=c["same"][1], emotion_u8=c["same"][1][:, :60])),
                      (L.SpkError, dict(frames_u8=stack[:1].expand(S, 72, 64), inplace=True))]:
        with pytest.raises(error):
            one.step(landmarks=c["same_lm"][1], **kw)
        assert same_states(states(one), was)
    assert not stack.any()
