"""GPU checks of ``IRFD.live`` / ``IRFD.live_room`` with ``pixel_format="rgb32"`` (speak-hack_amd/live.py over csrc/frame_sim_rgb32.hip
and csrc/frame_table_rgb32.hip).  The criterion is the rgb24 session / room of tests/test_live_room_table_gpu.py on the STRIPPED
feeds: a session and a room on RGB32 feeds -- one pitched tensor, an ``Rgb32Table``, a list of three frames of three sizes one of
which is a region of interest at a pixel offset -- give the same colour bytes and the same filter, feature and colour states, bit for
bit, and leave every fourth byte, pitch byte and surrounding byte as it was; any split of the frames gives the same bytes;
``inplace=True`` writes the caller's buffer; ``room.reset(slot)`` touches one slot; a tick on a list calls the three
``_rgb32_sim_table`` entry points and no other of the video edge; every refusal comes before a launch.  Model, template, settings,
seeds, feeds and layout are that file's (S = 3, T = 3, SIZE 128), imported from it: one model load for the module."""
import pytest
import torch

from test_live_room_table_gpu import COMMON, FEATS, LAYOUT, S, SEEDS, T, dev, feeds, irfd, pkg, same_states, states, view  # noqa: F401

pytestmark = pytest.mark.gpu
PAD, FRONT, BACK = 0xA5, 68, 60
ORDER = "bgra"                                                             # COMMON has channel_order="bgr": its order with an alpha behind it
RGB32 = dict(COMMON, pixel_format="rgb32", channel_order=ORDER)


def widen(colour, order=ORDER, seed=5):
    """Packed frames [...,H,W,3] on the device -> RGB32 frames [...,H,W,4] with the same colour bytes at the order's offset, a random
    fourth byte below 255, at row pitch 4 W + 16 (padding PAD) between guards of FRONT and BACK bytes: the first pixel is 4-aligned
    and not 16-aligned"""
    *lead, H, W, _ = colour.shape
    n = 1
    for k in lead:
        n *= k
    pitch = 4 * W + 16
    raw = torch.full((FRONT + BACK + n * H * pitch,), PAD, dtype=torch.uint8, device=colour.device)
    out = raw[FRONT:FRONT + n * H * pitch].view(*lead, H, pitch)[..., :4 * W].unflatten(-1, (W, 4))
    first = 1 if order[0] == "a" else 0
    out[..., first:first + 3] = colour
    g = torch.Generator().manual_seed(seed)
    out[..., 3 - 3 * first] = torch.randint(0, 255, (*lead, H, W), generator=g, dtype=torch.uint8).to(colour.device)
    assert out.data_ptr() % 16 == 4 and not out.is_contiguous()
    return out


def colour_of(frames, order=ORDER):
    first = 1 if order[0] == "a" else 0
    return frames[..., first:first + 3]


def fourth_of(frames, order=ORDER):
    return frames[..., 0 if order[0] == "a" else 3]


def session_states(s):
    return [t.clone() for t in (s.lm_state, s.feature_state, s.colour_state)]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def padding_intact(frames):
    """The pitch bytes and the guards of a tensor ``widen`` made"""
    raw, W = frames._base, frames.size(-2)
    body = raw[FRONT:-BACK].view(-1, 4 * W + 16)
    return bool((body[:, 4 * W:] == PAD).all()) and bool((raw[:FRONT] == PAD).all()) and bool((raw[-BACK:] == PAD).all())


# ---- a session ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["bgra", "abgr"])
def test_a_session_is_the_rgb24_session_on_the_stripped_feed(irfd, pkg, feeds, dev, order):
    c = feeds
    stripped, lm = c["same"][:, 0].contiguous(), c["same_lm"][:, 0].clone()
    lm[1, 3] = float("nan")                                                 # one point lost for a frame: held
    theirs = irfd.live(c["photos"][0], features=FEATS, seed=7, **COMMON)
    want = theirs.step(stripped, lm)
    mine = irfd.live(c["photos"][0], features=FEATS, seed=7, **dict(RGB32, channel_order=order))
    feed = widen(stripped, order)
    keep = feed.clone()
    whole = mine.step(feed, lm)
    assert whole.dtype == torch.uint8 and tuple(whole.shape) == (T, 48, 64, 4) and whole.is_contiguous() and mine.frames == T
    assert torch.equal(colour_of(whole, order), want) and torch.equal(fourth_of(whole, order), fourth_of(keep, order))
    assert torch.equal(feed, keep) and padding_intact(feed)
    was = session_states(mine)
    assert same(was, session_states(theirs)) and all(bool(t.any()) for t in was)          # filter, feature and colour states, bit for bit
    for t in range(T):
        assert not torch.equal(whole[t], keep[t]), t                        # a frame that was pasted differs from its input
    # any split of the frames, and a contiguous feed
    mine.reset()
    split = torch.cat([mine.step(feed[:1], lm[:1]), mine.step(feed[1:], lm[1:])])
    assert torch.equal(split, whole) and same(session_states(mine), was)
    mine.reset()
    assert torch.equal(mine.step(feed.contiguous(), lm), whole) and same(session_states(mine), was)
    # in place: the caller's buffer, with the same bytes, its padding untouched
    mine.reset()
    assert mine.step(feed, lm, inplace=True) is feed and torch.equal(feed, whole) and padding_intact(feed)
    # the emotion feed is taken in the same form
    other = torch.randint(0, 256, stripped.shape, generator=torch.Generator().manual_seed(35), dtype=torch.uint8).to(dev)
    mine.reset(), theirs.reset()
    got = mine.step(keep, lm, emotion_u8=widen(other, order, seed=9))
    assert torch.equal(colour_of(got, order), theirs.step(stripped, lm, emotion_u8=other))
    # lost for longer than hold: the frame comes back byte for byte; the held frame is pasted
    gone = c["same_lm"][:, 0].clone()
    gone[1:] = float("nan")
    short = irfd.live(c["photos"][0], seed=7, **dict(RGB32, channel_order=order, track=dict(hold=1), features=dict(hold=1)))
    out = short.step(keep, gone)
    assert torch.equal(out[2], keep[2]) and not torch.equal(out[1], keep[1]) and not torch.equal(out[0], keep[0])


# ---- a room ---------------------------------------------------------------------------------------------------------------------
def test_a_room_over_one_tensor_and_over_a_table_is_the_rgb24_room(irfd, pkg, feeds):
    c = feeds
    mine = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **RGB32)
    tabled = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **RGB32)
    theirs = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **COMMON)
    for t in range(T):
        tick = widen(c["same"][t])
        keep = tick.clone()
        got, want = mine.step(tick, c["same_lm"][t]), theirs.step(c["same"][t], c["same_lm"][t])
        assert tuple(got.shape) == (S, 48, 64, 4) and torch.equal(tick, keep), t
        assert torch.equal(colour_of(got), want) and torch.equal(fourth_of(got), fourth_of(keep)), t
        assert same_states(states(mine), states(theirs)), t
        assert all(not torch.equal(got[s], tick[s]) for s in range(S)), t   # pasted in every tick: the lost frame of feed 1 is held
        # an Rgb32Table over the same frames, in place: the table's tensors, with the same bytes
        again = widen(c["same"][t])
        table = pkg.ops.Rgb32Table(again)
        out = tabled.step(table, c["same_lm"][t], inplace=True)
        assert all(a is b for a, b in zip(out, table.frames)) and torch.equal(again, got) and padding_intact(again), t
        assert same_states(states(tabled), states(theirs)), t
    assert mine.frames.tolist() == [T] * S
    # in place on one tensor returns the tensor
    mine.reset()
    tick = widen(c["same"][0])
    first = mine.step(tick.clone(), c["same_lm"][0])
    mine.reset()
    assert mine.step(tick, c["same_lm"][0], inplace=True) is tick and torch.equal(tick, first) and padding_intact(tick)


def rois(wholes):
    """This tick's whole packed surfaces [bh,bw,3] per feed -> (the rgb24 frames as the rgb24 room takes them, the RGB32 frames: views
    of whole RGB32 surfaces in allocations of their own; the whole RGB32 surfaces)"""
    held = [widen(w, seed=60 + s) for s, w in enumerate(wholes)]
    return [view(w, s) for s, w in enumerate(wholes)], [view(h, s) for s, h in enumerate(held)], held


def test_feeds_of_three_sizes_are_the_rgb24_room(irfd, pkg, feeds):
    c = feeds
    mine = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **RGB32)
    theirs = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **COMMON)
    for t in range(T):
        wholes = [c["mixed"][s][t].clone() for s in range(S)]
        before = [w.clone() for w in wholes]
        packed, frames, held = rois(wholes)
        was = [h.clone() for h in held]
        assert tuple(frames[1].shape) == (40, 52, 4) and frames[1].stride(0) == 4 * 60 + 16 and frames[1].data_ptr() % 16 == 4
        got = mine.step(frames, c["mixed_lm"][t], inplace=True)
        assert got is frames
        theirs.step(packed, c["mixed_lm"][t], inplace=True)
        assert same_states(states(mine), states(theirs)), t
        for s in range(S):
            # the whole surfaces, region and surroundings: the colour bytes of the rgb24 room's whole surface, the fourth bytes as they were
            assert torch.equal(colour_of(held[s]), wholes[s]) and torch.equal(fourth_of(held[s]), fourth_of(was[s])), (t, s)
            assert not torch.equal(wholes[s], before[s]) and padding_intact(held[s]), (t, s)
    assert mine.frames.tolist() == [T] * S
    # cloned: a list of new contiguous tensors, the caller's surfaces untouched
    wholes = [c["mixed"][s][0].clone() for s in range(S)]
    _, frames, held = rois(wholes)
    keep = [h.clone() for h in held]
    room = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **RGB32)
    out = room.step(frames, c["mixed_lm"][0])
    assert isinstance(out, list) and [tuple(o.shape) for o in out] == [(h, w, 4) for *_, h, w in LAYOUT] and all(o.is_contiguous() for o in out)
    assert all(torch.equal(a, b) for a, b in zip(held, keep))
    room.reset()
    room.step(frames, c["mixed_lm"][0], inplace=True)
    assert all(torch.equal(f, o) for f, o in zip(frames, out))


def test_reset_touches_one_slot(irfd, feeds):
    c = feeds
    room = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **RGB32)
    fresh = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **RGB32)
    room.step(widen(c["same"][0]), c["same_lm"][0])
    was = [t.view(S, -1).clone() for t in states(room)]
    room.reset(1)
    now = [t.view(S, -1) for t in states(room)]
    assert all(torch.equal(n[s], w[s]) for n, w in zip(now, was) for s in (0, 2)) and all(not bool(n[1].any()) for n in now)
    assert all(bool(w[1].any()) for w in was)
    # slot 1 then starts over: its first tick is that of a fresh room's slot 1
    lm = c["same_lm"][0]
    got, first = room.step(widen(c["same"][0]), lm), fresh.step(widen(c["same"][0]), lm)
    assert torch.equal(got[1], first[1]) and not torch.equal(got[0], first[0])


def test_a_tick_on_a_list_calls_the_rgb32_table_entry_points(irfd, pkg, feeds, monkeypatch):
    c, lib = feeds, pkg._lib.lib()
    mine = ("spk_frames_rgb32_to_f32_sim_table", "spk_paste_colour_sums_rgb32_sim_table", "spk_frames_paste_rgb32_sim_table")
    names = [n for n in pkg._lib._PROTOTYPES if "frames_" in n or "paste_colour_" in n]         # every entry point of the video edge
    assert set(mine) <= set(names) and sum("rgb32" in n for n in names) == 9
    calls = dict.fromkeys(names, 0)

    def counting(n, real):
        def f(*a):
            calls[n] += 1
            return real(*a)
        return f

    room = irfd.live_room(c["photos"], seed=7, **RGB32)
    room.step(rois([c["mixed"][s][0].clone() for s in range(S)])[1], c["mixed_lm"][0], inplace=True)
    frames = rois([c["mixed"][s][1].clone() for s in range(S)])[1]
    for n in names:
        monkeypatch.setattr(lib, n, counting(n, getattr(lib, n)))
    room.step(frames, c["mixed_lm"][1], inplace=True)
    monkeypatch.undo()
    assert {n: k for n, k in calls.items() if k} == dict.fromkeys(mine, 1)


def test_refusals_leave_the_states_and_the_buffers_as_they_were(irfd, pkg, feeds, dev):
    c, L = feeds, pkg._lib
    room = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **RGB32)
    lm = c["mixed_lm"][0]
    room.step(rois([c["mixed"][s][0].clone() for s in range(S)])[1], lm, inplace=True)        # a room in mid-call: its states are not empty
    packed, frames, held = rois([c["mixed"][s][1].clone() for s in range(S)])
    before, was = [h.clone() for h in held], states(room)
    assert all(bool(t.any()) for t in was)
    wide = torch.zeros(40, 104, 4, dtype=torch.uint8, device=dev)
    odd = torch.zeros(56 * 72 * 4 + 1, dtype=torch.uint8, device=dev)[1:].view(56, 72, 4)
    refused = [(ValueError, dict(frames_u8=frames[:2])),                                        # wrong list length
               (ValueError, dict(frames_u8=frames + frames[:1])),
               (ValueError, dict(frames_u8=[frames[0], None, frames[2]])),                      # a None element
               (ValueError, dict(frames_u8=[frames[0], frames[1].float(), frames[2]])),         # wrong dtype
               (ValueError, dict(frames_u8=[frames[0], packed[1], frames[2]])),                 # a packed frame among them
               (ValueError, dict(frames_u8=packed)),                                            # the frames of another format
               (ValueError, dict(frames_u8=pkg.ops.FrameTable(packed))),                        # and its table
               (L.SpkError, dict(frames_u8=[frames[0], frames[1].cpu(), frames[2]])),           # wrong device
               (ValueError, dict(frames_u8=[frames[0], wide[:, ::2], frames[2]])),              # a pixel stride of 8
               (ValueError, dict(frames_u8=[frames[0], frames[1], odd])),                       # a misaligned frame
               (ValueError, dict(frames_u8=frames, emotion_u8=[frames[0], frames[2], frames[1]])),          # sizes differ feed by feed
               (ValueError, dict(frames_u8=frames, emotion_u8=frames[:2])),
               (L.SpkError, dict(frames_u8=[frames[0], frames[1], frames[1][4:30, 3:40]], inplace=True)),   # two elements in one buffer
               (L.SpkError, dict(frames_u8=[frames[0], frames[0], frames[2]], inplace=True))]
    for n, (error, kw) in enumerate(refused):
        with pytest.raises(error):
            room.step(landmarks=lm, **kw)
        assert same_states(states(room), was), n
    assert all(torch.equal(a, b) for a, b in zip(held, before)) and not wide.any() and not odd.any()
    # what was refused in place is fine where every frame is cloned first, and the room goes on
    out = room.step([frames[0], frames[0], frames[2]], lm)
    assert len(out) == S and out[0] is not out[1] and all(torch.equal(a, b) for a, b in zip(held, before))
    assert not same_states(states(room), was)
    # a session: the same kinds, refused before the filters have moved
    s = irfd.live(c["photos"][0], features=FEATS, seed=7, **RGB32)
    stripped, one_lm = c["same"][:, 0].contiguous(), c["same_lm"][:, 0]
    feed = widen(stripped)
    s.step(feed, one_lm)
    was, keep = session_states(s), feed.clone()
    misaligned = torch.zeros(T * 48 * 64 * 4 + 2, dtype=torch.uint8, device=dev)[2:].view(T, 48, 64, 4)
    refused = [(ValueError, dict(frames_u8=stripped)),                                          # a packed feed
               (ValueError, dict(frames_u8=feed[0])),                                           # one frame without its batch axis
               (ValueError, dict(frames_u8=[feed])),
               (L.SpkError, dict(frames_u8=feed.cpu())),
               (ValueError, dict(frames_u8=feed, emotion_u8=feed[:2])),
               (L.SpkError, dict(frames_u8=feed, emotion_u8=feed.cpu())),
               (L.SpkError, dict(frames_u8=misaligned, inplace=True)),                          # written frames must be aligned words
               (L.SpkError, dict(frames_u8=feed[:1].expand(T, -1, -1, -1), inplace=True))]     # frames that share bytes
    for n, (error, kw) in enumerate(refused):
        with pytest.raises(error):
            s.step(landmarks=one_lm, **kw)
        assert same(session_states(s), was), n
    assert torch.equal(feed, keep) and not misaligned.any()
    for name, order in (("rgba", "bgra"), ("rgb32", "bgr"), ("rgb24", "bgra")):
        with pytest.raises(ValueError, match="pixel_format must be 'rgb24' or 'nv12' or 'i420'|channel_order must be"):
            irfd.live(c["photos"][0], seed=7, **dict(RGB32, pixel_format=name, channel_order=order))
