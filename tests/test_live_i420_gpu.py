"""GPU checks of ``IRFD.live`` / ``IRFD.live_room`` with ``pixel_format="i420"`` (speak-hack_amd/live.py over csrc/frame_sim_i420.hip
and csrc/frame_table_i420.hip).  The criterion is the NV12 session / room of tests/test_live_nv12_gpu.py on the INTERLEAVED feeds: a
session and a room on I420 feeds -- a triple of pitched planes, one packed stacked tensor, a list of three surfaces of three sizes
one of which is a region of interest -- give the same Y, U and V bytes and the same filter, feature and colour states, bit for bit;
any split of the frames gives the same bytes; a feed lost beyond ``hold`` gets its surface back untouched; a tick on a list calls the
three ``_i420_sim_table`` entry points and no NV12 one; every refusal comes before a launch.  Model, template, settings, seeds, feeds
and layout are that file's (S = 3, T = 3, SIZE 128), imported from it."""
import pytest
import torch

from test_live_nv12_gpu import (FEATS, LAYOUT, NV12, PAD, S, SEEDS, T, dev, feeds, irfd, pkg, same_states, states, surface,  # noqa: F401
                                view)

pytestmark = pytest.mark.gpu
I420 = dict(NV12, pixel_format="i420")


def pitched(plane, pad):
    """A copy of a chroma plane [..., rows, width] at row pitch ``width + pad`` from an odd offset of its allocation, padding PAD"""
    *lead, rows, width = plane.shape
    n = 1
    for k in lead:
        n *= k
    raw = torch.full((1 + n * rows * (width + pad),), PAD, dtype=torch.uint8, device=plane.device)
    out = raw[1:].view(*lead, rows, width + pad)[..., :width]
    out.copy_(plane)
    return out


def triple(pkg, nv12, copy=True):
    """What ``nv12_planes`` takes -> the I420 surface with the same bytes: the Y plane (a copy with its pitch, or the view itself) and
    U and V planes of their own, at odd pitches that differ, from odd addresses"""
    y, uv = pkg.ops.nv12_planes(nv12)
    if nv12.dim() == 2 if isinstance(nv12, torch.Tensor) else nv12[0].dim() == 2:
        y, uv = y[0], uv[0]
    if copy:
        keep = torch.full((*y.shape[:-1], y.size(-1) + 16), PAD, dtype=torch.uint8, device=y.device)[..., :y.size(-1)]
        keep.copy_(y)
        y = keep
    return y, pitched(uv[..., 0], 1), pitched(uv[..., 1], 3)


def packed(t):
    """A triple of planes [N,...] -> one contiguous packed tensor [N,3H/2,W]"""
    y, u, v = t
    return torch.cat([p.flatten(1) for p in (y, u, v)], 1).view(y.size(0), 3 * y.size(1) // 2, y.size(2))


def same_bytes(pkg, i420, nv12):
    """An I420 result and an NV12 result hold the same Y, U and V bytes"""
    (y, u, v), (ny, nuv) = pkg.ops.i420_planes(i420), pkg.ops.nv12_planes(nv12)
    return torch.equal(y, ny) and torch.equal(u, nuv[..., 0]) and torch.equal(v, nuv[..., 1])


# ---- a session ------------------------------------------------------------------------------------------------------------------
def test_a_session_is_the_nv12_session_on_the_interleaved_feed(irfd, pkg, feeds, dev):
    c = feeds
    surf, lm = c["one"], c["one_lm"].clone()
    lm[1, 3] = float("nan")                                                 # one point lost for a frame: held
    theirs = irfd.live(c["photos"][0], features=FEATS, seed=7, **NV12)
    want = theirs.step(surf, lm)
    mine = irfd.live(c["photos"][0], features=FEATS, seed=7, **I420)
    feed = triple(pkg, surf)
    assert feed[1].data_ptr() % 2 == 1 and feed[1].stride(1) % 2 == 1 and feed[1].stride(1) != feed[2].stride(1)
    keep = [p.clone() for p in feed]
    whole = mine.step(feed, lm)
    assert whole.dtype == torch.uint8 and whole.shape == (T, 72, 64) and whole.is_contiguous() and mine.frames == T
    assert same_bytes(pkg, whole, want) and all(torch.equal(a, b) for a, b in zip(feed, keep))
    was = states(mine)
    assert same_states(was, states(theirs)) and all(bool(t.any()) for t in was)               # filter, feature and colour states, bit for bit
    for t in range(T):
        assert not same_bytes(pkg, whole[t], surf[t]), t                    # a frame that was pasted differs from its input
    # any split of the frames, and the packed tensor form
    mine.reset()
    split = torch.cat([mine.step(tuple(p[:1] for p in feed), lm[:1]), mine.step(tuple(p[1:] for p in feed), lm[1:])])
    assert torch.equal(split, whole) and same_states(states(mine), was)
    mine.reset()
    assert torch.equal(mine.step(packed(feed), lm), whole) and same_states(states(mine), was)
    # in place on the triple: the triple, with the same bytes, its padding untouched
    mine.reset()
    assert mine.step(feed, lm, inplace=True) is feed and torch.equal(packed(feed), whole)
    assert all(bool((p._base.view(-1)[1:].view(T, p.size(1), -1)[:, :, p.size(2):] == PAD).all()) for p in feed[1:])
    # another colour is another result; the emotion feed is taken in the same form
    wide = irfd.live(c["photos"][0], features=FEATS, seed=7, **dict(I420, standard="bt709", full_range=True))
    assert not torch.equal(wide.step(packed(keep), lm), whole)
    emo = surface(35, T, 48, 64, dev)
    mine.reset(), theirs.reset()
    assert same_bytes(pkg, mine.step(packed(keep), lm, emotion_u8=triple(pkg, emo)), theirs.step(surf, lm, emotion_u8=emo))
    # lost for longer than hold: the surface comes back byte for byte; the held frame is pasted
    gone = c["one_lm"].clone()
    gone[1:] = float("nan")
    short = irfd.live(c["photos"][0], seed=7, **dict(I420, track=dict(hold=1), features=dict(hold=1)))
    out = short.step(packed(keep), gone)
    assert torch.equal(out[2], packed(keep)[2]) and not torch.equal(out[1], packed(keep)[1]) and not torch.equal(out[0], packed(keep)[0])


# ---- a room ---------------------------------------------------------------------------------------------------------------------
def test_a_room_over_one_stacked_tensor_is_the_nv12_room(irfd, pkg, feeds):
    c = feeds
    mine = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **I420)
    theirs = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **NV12)
    for t in range(T):
        tick = packed(triple(pkg, c["same"][t], copy=False))
        assert tick.is_contiguous() and tick.shape == (S, 72, 64)
        keep = tick.clone()
        got, want = mine.step(tick, c["same_lm"][t]), theirs.step(c["same"][t], c["same_lm"][t])
        assert got.shape == (S, 72, 64) and torch.equal(tick, keep) and same_bytes(pkg, got, want), t
        assert same_states(states(mine), states(theirs)), t
        assert all(not torch.equal(got[s], tick[s]) for s in range(S)), t   # pasted in every tick: the lost frame of feed 1 is held
    assert mine.frames.tolist() == [T] * S
    # in place on one tensor returns the tensor; on a triple of planes, the triple
    again = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **I420)
    first = again.step(packed(triple(pkg, c["same"][0])), c["same_lm"][0])
    tick = first.clone().copy_(packed(triple(pkg, c["same"][0])))
    again.reset()
    assert again.step(tick, c["same_lm"][0], inplace=True) is tick and torch.equal(tick, first)
    planes = triple(pkg, c["same"][0])
    again.reset()
    assert again.step(planes, c["same_lm"][0], inplace=True) is planes and torch.equal(packed(planes), first)


def rois(pkg, wholes):
    """This tick's whole NV12 surfaces [3H/2,W] per feed -> (the NV12 surfaces as the NV12 room takes them, the I420 surfaces: whole
    planes de-interleaved into allocations of their own, the region of interest a triple of views of them; the whole I420 planes)"""
    nv12, mine, held = [], [], []
    for s, whole in enumerate(wholes):
        bh, bw, y0, x0, h, w = LAYOUT[s]
        y, u, v = triple(pkg, whole)
        held.append((y, u, v))
        nv12.append(view(whole, s))
        mine.append((y[y0:y0 + h, x0:x0 + w], u[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], v[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2]))
    return nv12, mine, held


def test_feeds_of_three_sizes_are_the_nv12_room(irfd, pkg, feeds):
    c = feeds
    mine = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **I420)
    theirs = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **NV12)
    for t in range(T):
        wholes = [c["mixed"][s][t].clone() for s in range(S)]
        before = [w.clone() for w in wholes]
        nv12, surfaces, held = rois(pkg, wholes)
        assert tuple(surfaces[1][0].shape) == (40, 52) and surfaces[1][1].stride(0) == 31 and tuple(surfaces[1][1].shape) == (20, 26)
        got = mine.step(surfaces, c["mixed_lm"][t], inplace=True)
        assert got is surfaces
        theirs.step(nv12, c["mixed_lm"][t], inplace=True)
        assert same_states(states(mine), states(theirs)), t
        for s in range(S):
            # the whole planes, region and surroundings: the bytes of the NV12 room's whole surface
            assert same_bytes(pkg, held[s], wholes[s]), (t, s)
            assert not torch.equal(wholes[s], before[s]), (t, s)
    assert mine.frames.tolist() == [T] * S
    # cloned: a list of new packed tensors, the caller's planes untouched; a PlanarTable is taken as the list it was made from
    wholes = [c["mixed"][s][0].clone() for s in range(S)]
    nv12, surfaces, held = rois(pkg, wholes)
    keep = [tuple(p.clone() for p in h) for h in held]
    room = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **I420)
    out = room.step(surfaces, c["mixed_lm"][0])
    assert isinstance(out, list) and [tuple(o.shape) for o in out] == [(3 * h // 2, w) for *_, h, w in LAYOUT] and all(o.is_contiguous() for o in out)
    assert all(torch.equal(a, b) for h, k in zip(held, keep) for a, b in zip(h, k))
    table = pkg.ops.PlanarTable(surfaces)
    room.reset()
    again = room.step(table, c["mixed_lm"][0], inplace=True)
    assert all(a is b for a, b in zip(again, table.surfaces))
    assert all(torch.equal(packed(tuple(p.unsqueeze(0) for p in surf))[0], o) for surf, o in zip(surfaces, out))


def test_a_tick_on_a_list_calls_the_i420_table_entry_points(irfd, pkg, feeds, monkeypatch):
    c, lib = feeds, pkg._lib.lib()
    mine = ("spk_frames_i420_to_f32_sim_table", "spk_paste_colour_sums_i420_sim_table", "spk_frames_paste_i420_sim_table")
    names = [n for n in pkg._lib._PROTOTYPES if "frames_" in n or "paste_colour_" in n]         # every entry point of the video edge
    assert set(mine) <= set(names) and sum("nv12" in n for n in names) >= 11
    calls = dict.fromkeys(names, 0)

    def counting(n, real):
        def f(*a):
            calls[n] += 1
            return real(*a)
        return f

    room = irfd.live_room(c["photos"], seed=7, **I420)
    _, first, _ = rois(pkg, [c["mixed"][s][0].clone() for s in range(S)])
    room.step(first, c["mixed_lm"][0], inplace=True)
    _, surfaces, _ = rois(pkg, [c["mixed"][s][1].clone() for s in range(S)])
    for n in names:
        monkeypatch.setattr(lib, n, counting(n, getattr(lib, n)))
    room.step(surfaces, c["mixed_lm"][1], inplace=True)
    monkeypatch.undo()
    assert {n: k for n, k in calls.items() if k} == dict.fromkeys(mine, 1)


def test_refusals_leave_the_states_and_the_buffers_as_they_were(irfd, pkg, feeds, dev):
    c, L = feeds, pkg._lib
    room = irfd.live_room(c["photos"], features=FEATS, seed=SEEDS, **I420)
    lm = c["mixed_lm"][0]
    room.step(rois(pkg, [c["mixed"][s][0].clone() for s in range(S)])[1], lm, inplace=True)   # a room in mid-call: its states are not empty
    _, surfaces, held = rois(pkg, [c["mixed"][s][1].clone() for s in range(S)])
    before, was = [tuple(p.clone() for p in h) for h in held], states(room)
    assert all(bool(t.any()) for t in was)
    wide = torch.zeros(72, 128, dtype=torch.uint8, device=dev)
    y2, u2, v2 = surfaces[2]
    side = torch.zeros(28, 72, dtype=torch.uint8, device=dev)
    refused = [(ValueError, dict(frames_u8=surfaces[:2])),                                      # wrong list length
               (ValueError, dict(frames_u8=surfaces + surfaces[:1])),
               (ValueError, dict(frames_u8=[surfaces[0], None, surfaces[2]])),                  # a None element
               (ValueError, dict(frames_u8=[surfaces[0], surfaces[1], (y2[:, :71], u2, v2)])),  # an odd size
               (ValueError, dict(frames_u8=[surfaces[0], surfaces[1], (y2, u2.float(), v2)])),  # wrong dtype
               (ValueError, dict(frames_u8=[surfaces[0], surfaces[1], (y2, u2)])),              # a pair is no I420 surface
               (ValueError, dict(frames_u8=[surfaces[0], surfaces[1], c["mixed"][2][1][:, :70]])),      # a packed surface that is not contiguous
               (L.SpkError, dict(frames_u8=[tuple(p.cpu() for p in surfaces[0]), surfaces[1], surfaces[2]])),      # wrong device
               (ValueError, dict(frames_u8=[(wide[:48, ::2], *surfaces[0][1:]), surfaces[1], surfaces[2]])),        # a pixel stride
               (ValueError, dict(frames_u8=surfaces, emotion_u8=[surfaces[2], surfaces[1], surfaces[0]])),         # sizes differ feed by feed
               (ValueError, dict(frames_u8=surfaces, emotion_u8=surfaces[:2])),
               (L.SpkError, dict(frames_u8=[surfaces[0], surfaces[1], (y2, side[:, :36], side[:, 36:])], inplace=True)),   # chroma halves side by side
               (L.SpkError, dict(frames_u8=[surfaces[0], surfaces[0], surfaces[2]], inplace=True))]                # elements that share bytes
    for n, (error, kw) in enumerate(refused):
        with pytest.raises(error):
            room.step(landmarks=lm, **kw)
        assert same_states(states(room), was), n
    assert all(torch.equal(a, b) for h, k in zip(held, before) for a, b in zip(h, k)) and not side.any()
    # what was refused in place is fine where every surface is cloned first, and the room goes on
    out = room.step([surfaces[0], surfaces[0], surfaces[2]], lm)
    assert len(out) == S and out[0] is not out[1] and all(torch.equal(a, b) for h, k in zip(held, before) for a, b in zip(h, k))
    assert not same_states(states(room), was)
    # a session: the same kinds, refused before the filters have moved; and the names that are not the format's
    s = irfd.live(c["photos"][0], features=FEATS, seed=7, **I420)
    feed, one_lm = triple(pkg, c["one"]), c["one_lm"]
    s.step(feed, one_lm)
    was, keep = states(s), [p.clone() for p in feed]
    stack = torch.zeros(2, 24, 32, dtype=torch.uint8, device=dev)
    y, u, v = feed
    refused = [(ValueError, dict(frames_u8=c["one"])),                                          # a packed tensor with a pitch: give a triple
               (ValueError, dict(frames_u8=packed(feed)[:, :71])),                              # rows that are not 3H/2
               (ValueError, dict(frames_u8=packed(feed).float())),
               (ValueError, dict(frames_u8=(y, u))),                                            # an NV12-style pair
               (ValueError, dict(frames_u8=(y, u, v[:, :, :31]))),
               (L.SpkError, dict(frames_u8=tuple(p.cpu() for p in feed))),
               (ValueError, dict(frames_u8=feed, emotion_u8=tuple(p[:2] for p in feed))),
               (L.SpkError, dict(frames_u8=feed, emotion_u8=tuple(p.cpu() for p in feed))),
               (L.SpkError, dict(frames_u8=(y, stack[:1].expand(T, 24, 32), v), inplace=True))]  # frames that share bytes
    for n, (error, kw) in enumerate(refused):
        with pytest.raises(error):
            s.step(landmarks=one_lm, **kw)
        assert same_states(states(s), was), n
    assert all(torch.equal(a, b) for a, b in zip(feed, keep)) and not stack.any()
    for name in ("yuv420", "yuv420p"):
        with pytest.raises(ValueError, match="pixel_format must be 'rgb24' or 'nv12'"):
            irfd.live(c["photos"][0], seed=7, **dict(I420, pixel_format=name))
