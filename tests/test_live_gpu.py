"""GPU checks of ``IRFD.live`` / ``LiveSession.step`` (speak-hack_amd/live.py): with the filters off a step over a clip is
``reenact_video`` with landmarks byte for byte; with them on it is the explicit composition of ``ops.*`` calls, whatever the split of
the clip into steps; a drop-out beyond ``hold`` leaves its frames alone and restarts clean; and a step makes the library calls the
docstring names, no more.  The model and clip are those of the reenact tests: recipe weights, 128 -> 256 pixels, T = 5 BGR frames of
48 x 64, five tracked landmarks."""
import importlib

import numpy as np
import pytest
import torch

import blend_cases as BC
import landmark_ref as LR
from oracle import irfd_ref as IR
from oracle.weights_recipe import fill_state_dict

pytestmark = pytest.mark.gpu
SIZE, R, T = 128, 256, 5
TEMPLATE5 = [(44.0, 52.0), (84.0, 52.0), (64.0, 74.0), (48.0, 96.0), (80.0, 96.0)]
CONTOUR = [0, 1, 4, 3]
MATTE = dict(matte_softness=6.0, matte_grow=3.0)


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
def clip(pkg, dev):
    """Identity photo, T = 5 BGR frames of 48 x 64, five tracked landmarks per frame, every frame valid"""
    ops = pkg.ops
    rng = np.random.default_rng(23)
    true = ops.similarity_rows([(23.3 + 0.7 * t, 32.6 - 0.5 * t) for t in range(T)], [34.0 + 1.5 * t for t in range(T)],
                               [0.2 - 0.07 * t for t in range(T)], SIZE)
    lm = torch.from_numpy((LR.apply(true.numpy(), TEMPLATE5) + rng.standard_normal((T, 5, 2)) / 3).astype(np.float32)).to(dev)
    return dict(ident_u8=BC.frames(31, 56, 72, 3).to(dev), pose_u8=BC.frames(32, T, 48, 64, 3).to(dev), lm=lm)


def in_steps(session, split, frames, lm, **kw):
    out, n0 = [], 0
    for n in split:
        out.append(session.step(frames[n0:n0 + n], lm[n0:n0 + n], **kw))
        n0 += n
    assert session.frames == n0
    return torch.cat(out)


def test_filters_off_is_reenact_video_with_landmarks(irfd, pkg, clip, dev):
    c, ops = clip, pkg.ops
    keep = c["pose_u8"].clone()
    want = irfd.reenact_video(c["ident_u8"], c["pose_u8"], size=SIZE, align=ops.LandmarkAlign(c["lm"], TEMPLATE5), paste=True,
                              matte=ops.LandmarkMatte(CONTOUR, smooth=0, softness=6.0, grow=3.0), colour_match=True, seed=7, feather=4,
                              channel_order="bgr")
    s = irfd.live(c["ident_u8"], size=SIZE, template=TEMPLATE5, contour=CONTOUR, channel_order="bgr", track=None, features=None, feather=4,
                  colour_match=True, colour_decay=0.0, seed=7, **MATTE)
    got = s.step(c["pose_u8"], c["lm"])
    assert got.dtype == torch.uint8 and got.shape == (T, 48, 64, 3) and torch.equal(got, want) and s.frames == T
    assert torch.equal(c["pose_u8"], keep) and got.data_ptr() != c["pose_u8"].data_ptr() and not torch.equal(got, keep)
    # in place; and frame by frame (the noise index of frame t is t)
    video = c["pose_u8"].clone()
    s.reset()
    assert s.step(video, c["lm"], inplace=True) is video and torch.equal(video, want)
    s.reset()
    assert torch.equal(in_steps(s, [1] * T, c["pose_u8"], c["lm"]), want)
    # an emotion feed of its own goes through the same rows
    emo = BC.frames(33, T, 48, 64, 3).to(dev)
    want_e = irfd.reenact_video(c["ident_u8"], c["pose_u8"], emo, size=SIZE, align=ops.LandmarkAlign(c["lm"], TEMPLATE5), paste=True,
                                seed=7, feather=4, channel_order="bgr")
    plain = irfd.live(c["ident_u8"], size=SIZE, template=TEMPLATE5, channel_order="bgr", track=None, feather=4, seed=7)
    assert torch.equal(plain.step(c["pose_u8"], c["lm"], emotion_u8=emo), want_e) and not torch.equal(want_e, want)


def test_filters_on_is_the_composition_of_ops_in_any_split(irfd, pkg, clip, dev):
    c, ops = clip, pkg.ops
    lm = c["lm"].clone()
    lm[1] = float("nan")                                                    # the tracker lost the face for a frame: held
    lm[3:5, 3] = float("nan")                                               # and one point for two frames
    track, feats = dict(hold=2, beta=0.1), dict(hold=2, min_cutoff=2.0)
    s = irfd.live(c["ident_u8"], size=SIZE, template=TEMPLATE5, contour=CONTOUR, channel_order="bgr", track=track, features=feats, feather=4,
                  colour_match=True, colour_decay=0.8, seed=7, **MATTE)
    whole = in_steps(s, [T], c["pose_u8"], lm)
    lm_state = s.lm_state.clone()
    for split in ([2, 3], [1] * T):
        s.reset()
        assert not s.lm_state.any() and not s.feature_state.any() and not s.colour_state.any()
        assert torch.equal(in_steps(s, split, c["pose_u8"], lm), whole), split
        # the landmarks' state to the bit; the other two hang on the encoders and the decoder, whose fp32 results are those of
        # ``reenact_video`` at that chunk size: the same bytes once quantised, not the same bits before
        assert torch.equal(s.lm_state, lm_state), split
    # the explicit composition
    y_lm, wy = ops.causal_filter(lm, ops.causal_filter_state(10, 2, dev), **track)
    assert torch.isfinite(y_lm).all() and torch.equal(y_lm[1], y_lm[0])      # frame 1 is held whole
    rows = ops.similarity_from_landmarks(y_lm, TEMPLATE5, weights=wy)
    pose = ops.frames_from_u8_aligned(c["pose_u8"], SIZE, rows, channel_order="bgr")
    fi = irfd.encode(ops.frames_from_u8(c["ident_u8"], SIZE, channel_order="bgr"), "Ei")
    assert torch.equal(fi, s.fi)
    f = torch.cat([irfd.encode(pose, "Ee").view(T, -1), irfd.encode(pose, "Ep").view(T, -1)], 1)
    f, _ = ops.causal_filter(f, ops.causal_filter_state(4096, 1, dev), group=1, **feats)
    y = irfd._decode_eval(torch.cat([fi.view(1, -1).expand(T, -1), f], 1), None, "f32", "rgb", dict(seed=7, frame0=0, fixed_noise=False))
    half = rows * torch.tensor([0.5, 0.5, 1.0, 1.0], device=dev)
    matte = ops.matte_from_landmarks(y_lm, half, R, CONTOUR, softness=6.0, grow=3.0, fallback=[tuple(2.0 * v for v in TEMPLATE5[i]) for i in CONTOUR])
    sums = ops.paste_colour_sums(y, c["pose_u8"], half, matte=matte, feather=4, channel_order="bgr")
    colour = ops.colour_rows_causal(sums, torch.zeros(13, dtype=torch.float64, device=dev), 0.8)
    want = ops.frames_paste_u8_aligned(y, c["pose_u8"], half, matte=matte, colour=colour, feather=4, channel_order="bgr")
    assert torch.equal(whole, want)
    # the filters do something: the raw landmarks give other bytes
    raw = irfd.live(c["ident_u8"], size=SIZE, template=TEMPLATE5, contour=CONTOUR, channel_order="bgr", track=None, feather=4, colour_match=True,
                    colour_decay=0.8, seed=7, **MATTE)
    other = raw.step(c["pose_u8"], lm)
    assert torch.equal(other[1], c["pose_u8"][1]) and not torch.equal(whole[1], c["pose_u8"][1]) and not torch.equal(other[2], whole[2])


def test_drop_out_beyond_hold_passes_through_and_restarts_clean(irfd, pkg, clip, dev):
    c = clip
    lm = c["lm"].clone()
    lm[1:4] = float("nan")                                                  # hold = 1: frame 1 is held, frames 2 and 3 have expired
    kw = dict(size=SIZE, template=TEMPLATE5, contour=CONTOUR, channel_order="bgr", track=dict(hold=1), features=dict(hold=1), feather=4,
              colour_match=True, colour_decay=0.0, seed=7, noise="fixed", **MATTE)
    s = irfd.live(c["ident_u8"], **kw)
    got = s.step(c["pose_u8"], lm)
    assert torch.equal(got[2:4], c["pose_u8"][2:4])
    for t in (0, 1, 4):
        assert not torch.equal(got[t], c["pose_u8"][t]), t
    assert s.lm_state[:, 0].cpu().tolist() == [1.0] * 5 and s.frames == T
    fresh = irfd.live(c["ident_u8"], **kw)
    assert torch.equal(fresh.step(c["pose_u8"][4:5], lm[4:5])[0], got[4])
    # a session that never saw a face passes everything through
    blind = irfd.live(c["ident_u8"], **kw)
    assert torch.equal(blind.step(c["pose_u8"], torch.full_like(lm, float("nan"))), c["pose_u8"]) and not blind.lm_state.any()


def test_the_launches_of_a_step(irfd, pkg, clip, dev, monkeypatch):
    c, lib = clip, pkg._lib.lib()
    names = ("spk_launch_list", "spk_causal_filter", "spk_sim_fit_landmarks", "spk_matte_from_landmarks", "spk_colour_rows_causal",
             "spk_frames_paste_u8_sim_blend", "spk_frames_paste_u8_sim", "spk_paste_colour_sums_sim", "spk_paste_colour_match_sim",
             "spk_frames_u8_to_f32_sim", "spk_sim_smooth", "spk_colour_rows_window", "spk_conv2d_fwd")

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

    kw = dict(size=SIZE, template=TEMPLATE5, contour=CONTOUR, channel_order="bgr", feather=4, colour_match=True, seed=7, **MATTE)
    irfd.live(c["ident_u8"], **kw)                                          # Ei's plan for one image exists from here on
    s, calls = counted(lambda: irfd.live(c["ident_u8"], **kw))
    assert calls == {"spk_launch_list": 1}, calls                           # Ei, once
    s.step(c["pose_u8"][:1], c["lm"][:1])                                   # the plans of one frame exist from here on
    per_step = {"spk_launch_list": 3, "spk_causal_filter": 1, "spk_sim_fit_landmarks": 1, "spk_frames_u8_to_f32_sim": 1,
                "spk_matte_from_landmarks": 1, "spk_paste_colour_sums_sim": 1, "spk_colour_rows_causal": 1, "spk_frames_paste_u8_sim_blend": 1}
    for t in (1, 2):
        _, calls = counted(lambda: s.step(c["pose_u8"][t:t + 1], c["lm"][t:t + 1]))
        assert calls == per_step, calls                                     # Ee, Ep, Gd; no Ei, no window, no smoothing
    both = irfd.live(c["ident_u8"], features={}, **kw)
    both.step(c["pose_u8"][:1], c["lm"][:1])
    _, calls = counted(lambda: both.step(c["pose_u8"][1:2], c["lm"][1:2], emotion_u8=c["pose_u8"][2:3]))
    assert calls == dict(per_step, spk_causal_filter=2, spk_frames_u8_to_f32_sim=2), calls
    bare = irfd.live(c["ident_u8"], size=SIZE, template=TEMPLATE5, channel_order="bgr", track=None, seed=7)
    bare.step(c["pose_u8"][:1], c["lm"][:1])
    _, calls = counted(lambda: bare.step(c["pose_u8"][1:2], c["lm"][1:2]))
    assert calls == {"spk_launch_list": 3, "spk_sim_fit_landmarks": 1, "spk_frames_u8_to_f32_sim": 1, "spk_frames_paste_u8_sim": 1}, calls
