"""GPU checks of the two kernels a live room adds.  ``spk_noise_fill_rows`` (csrc/noise.hip): every batch row is the row the existing
fill makes from that row's (seed, frame), bit for bit, on the float4 and on the scalar-tail path; the tables' values reach the
counter as ``spk_noise_bits_host`` maps its arguments; a rows-seeded ``DecoderPlan`` is the seeded plan where the tables say what
the seeded plan would.  ``spk_colour_rows_causal_feeds`` (csrc/causal_filter.hip): rows and states are those of S separate
``ops.colour_rows_causal`` calls, bit for bit, in any split of the frames, with S = 22 crossing the 21 feeds one wave holds.

Every comparison between device results is equality of bits.  The one comparison with fp64 -- block 0 of a row against the
Box-Muller of tests/philox_ref.py on the host routine's bits -- uses the bound of tests/test_noise_gpu.py for the same arithmetic
(4 x the largest deviation measured there, 2.356e-6; a wrong bit gives an error of order 1)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import blend_cases as BC
import live_room_ref as RR
import philox_ref as PR
from oracle.weights_recipe import fill_state_dict, recipe_input

pytestmark = pytest.mark.gpu
BOUND = 4 * 5.890e-7
SEEDS, FRAMES = (7, 7, 2 ** 63 + 3), (0, 5, 2 ** 32 + 1)
# (hw, dst offset in floats from a 16-byte boundary): the float4 path, and the scalar path with a tail
NOISE_CASES = [((16, 64), 0), ((16, 6), 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("speak-hack_amd")
    p._lib.lib()
    return p


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def guarded(dev, nbytes, guard, dtype):
    raw = torch.full((guard + nbytes + guard,), 0xA5, dtype=torch.uint8, device=dev)
    return raw, raw[guard:guard + nbytes].view(dtype)


def intact(raw, nbytes, guard):
    return bool(torch.all(raw[:guard] == 0xA5)) and bool(torch.all(raw[guard + nbytes:] == 0xA5))


def fill_rows(pkg, dev, hw, B, seeds, frames, offset=0):
    """-> dst [B * sum(hw)] filled by the rows kernel, ``offset`` floats past a 16-byte boundary, with the guard floats checked"""
    n = B * sum(hw)
    store = torch.full((4 + offset + n + 4,), float("nan"), device=dev)
    assert store.data_ptr() % 16 == 0
    dst = store[4 + offset:4 + offset + n]
    pkg.ops.noise_fill_rows(dst, hw, B, pkg.ops.seed_rows(seeds, dev), torch.tensor(frames, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    assert torch.isnan(store[:4 + offset]).all() and torch.isnan(store[4 + offset + n:]).all(), "wrote outside dst"
    assert torch.isfinite(dst).all()
    return dst


@pytest.mark.parametrize("hw,offset", NOISE_CASES, ids=["float4", "scalar tail"])
def test_noise_rows_are_the_rows_of_the_existing_fill(pkg, dev, hw, offset, monkeypatch):
    ops, B = pkg.ops, 3
    got = fill_rows(pkg, dev, hw, B, SEEDS, FRAMES, offset)
    layers = [t.view(B, v) for t, v in zip(got.split([B * v for v in hw]), hw)]
    lib = pkg._lib.lib()
    for b, (seed, frame) in enumerate(zip(SEEDS, FRAMES)):
        one = ops.noise_fill(torch.empty(sum(hw), device=dev), hw, 1, seed, frame0=frame)
        for l, (mine, theirs) in enumerate(zip(layers, one.split(list(hw)))):
            assert same_bits(mine[b], theirs), (b, l)
        # block 0 of the row: the host routine's bits of the TABLE value (two's complement), through philox_ref's Box-Muller
        pattern = int(ops.seed_rows([seed])[0])
        bits = (ctypes.c_uint32 * 4)()
        assert lib.spk_noise_bits_host(ctypes.c_uint64(pattern & (2 ** 64 - 1)), frame, 0, 0, bits) == 0
        assert list(bits) == [int(v) for v in PR.noise_bits(seed, frame, 0, np.uint64(0))]
        with monkeypatch.context() as mp:
            mp.setattr(PR, "noise_bits", lambda *a, host=np.array([list(bits)], dtype=np.uint64): host)
            want = PR.noise_plane(seed, frame, 0, 4)
        err = float(np.abs(layers[0][b, :4].cpu().numpy().astype(np.float64) - want).max())
        print(f"noise rows hw={hw} row {b}: block 0, max |device - fp64 of the host bits| = {err:.3e} (bound {BOUND:.3e})")
        assert err <= BOUND
    assert same_bits(layers[0][0], layers[0][0].clone()) and not same_bits(layers[0][0], layers[0][1])     # one seed, two frames
    # equal seeds and consecutive frames: the whole buffer is the stepped fill's
    f = 2 ** 32 - 1                                                       # the carry into the frame's high word lies inside the batch
    stepped = ops.noise_fill(torch.empty(B * sum(hw), device=dev), hw, B, 11, frame0=f)
    assert same_bits(fill_rows(pkg, dev, hw, B, (11,) * B, (f, f + 1, f + 2), offset), stepped)


def test_decoder_noise_rows_is_decoder_noise(pkg, dev):
    ops = pkg.ops
    shapes = [(3, 1, 4, 4), (3, 1, 8, 8), (3, 1, 8, 8), (3, 1, 16, 16)]
    f = 40
    rows = ops.decoder_noise_rows(shapes, ops.seed_rows([5] * 3, dev), torch.tensor([f, f + 1, f + 2], device=dev))
    want = ops.decoder_noise(shapes, 5, frame0=f, device=dev)
    assert len(rows) == len(want) and all(same_bits(a, b) for a, b in zip(rows, want))
    assert all(a.data_ptr() + a.numel() * 4 == b.data_ptr() for a, b in zip(rows, rows[1:]))      # views of one flat buffer
    with pytest.raises(pkg._lib.SpkError, match="overlaps"):              # the library's own refusal reaches the caller
        flat = torch.zeros(3 * 16 + 8, device=dev)
        table = flat[46:52].view(torch.int64)                              # bytes [184, 208): the last 8 of dst are the table's first
        ops.noise_fill_rows(flat[:3 * 16], (16,), 3, table, table.clone())


@pytest.fixture(scope="module")
def syn32(pkg, dev):
    s = pkg.SynthesisNetwork(resolution=32).eval()
    s.load_state_dict(fill_state_dict(s.state_dict(), prefix="noise.syn32."))
    return s.to(dev)


def test_rows_seeded_plan_is_the_seeded_plan(pkg, dev, syn32):
    L, PL, ops = pkg._lib, importlib.import_module("speak-hack_amd.plan"), pkg.ops
    B, f = 3, 2
    w = recipe_input("noise.syn32.w", (B, syn32.num_layers, 512)).to(dev)
    rows_plan, seeded, plain = PL.DecoderPlan(syn32, B, dev, seeded="rows"), PL.DecoderPlan(syn32, B, dev, seeded=True), PL.DecoderPlan(syn32, B, dev)
    assert rows_plan.ops[0][0] == L.OP_NOISE_FILL_ROWS == 14 and [k for k, _ in rows_plan.ops].count(L.OP_NOISE_FILL_ROWS) == 1
    assert seeded.ops[0][0] == L.OP_NOISE_FILL and len(seeded.ops) == len(rows_plan.ops) == len(plain.ops) + 1
    assert not rows_plan.seeded and rows_plan.seed_rows and seeded.seeded and not seeded.seed_rows and not plain.seeded and not plain.seed_rows
    seeds, frames = ops.seed_rows([7] * B, dev), torch.tensor([f, f + 1, f + 2], device=dev)
    with torch.no_grad():
        rng = torch.cuda.get_rng_state(dev)
        got = rows_plan.run(w, seed_rows=seeds, frame_rows=frames)
        assert torch.equal(torch.cuda.get_rng_state(dev), rng)             # the device generator stays where it was
        want = seeded.run(w, seed=7, frame0=f)
        assert got.shape == (B, 3, 32, 32) and same_bits(got, want)
        # the tables are patched per run and read on the device: other rows, other frames
        mixed_seeds, mixed_frames = ops.seed_rows(SEEDS, dev), torch.tensor(FRAMES, device=dev)
        mixed = rows_plan.run(w, seed_rows=mixed_seeds, frame_rows=mixed_frames)
        assert same_bits(mixed, plain.run(w, ops.decoder_noise_rows(syn32.noise_shapes(B), mixed_seeds, mixed_frames)))
        assert same_bits(mixed[0], seeded.run(w, seed=7, frame0=0)[0]) and not same_bits(mixed[1], want[1])
        frames.add_(1)                                                      # advanced on the device, same pointer
        assert same_bits(rows_plan.run(w, seed_rows=seeds, frame_rows=frames), seeded.run(w, seed=7, frame0=f + 1))
        # each form runs its own calls only
        noises = ops.decoder_noise(syn32.noise_shapes(B), 1, device=dev)
        for plan, args, kw in ((plain, (w,), dict(seed_rows=seeds, frame_rows=frames)), (seeded, (w,), dict(seed_rows=seeds, frame_rows=frames)),
                               (seeded, (w,), dict(seed=7, seed_rows=seeds, frame_rows=frames)), (rows_plan, (w,), {}),
                               (rows_plan, (w,), dict(seed=7)), (rows_plan, (w, noises), {}), (rows_plan, (w,), dict(seed_rows=seeds)),
                               (rows_plan, (w,), dict(seed=7, seed_rows=seeds, frame_rows=frames)),
                               (rows_plan, (w, noises), dict(seed_rows=seeds, frame_rows=frames)),
                               (rows_plan, (w,), dict(seed_rows=seeds[:2], frame_rows=frames)),
                               (rows_plan, (w,), dict(seed_rows=seeds, frame_rows=frames.to(torch.int32)))):
            with pytest.raises(ValueError):
                plan.run(*args, **kw)
        with pytest.raises(L.SpkError):
            rows_plan.run(w, seed_rows=seeds.cpu(), frame_rows=frames)
        with pytest.raises(ValueError):
            PL.DecoderPlan(syn32, B, dev, seeded="columns")
        assert same_bits(seeded.run(w, seed=1), plain.run(w, noises))       # and the two older forms run as before


# ---- the feeds' colour rows -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean_sums(pkg, dev):
    """[7,13]: ``paste_colour_sums`` on the four frames of blend case "generic" and the three of "gain cap", which all take part;
    and the rows of ``paste_colour_match`` on them"""
    a, b = BC.case("generic"), BC.case("gain cap")
    x, bg, rows = (torch.cat([a[k], b[k]]).to(dev) for k in ("x", "bg", "rows"))
    sums = pkg.ops.paste_colour_sums(x, bg, rows)
    assert sums.shape == (RR.N, 13) and (sums[:, 0] > BC.MIN_WEIGHT).all() and torch.isfinite(sums).all()
    return sums, pkg.ops.paste_colour_match(x, bg, rows)


def feed_sums(clean, S):
    """[7,S,13]: feed s sees the clip rotated by s frames and weighed 1 + s / 8 times (sums are linear: still sums of a clip), with
    the participation pattern of ``live_room_ref`` in it"""
    feeds = torch.stack([torch.roll(clean, s, 0) * (1.0 + s / 8.0) for s in range(S)], 1)
    return RR.spoil(feeds)


@pytest.mark.parametrize("S", [1, 4, 22])
def test_colour_feeds_are_separate_calls_bit_for_bit(pkg, dev, clean_sums, S):
    ops, N = pkg.ops, RR.N
    clean, match_rows = clean_sums
    sums = feed_sums(clean, S)
    low, nan, ok = RR.pattern(S)
    assert sums.shape == (N, S, 13) and 0.0 < float(sums[2, low, 0]) < BC.MIN_WEIGHT and bool(torch.isnan(sums[5, nan, 7]))
    for decay in RR.DECAYS:
        raw_s, state = guarded(dev, S * 13 * 8, 256, torch.float64)
        state = state.view(S, 13).zero_()
        raw_r, out = guarded(dev, N * S * 24, 256, torch.float32)
        got = ops.colour_rows_causal_feeds(sums, state, decay, out=out.view(N, S, 3, 2))
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and intact(raw_s, S * 104, 256) and intact(raw_r, N * S * 24, 256)
        for s in range(S):
            one_state = torch.zeros(13, dtype=torch.float64, device=dev)
            one = ops.colour_rows_causal(sums[:, s].contiguous(), one_state, decay)
            assert same_bits(got[:, s], one) and same_bits(state[s], one_state), (decay, s)
        assert same_bits(got[2, low], got[1, low]) and same_bits(got[5, nan], got[4, nan])       # a rejected frame repeats the previous row
        if S > 1:
            assert not same_bits(got[2, ok], got[1, ok]) and not same_bits(got[:, 0], got[:, 1])
        for split in ([3, 4], [1] * N):
            st, parts, n0 = torch.zeros(S, 13, dtype=torch.float64, device=dev), [], 0
            for n in split:
                parts.append(ops.colour_rows_causal_feeds(sums[n0:n0 + n].contiguous(), st, decay))
                n0 += n
            assert same_bits(torch.cat(parts), got) and same_bits(st, state), (decay, split)
    if S == 1:                                                             # the feed of a room of one: the existing entry on clean frames too
        st1, st = torch.zeros(1, 13, dtype=torch.float64, device=dev), torch.zeros(13, dtype=torch.float64, device=dev)
        assert same_bits(ops.colour_rows_causal_feeds(clean.view(N, 1, 13), st1, 0.8)[:, 0], ops.colour_rows_causal(clean, st, 0.8))
        assert same_bits(st1[0], st)
    else:                                                                  # decay = 0 on the clean feed: the rows of the match
        st = torch.zeros(S, 13, dtype=torch.float64, device=dev)
        assert ok == 0 and same_bits(ops.colour_rows_causal_feeds(sums, st, 0.0)[:, 0], match_rows)
        assert same_bits(st[0], clean[N - 1])
