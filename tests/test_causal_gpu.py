"""GPU checks of the causal filters (csrc/causal_filter.hip) against the numpy fp64 model of tests/causal_ref.py.

Bounds.  FILTER: ``|y - ref| <= 2^-22 max(1, |ref|)``: kernel and model run the same fp64 recursion, which they round differently
(the kernel contracts ``a x + (1 - a) xh`` into an fma) by a few 2^-53 a frame, relative to values of 1 ... 100; the one rounding of
``xh`` to fp32 is 2^-24 relative, and 2^-22 leaves a factor of four for the ulp at a binade's top and the contraction.  NaNs are at
exactly the model's places, ``wy`` and the state's ``k`` are exact (weights and counters are copied, not computed), the rest of the
state is within 1e-12 relative: nine frames of roundings at 2^-53, amplified by the cancellation in ``x - xh`` (both of the order of
100, their difference of the order of 1, so 100 x) -- some 1e-13.  COLOUR ROWS: the project's row bounds, ``|g - g_ref| / g_ref <=
2^-22`` and ``|o - o_ref| <= 2^-15`` (tests/test_colour_window_gpu.py), with the model fed the sums the device made.  Every split of
a call is ``torch.equal`` to the whole call: the state is the unrounded recursion."""
import importlib

import numpy as np
import pytest
import torch

import blend_cases as BC
import causal_ref as CR

pytestmark = pytest.mark.gpu
TOL_Y, TOL_STATE = 2.0 ** -22, 1e-12
SPLITS = ([9], [4, 5], [1] * 9)


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


# name of the series, how the weights are passed ("frames": [N,G], stride G; "one": [G], stride 0; None)
FILTER_CASES = [("landmarks", "frames"), ("landmarks", "one"), ("landmarks", None), ("features", None), ("triples", None)]
ONE_SET = np.array([1.0, 0.5, 2.0, float("nan"), 0.0], dtype=np.float32)      # stride 0: point 3 has a NaN weight, point 4 a zero one


@pytest.mark.parametrize("name,how", FILTER_CASES)
def test_filter_against_the_model_and_in_splits(pkg, dev, name, how):
    ops = pkg.ops
    x, w, group = CR.series(name)
    w = {"frames": w, "one": ONE_SET, None: None}[how]
    N, D = x.shape
    G = D // group
    kw = dict(group=group, hold=2)
    ref_state = CR.empty_state(D, group)
    ref_y, ref_wy = CR.causal_filter(x, ref_state, w, **kw)
    xd, wd = torch.from_numpy(np.array(x)).to(dev), None if w is None else torch.from_numpy(np.array(w)).to(dev)
    # the whole call, between guard bytes
    raw_s, state = guarded(dev, G * (2 + 2 * group) * 8, 256, torch.float64)
    state = state.view(G, 2 + 2 * group).zero_()
    raw_y, out = guarded(dev, N * D * 4, 256, torch.float32)
    y, wy = ops.causal_filter(xd, state, weights=wd, out=out.view(N, D), **kw)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr() and intact(raw_s, state.numel() * 8, 256) and intact(raw_y, N * D * 4, 256)
    assert y.dtype == torch.float32 and tuple(y.shape) == (N, D) and wy.dtype == torch.float32 and tuple(wy.shape) == (N, G)
    got, got_wy, got_state = y.cpu().numpy().astype(np.float64), wy.cpu().numpy().astype(np.float64), state.cpu().numpy()
    nan = np.isnan(ref_y)
    assert (np.isnan(got) == nan).all() and nan.any() and (~nan).any()      # NaNs at exactly the model's places
    err = np.abs(got - ref_y)[~nan] / np.maximum(1.0, np.abs(ref_y[~nan]))
    assert (got_wy == ref_wy).all()                                         # exact
    assert (got_state[:, 0] == ref_state[:, 0]).all()                       # k: exact
    rest, ref_rest = got_state[:, 1:], ref_state[:, 1:]
    nz = ref_rest != 0
    err_s = np.abs(rest[nz] - ref_rest[nz]) / np.abs(ref_rest[nz])
    print(f"filter, {name} weights={how}: largest |y - ref| / max(1, |ref|) = {err.max():.3e} (bound {TOL_Y:.3e}); state: largest relative "
          f"deviation {err_s.max():.3e} (bound {TOL_STATE:.0e}); k = {sorted(set(got_state[:, 0].tolist()))}")
    assert err.max() <= TOL_Y
    assert err_s.max() <= TOL_STATE and (rest[~nz] == 0).all()
    # every split gives the bits of the whole call -- on a copy, and in place
    for split in SPLITS[1:]:
        for inplace in (False, True):
            st, ys, wys, n0 = ops.causal_filter_state(D, group, dev), [], [], 0
            for n in split:
                part = xd[n0:n0 + n].clone()
                yp, wyp = ops.causal_filter(part, st, weights=wd if wd is None or wd.dim() == 1 else wd[n0:n0 + n], out=part if inplace else None,
                                            **kw)
                assert (yp.data_ptr() == part.data_ptr()) == inplace
                ys.append(yp), wys.append(wyp)
                n0 += n
            assert same_bits(torch.cat(ys), y) and same_bits(torch.cat(wys), wy) and same_bits(st, state), (split, inplace)
    # [N,K,2] landmarks are [N,2K] signals
    if name == "landmarks":
        y3, wy3 = ops.causal_filter(xd.view(N, G, 2), ops.causal_filter_state(D, 2, dev), weights=wd, **kw)
        assert tuple(y3.shape) == (N, G, 2) and same_bits(y3.view(N, D), y) and same_bits(wy3, wy)


def test_filter_drop_out_pattern(pkg, dev):
    """The pattern of ``causal_ref.series('landmarks')`` at hold = 2, read off the device's result: point 1 bridged over 2 frames,
    point 2 held, held, NaN, NaN and restarted with the sample itself, point 3 never valid, point 4 without a weight in frames 1, 6."""
    x, w, _ = CR.series("landmarks")
    xd, wd = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(w)).to(dev)
    state = pkg.ops.causal_filter_state(10, 2, dev)
    y, wy = pkg.ops.causal_filter(xd, state, weights=wd, hold=2)
    y, wy, k = y.view(9, 5, 2).cpu(), wy.cpu(), state[:, 0].cpu().tolist()
    assert torch.equal(y[3, 1], y[2, 1]) and torch.equal(y[4, 1], y[2, 1]) and wy[3:5, 1].tolist() == [float(w[2, 1])] * 2
    assert torch.equal(y[2, 2], y[1, 2]) and torch.equal(y[3, 2], y[1, 2]) and y[4:6, 2].isnan().all() and wy[4:6, 2].tolist() == [0.0, 0.0]
    assert torch.equal(y[6, 2], xd.view(9, 5, 2)[6, 2].cpu())               # re-initialised: the sample itself
    assert y[:, 3].isnan().all() and (wy[:, 3] == 0).all() and k[3] == 0.0
    assert torch.equal(y[1, 4], y[0, 4]) and torch.equal(y[6, 4], y[5, 4])  # a zero and a NaN weight: held
    assert torch.isfinite(y[7, [0, 1, 2, 4]]).all()                         # the frame that is NaN throughout: held
    assert k == [1.0, 1.0, 1.0, 0.0, 1.0]


def clip_sums(pkg, dev):
    """N = 7 frames: the four of blend case "generic" and the three of "gain cap" (16 x 16 generated images on 40 x 56 frames)
    -> (x, bg, rows) on the device"""
    a, b = BC.case("generic"), BC.case("gain cap")
    return tuple(torch.cat([a[k], b[k]]).to(dev) for k in ("x", "bg", "rows"))


def test_colour_rows_against_the_model_and_in_splits(pkg, dev):
    ops = pkg.ops
    x, bg, rows = clip_sums(pkg, dev)
    clean = ops.paste_colour_sums(x, bg, rows)
    assert (clean[:, 0] > BC.MIN_WEIGHT).all() and torch.isfinite(clean).all()
    # decay = 0 over frames that all take part: the rows of the match, bit for bit
    state = torch.zeros(13, dtype=torch.float64, device=dev)
    assert same_bits(ops.colour_rows_causal(clean, state, 0.0), ops.paste_colour_match(x, bg, rows))
    assert same_bits(state, clean[6])
    # one frame under min_weight, one frame with a NaN sum
    sums = clean.clone()
    sums[2] *= 3.0 / sums[2, 0]
    sums[5, 7] = float("nan")
    for decay in (0.8, 1.0, 0.0):
        ref_state = np.zeros(13)
        ref = CR.colour_rows_causal(sums.cpu().numpy(), ref_state, decay)
        assert ref["part"].tolist() == [True, True, False, True, True, False, True]
        raw_s, state = guarded(dev, 13 * 8, 256, torch.float64)
        state.zero_()
        raw_r, out = guarded(dev, 7 * 24, 256, torch.float32)
        got_dev = ops.colour_rows_causal(sums, state, decay, out=out.view(7, 3, 2))
        torch.cuda.synchronize()
        assert got_dev.data_ptr() == out.data_ptr() and intact(raw_s, 104, 256) and intact(raw_r, 168, 256)
        got, want = got_dev.cpu().numpy().astype(np.float64), ref["rows"]
        eg, eo = np.abs(got[:, :, 0] - want[:, :, 0]) / want[:, :, 0], np.abs(got[:, :, 1] - want[:, :, 1])
        es = np.abs(state.cpu().numpy() - ref_state) / np.abs(ref_state)
        print(f"colour rows, decay {decay}: largest |g - g_ref| / g_ref = {eg.max():.3e} (bound {2.0 ** -22:.3e}), largest |o - o_ref| = "
              f"{eo.max():.3e} (bound {2.0 ** -15:.3e}); P: largest relative deviation {es.max():.3e}")
        assert eg.max() <= 2.0 ** -22 and eo.max() <= 2.0 ** -15 and es.max() <= TOL_STATE
        for n in (2, 5):                                                    # the rejected frames repeat the previous row
            assert same_bits(got_dev[n], got_dev[n - 1])
        assert not same_bits(got_dev[1], got_dev[0]) and not same_bits(got_dev[3], got_dev[2])
        for split in ([3, 4], [1] * 7):
            st, parts, n0 = torch.zeros(13, dtype=torch.float64, device=dev), [], 0
            for n in split:
                parts.append(ops.colour_rows_causal(sums[n0:n0 + n], st, decay))
                n0 += n
            assert same_bits(torch.cat(parts), got_dev) and same_bits(st, state), (decay, split)
    # nothing yet, and a frame without statistics: (1, 0) by rule; the row formula's parameters reach the kernel
    state = torch.zeros(13, dtype=torch.float64, device=dev)
    assert ops.colour_rows_causal(sums[2:3], state, 0.9).cpu().tolist() == [[[1.0, 0.0]] * 3] and not state.any()
    assert ops.colour_rows_causal(clean, state.zero_(), 0.9, min_weight=1e9).cpu().tolist() == [[[1.0, 0.0]] * 3] * 7 and not state.any()
    assert (ops.colour_rows_causal(clean, state.zero_(), 0.9, max_gain=1.0)[:, :, 0] == 1.0).all()
    assert (ops.colour_rows_causal(clean, state.zero_(), 0.9, min_sigma=200.0)[:, :, 0] == 1.0).all()


def test_entry_points_refuse_on_the_device_side_of_the_launchers(pkg, dev):
    """What the launchers hand through to the C checks (``SpkError`` from ``SPK_EINVAL``), and the tensors they refuse themselves"""
    ops, E = pkg.ops, pkg._lib.SpkError
    x, state = torch.zeros(3, 10, device=dev), ops.causal_filter_state(10, 2, dev)
    with pytest.raises(E, match="float32"):
        ops.causal_filter(x.double(), state)
    with pytest.raises(E, match="state"):
        ops.causal_filter(x, state.cpu())
    with pytest.raises(E, match="state"):
        ops.causal_filter(x, torch.zeros(6, 5, dtype=torch.float64, device=dev).t())
    with pytest.raises(E, match="out"):
        ops.causal_filter(x, state, out=torch.zeros(10, 3, device=dev).t())
    with pytest.raises(E, match="overlaps"):                                # the C check: a state inside the signal
        buf = torch.zeros(64, dtype=torch.float64, device=dev)
        ops.causal_filter(buf.view(torch.float32)[:30].view(3, 10), buf[:30].view(5, 6))
    sums, P = torch.zeros(4, 13, dtype=torch.float64, device=dev), torch.zeros(13, dtype=torch.float64, device=dev)
    with pytest.raises(E, match="state"):
        ops.colour_rows_causal(sums, P.cpu(), 0.5)
    with pytest.raises(E, match="overlap"):
        ops.colour_rows_causal(sums, sums[1], 0.5)
