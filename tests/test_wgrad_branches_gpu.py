"""The weight gradient (csrc/wgrad_mfma_f32.hip) branch by branch against the fp64 evaluation of the whole operator
(tests/wgrad_cases.py), and the three slab reducers on their own (tests/wgrad_reduce_ref.py).

Every case launches the descriptor ``ops.wgrad_desc`` assembles -- past the Winograd router of ``ops.conv2d_wgrad`` -- with NaN
guard floats around dw, the declared tensors 4 bytes off a 16-byte boundary, and a NaN-filled workspace of exactly
``spk_conv2d_wgrad_workspace_bytes`` with guard floats behind it.  ``spk_conv2d_wgrad_launch_form`` is asked again of that very
descriptor (real pointers) and must give the declared form; dw is held to the reference; every guard float must be untouched; a
second identical launch must reproduce dw bit for bit.

The bound is measured on the reference, never on the kernel: per case max(4 x the error of the same chain in fp32 on the CPU,
sqrt(B H W) 2^-24); a single element: |dw - ref| <= 8 x bound x rms(ref).  Which kernel, geometry and reducer each case reaches is
asserted without a GPU in tests/test_wgrad_forms_cpu.py, which also seeds the faults these checks exist for into the reference
(each lands >= 10 x over a limit).  Scope: the shipped dispatch; the test fails, not skips, if one of wgrad_cases.ENV_SWITCHES
is set.

The reducers: with scale = 1 and accumulate = 0 the device result equals the NumPy float32 emulation of the documented order bit
for bit (the dword and the vec form give the same bits on one input); with scale or accumulate it is held to the fp64 sum within
max(4 x the emulation's own error, 2^-24).

Measured on an MI355X (rel-L2 against the fp64 operator, and the bounds of the same cases; max |diff| as a share of its limit):
    tap 3x3 s1 (runtime geometry)     5.4e-8 .. 8.3e-8   (2.7e-7 .. 5.3e-7)    max |diff| / limit <= 0.33
    tap 3x3 s1, fixed 16x4 geometry   1.1e-7 .. 1.2e-7   (6.7e-7 .. 9.5e-7)    <= 0.16
    pipe                              1.3e-7 .. 3.2e-7   (9.5e-7 .. 1.1e-6)    <= 0.29
    wide16 / wide8                    8.3e-8 .. 1.9e-7   (4.8e-7 .. 2.7e-6)    <= 0.31
    s2_16 / s2_8                      9.8e-8 .. 1.4e-7   (3.8e-7 .. 9.2e-7)    <= 0.34
    tap 3x3 s2 (the s2 fallbacks)     7.8e-8 .. 1.0e-7   (4.1e-7 .. 7.7e-7)    <= 0.40
    up (bilinear, FIR + batch scale)  1.4e-7 .. 1.5e-7   (6.7e-7 .. 1.6e-6)    <= 0.19
    gemm1x1 (register-staged)         7.6e-8 .. 2.5e-7   (3.4e-7 .. 3.8e-6)    <= 0.55
    gemm1x1_dma                       1.0e-7 .. 2.8e-7   (4.1e-7 .. 1.3e-6)    <= 0.33
    tap 1x1                           7.5e-8 .. 1.4e-7   (4.2e-7 .. 5.2e-7)    <= 0.20
    tap 4x4 s2 (row passes)           8.8e-8 .. 9.7e-8   (4.4e-7 .. 5.8e-7)    <= 0.21
    stem                              6.4e-8 .. 1.2e-7   (3.5e-7 .. 1.5e-6)    <= 0.16
    tap 7x7 packed                    8.5e-8 .. 1.0e-7   (6.7e-7 .. 8.4e-7)    <= 0.10
    wino (routing case)               1.6e-7             (5.3e-7)              <= 0.25
    reducers: dword 2.6e-8 .. 1.1e-7, vec 0 .. 6.7e-8, deep 7.3e-8 .. 1.0e-7 against the fp64 sum (bounds 6.0e-8 .. 4.4e-7); all
    45 reducer cases, those with scale / accumulate included, equal the emulation bit for bit; dword and vec agree bit for bit.
The kernels sit a factor 3 to 7 inside their bounds (rel-L2 at most 0.31 of the bound); every guard float stayed untouched, every
second launch reproduced the first bit for bit.  No case found a fault."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import wgrad_cases as Wc
import wgrad_reduce_ref as Rr

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def pkg():
    Wc.require_default_dispatch()
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _buffer(n, dev, off=False, fill=NAN):
    """(whole buffer, a view of n floats, its start): the view 16-byte aligned, or (``off``) 4 bytes past that; Wc.GUARD floats of
    ``fill`` in front and behind."""
    buf = torch.full((Wc.GUARD + n + 4 + Wc.GUARD,), fill, device=dev)
    start = Wc.GUARD + (1 if off else 0)
    v = buf[start:start + n]
    assert v.data_ptr() % 16 == (4 if off else 0)
    return buf, v, start


def _placed(t, dev, off):
    """``t`` on the device, 16-byte aligned or 4 bytes off."""
    buf, v, _ = _buffer(t.numel(), dev, off, 0.0)
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


def _guards_untouched(buf, start, n):
    return bool(torch.isnan(buf[:start]).all()) and bool(torch.isnan(buf[start + n:]).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _hold(name, fig):
    for what, (v, lim) in fig.items():
        print(f"{name}: {what} {v:.3e} (limit {lim:.3e}, {v / lim:.2f} of it)")
    for what, (v, lim) in fig.items():
        assert v <= lim, (name, what, v, lim)


@pytest.mark.parametrize("c", Wc.CASES, ids=lambda c: c["name"])
def test_wgrad_branch_against_fp64(pkg, dev, c):
    ops, L = pkg.ops, pkg._lib
    t, ref = Wc.inputs(c), Wc.reference(c)
    g, x = _placed(t["g"], dev, "g" in c["misalign"]), _placed(t["x"], dev, "x" in c["misalign"])
    on = {k: t[k].to(dev) for k in ("a", "b", "s", "d") if k in t}
    shape = Wc.dw_shape(c)
    n = int(np.prod(shape))
    dw_buf, dw, dw_start = _buffer(n, dev, "dw" in c["misalign"])
    ws_floats = Wc.workspace_bytes(c, L) // 4
    ws_buf, ws, ws_start = _buffer(ws_floats, dev)

    def reset():
        dw.fill_(NAN)                      # every element must be written ...
        if c["accumulate"]:
            dw.copy_(t["base"].reshape(-1))    # ... or added to
        ws.fill_(NAN)                      # and no slab read that nobody wrote

    d, _ = ops.wgrad_desc(g, x, c["Cout"], c["Cin"], c["k"], c["stride"], upsample=bool(c["up"]), up_fir=c["up"] == "fir",
                          in_affine=(on["a"], on["b"]) if c["mode"] == "affine" else None, batch_scale=on.get("s"), g_scale=on.get("d"),
                          scale=c["scale"], out=dw.view(shape), accumulate=c["accumulate"], splits=c["splits"], groups=c["G"],
                          shared_input=c["shared"], fold=c["fold"], workspace=ws)
    if c["wino"]:
        d.flags |= L.CONV_WINOGRAD
    assert d.workspace_bytes == ws_floats * 4 and d.workspace == ws.data_ptr() and d.dw == dw.data_ptr()
    form = Wc.query(c, L, d)               # the launched descriptor, real pointers
    assert {k: form[k] for k in c["declares"]} == c["declares"], form
    assert form == Wc.query(c, L), "the device pointers change the form"
    assert form["workspace_bytes"] <= ws_floats * 4

    def launch():
        reset()
        L.check(L.lib().spk_conv2d_wgrad(C.byref(d), L.stream_ptr()), "spk_conv2d_wgrad")
        torch.cuda.synchronize()
        return dw.view(shape).clone()

    first = launch()
    _hold(c["name"], dict(Wc.figures(c, first), bound=(ref["bound"], Wc.TOL_OP)))
    assert _guards_untouched(dw_buf, dw_start, n), "dw: guard floats written"
    assert _guards_untouched(ws_buf, ws_start, ws_floats), "a write past spk_conv2d_wgrad_workspace_bytes"
    second = launch()
    assert torch.equal(_bits(first), _bits(second)), "a second identical launch differs"


@pytest.mark.parametrize("c,msg", Wc.REFUSALS, ids=[c["name"] for c, _ in Wc.REFUSALS])
def test_wgrad_refusals_with_device_tensors(pkg, dev, c, msg):
    ops, L = pkg.ops, pkg._lib
    H, W = Wc.out_hw(c)
    g = torch.zeros(c["B"], c["G"] * c["Cout"], H, W, device=dev)
    x = torch.zeros(c["B"], Wc.x_channels(c), c["Hs"], c["Ws"], device=dev)
    s = torch.ones(c["B"], c["Cin"], device=dev) if c["mode"] == "bscale" else None
    dd = torch.ones(c["B"], c["Cout"], device=dev) if c["mode"] == "bscale" else None
    dw = torch.full(Wc.dw_shape(c), NAN, device=dev)
    d, _ = ops.wgrad_desc(g, x, c["Cout"], c["Cin"], c["k"], c["stride"], upsample=bool(c["up"]), batch_scale=s, g_scale=dd, out=dw, groups=c["G"])
    with pytest.raises(L.SpkError, match=msg):
        L.check(L.lib().spk_conv2d_wgrad(C.byref(d), L.stream_ptr()), "spk_conv2d_wgrad")
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw).all())


# ---- the reducers on their own: spk_wgrad_reduce_slabs with synthetic slabs ------------------------------------------------------------
def _reduce(pkg, dev, c):
    L = pkg._lib
    slabs_h = Rr.slabs_of(c)
    slabs = torch.from_numpy(slabs_h).to(dev)
    assert slabs.data_ptr() % 16 == 0
    shape = (c["Cout_all"] // c["fold"], c["Cin"], c["taps"])
    n = int(np.prod(shape))
    buf, dw, start = _buffer(n, dev, c["misalign_dw"])
    if c["accumulate"]:
        dw.copy_(torch.from_numpy(Rr.base_of(c)).reshape(-1))
    form = L.WgradForm()
    args = (slabs.data_ptr(), dw.data_ptr(), c["n_slabs"], c["Cout_all"], c["Cin"], c["taps"])
    L.check(L.lib().spk_wgrad_reduce_form(*args, c["fold"], form), "spk_wgrad_reduce_form")
    assert Rr.REDUCERS[form.reducer] == c["reducer"]
    L.check(L.lib().spk_wgrad_reduce_slabs(*args, c["scale"], int(c["accumulate"]), c["fold"], L.stream_ptr()), "spk_wgrad_reduce_slabs")
    torch.cuda.synchronize()
    assert _guards_untouched(buf, start, n), "dw: guard floats written"
    assert torch.equal(slabs.cpu(), torch.from_numpy(slabs_h)), "the slabs are read only"
    return dw.view(shape).cpu().numpy()


@pytest.mark.parametrize("c", Rr.CASES, ids=lambda c: c["name"])
def test_wgrad_reducer(pkg, dev, c):
    got = _reduce(pkg, dev, c)
    ref, emu, bound = Rr.expected(c)
    err = float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref))
    worst = float(np.abs(got.astype(np.float64) - ref).max() / (Wc.MAX_FACTOR * bound * np.sqrt(np.mean(ref ** 2))))
    print(f"{c['name']}: rel-L2 {err:.3e} (bound {bound:.3e}), max|diff| {worst:.2f} of its limit, bitwise equal to the emulation: {np.array_equal(got, emu)}")
    if c["scale"] == 1.0 and not c["accumulate"]:
        assert np.array_equal(got.view(np.int32), emu.view(np.int32)), "not the documented summation order"
    assert err <= bound and worst <= 1.0


def test_wgrad_reducers_dword_and_vec_share_their_order(pkg, dev):
    a, b = (Rr.BY_NAME[n] for n in Rr.SAME_ORDER)
    assert np.array_equal(_reduce(pkg, dev, a).view(np.int32), _reduce(pkg, dev, b).view(np.int32))
