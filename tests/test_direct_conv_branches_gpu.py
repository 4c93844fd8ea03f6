"""csrc/conv_mfma_f32.hpp (the direct f32 MFMA conv) and the split-K finishers of csrc/conv_api.hip branch by branch, against the
fp64 evaluation of the whole operator (tests/direct_conv_cases.py): every case runs at its forced tile config, the launch form
is asked again of the very descriptor that is launched (``spk_conv2d_launch_form``, real pointers) and must be the declared one,
y / y_pre / the BatchNorm sums are held to the reference, and a second identical launch must reproduce y and y_pre bit for bit.

The bound is measured on the reference, never on the kernel: per case max(4 x the error of the same chain in fp32 on the CPU,
sqrt(kh kw Cin) 2^-24); a single element: |y - ref| <= 8 x bound x rms(ref); the sums: rel-L2 over channels < 1e-6 and per
channel within 8 x bound x rms(ref) x B H W (x 2 max|ref| for the squares).  Which geometry, ring, epilogue form and finisher
each case reaches is asserted without a GPU in tests/test_direct_conv_forms_cpu.py, which also seeds the faults these checks
exist for into the reference (each lands >= 10 x over a limit).

Every launch goes through ``ops.conv_desc`` -- the builder under ``conv2d_fused`` / ``conv3x3_fused`` / ``conv2d_dgrad`` /
``conv_transpose4x4_s2`` / ``conv3x3_wino`` -- and ``ops._launch_conv2d``, so that the residual and a forced config of the transposed
conv, which those wrappers do not pass on, can be part of a case.

Measured on an MI355X (rel-L2 against the fp64 operator, and the bounds of the same cases; max |diff| as a share of its limit):
    3x3 s1, configs 0-7     6.3e-8 .. 1.8e-7   (3.6e-7 .. 8.0e-7)    max |diff| / limit <= 0.42   (y_pre: the same range)
    3x3 s2                  7.7e-8 .. 1.2e-7   (4.4e-7 .. 5.6e-7)    <= 0.33
    7x7 s2                  1.7e-7 .. 2.2e-7   (7.2e-7 .. 1.0e-6)    <= 0.30
    4x4 s2                  9.2e-8 .. 1.2e-7   (4.8e-7 .. 5.8e-7)    <= 0.30
    1x1, s1 and s2          5.0e-8 .. 7.4e-8   (2.2e-7 .. 3.2e-7)    <= 0.50
    2x2 parity (dgrad s2)   6.6e-8 .. 9.1e-8   (3.4e-7 .. 4.1e-7)    <= 0.31
    2x2 parity (transpose)  7.8e-8 .. 1.0e-7   (3.4e-7 .. 3.8e-7)    <= 0.29
    sliced, both finishers  6.3e-8 .. 1.3e-7   (3.7e-7 .. 1.0e-6)    <= 0.39
    sliced Winograd         1.1e-7             (1.4e-6)              <= 0.07
    sliced config 13        1.4e-7 .. 2.4e-7   (2.9e-6)              <= 0.08
    BatchNorm sums: rel-L2 over channels 3.6e-9 .. 5.2e-8 (limit 1e-6); per channel <= 0.09 of the limit (sum), <= 0.02 (squares)
    staged against dword on one shape (staged and halved): bit for bit equal.
The kernel sits a factor 2 to 5 inside the bound everywhere; no case found a fault."""
import importlib

import pytest
import torch

import direct_conv_cases as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _buffer(shape, dev, off, fill=float("nan")):
    """(whole buffer, a contiguous view of ``shape``): 16-byte aligned, or (``off``) starting 4 bytes into the buffer; guard floats
    on both sides."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 8,), fill, device=dev)
    start = 5 if off else 4
    v = buf[start:start + n].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 if off else 0)
    return buf, v, start


def _guards_untouched(buf, start, n):
    return bool(torch.isnan(buf[:start]).all()) and bool(torch.isnan(buf[start + n:]).all())


class Launch:
    """One case on the device: operands, the descriptor, the form the library says it takes."""
    extra_slots = 0          # own-slot copies of the sums beyond the launch's pixel tiles (they must stay zero)

    def query(self):
        return self.ops.desc_launch_form(self.desc)

    def __init__(self, pkg, dev, c):
        ops, L = pkg.ops, pkg._lib
        self.c, self.ops, self.dev = c, ops, dev
        t, o, fam = D.inputs(c), c["opts"], c["family"]
        H, W = D.out_hw(c)
        B, G, Cout, cfg = c["B"], c["G"], c["Cout"], c["config"]
        Cy = G * Cout
        self.on_dev = {name: v.to(dev) for name, v in t.items() if name != "w"}      # (alive as long as the descriptor)
        on = self.on_dev.get
        ws = [w.to(dev) for w in t["w"]]
        if fam == "wino":
            wp = ops.pack_conv_weight_wino(ws[0])
        elif fam in ("dgrad_s2", "dgrad13"):
            wp = ops.pack_conv_weights_list(ws, cfg, 2)
        elif fam == "transpose4x4":
            wp = ops.pack_conv_weight(ws[0], cfg, 3)
        elif "transposed" in o:
            wp = ops.pack_conv_weights_list(ws, cfg, 1)
        else:
            wp = ops.pack_conv_weights_list(ws, cfg)
        self.keep = [wp, ws]
        mis = c["misalign"]
        self.out_buf, self.out, self.out_start = _buffer((B, Cy, H, W), dev, "out" in mis)
        self.pre_buf, self.pre, self.pre_start = _buffer((B, Cy, H, W), dev, "out_pre" in mis) if "y_pre" in o else (None, None, 0)
        noise = residual = None
        if "noise" in o:
            _, noise, _ = _buffer((B, 1, H, W), dev, "noise" in mis)
            noise.copy_(t["noise"])
        if "residual" in o:
            _, residual, _ = _buffer((B, Cy, H, W), dev, "residual" in mis)
            residual.copy_(t["residual"])
        self.y0 = on("y0")
        self.stats = None
        if c["stats"]:
            slots = ops.stats_slots(cfg, c["k"], c["stride"], B, c["Cin"], Cout, H, W) + self.extra_slots if c["stats"] == "own" else 1
            self.stats = torch.zeros(slots, 2, Cy, dtype=torch.float64, device=dev)
        out_scale, scale_dev, slope, gain = D.scalars(c)
        self.scale_dev = torch.tensor([scale_dev], device=dev) if scale_dev is not None else None
        kind = {"wino": L.CONV_WINOGRAD, "dgrad_s2": L.CONV_DGRAD_S2, "dgrad13": L.CONV_DGRAD_S2, "transpose4x4": L.CONV_TRANSPOSE4X4_S2}.get(fam, 0)
        k, stride = {"dgrad_s2": (3, 2), "dgrad13": (3, 2), "transpose4x4": (4, 2)}.get(fam, (c["k"], c["stride"]))
        self.desc, ws_bytes = ops.conv_desc(
            on("x"), wp, Cout, k, stride, flags=kind, out=self.out, hw=(H, W), bias=on("bias"), noise_w=on("noise_w"), noise=noise,
            style=on("style"), upsample="x2" in o, lrelu_slope=slope, out_scale=out_scale,
            in_affine=(on("in_scale"), on("in_shift")) if "affine" in o else None, batch_scale=on("bscale"), demod=on("demod"), act_gain=gain,
            stats=self.stats, out_pre=self.pre, accumulate="accum" in o, accum_half=on("half"),
            out_scale_dev=self.scale_dev, config=cfg, ksplit=c["ksplit"],
            groups=G, shared_input=c["shared"], residual=residual)
        self.keep += [noise, residual]
        if ws_bytes > 0:
            scratch = self.scratch = ops._workspace(dev, ws_bytes)
            self.desc.workspace, self.desc.workspace_bytes = scratch.data_ptr(), scratch.numel() * 4
        self.form = self.query()

    def run(self):
        """-> (y, y_pre, (sum, sumsq)) of one launch into freshly prepared destinations."""
        self.out_buf.fill_(float("nan"))
        if self.y0 is not None:
            self.out.copy_(self.y0)
        if self.pre_buf is not None:
            self.pre_buf.fill_(float("nan"))
        if self.stats is not None:
            self.stats.zero_()
        self.ops._launch_conv2d(self.desc)
        torch.cuda.synchronize()
        assert _guards_untouched(self.out_buf, self.out_start, self.out.numel()), "y: written outside the tensor"
        if self.pre_buf is not None:
            assert _guards_untouched(self.pre_buf, self.pre_start, self.pre.numel()), "y_pre: written outside the tensor"
        st = self.stats.sum(0).cpu() if self.stats is not None else None
        return self.out.clone(), self.pre.clone() if self.pre is not None else None, (st[0], st[1]) if st is not None else None


def _hold(c, y, pre, stats):
    fig = D.figures(c, y, pre, stats)
    for what, (v, lim) in fig.items():            # the figures first, then the assertions
        print(f"{c['name']}: {what} {v:.2e} (limit {lim:.2e}, {v / lim:.3f} of it)")
    for what, (v, lim) in fig.items():
        assert v <= lim, (c["name"], what, v, lim)


@pytest.mark.parametrize("c", D.CASES, ids=lambda c: c["name"])
def test_branch(pkg, dev, c):
    run = Launch(pkg, dev, c)
    form = dict(run.form, slices=run.form["ksplit"])
    assert {k: form[k] for k in c["declares"]} == c["declares"], form      # the launched descriptor takes the declared form
    y, pre, stats = run.run()
    _hold(c, y, pre, stats)
    y2, pre2, _ = run.run()
    assert torch.equal(y, y2), "a second identical launch differs"
    assert pre is None or torch.equal(pre, pre2)


@pytest.mark.parametrize("staged,dword", D.STAGED_VS_DWORD)
def test_staged_and_dword_epilogue_on_one_shape(pkg, dev, staged, dword):
    """The same shape through the staged (or halved) epilogue and, y 4 bytes off, through the dword one: each is held to the
    reference above; here the distance between the two is put on record."""
    a, b = Launch(pkg, dev, D.BY_NAME[staged]), Launch(pkg, dev, D.BY_NAME[dword])
    assert a.form["staged"] > 0 and b.form["staged"] == 0
    ya, yb = a.run()[0], b.run()[0]
    ref = D.reference(a.c)
    diff = float((ya - yb).abs().max())
    print(f"{staged} (staged = {a.form['staged']}) against {dword}: max |difference| {diff:.2e}")
    assert diff <= 2 * D.MAX_FACTOR * ref["bound"] * D.rms(ref["y"])        # (each within the single-element limit of one reference)
