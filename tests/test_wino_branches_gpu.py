"""csrc/conv3x3_wino_f32.hip kernel form by kernel form and region walk by region walk, against the fp64 evaluation of the whole
operator (tests/wino_cases.py).  Every case runs at the smallest batch that meets its walk target on THIS device
(``batch_for``), ``spk_conv2d_wino_form`` is asked again of the very launch (real pointers, the device's CU count) and must answer the
declared form, and y / y_pre / the toRGB image are held to the reference: the aggregate to the case's bound, every element to
8 x bound x rms(ref).  The bound is measured on the references, never on the kernel (max(4 x the error of the fp32 Winograd emulation,
sqrt(9 Cin) 2^-24) per output tensor); tests/test_wino_forms_cpu.py proves without a GPU which instantiation and which walk each case
reaches and that the walks cross image and slice boundaries.

Every output -- and the workspace of a sliced launch -- is a view into a larger buffer filled with a sentinel bit pattern, whose
guard bands must keep their bits.  (A LEAN_NOSTORE launch is chosen by y == NULL: it has no y buffer that could be looked at.)
Relations that differ in addressing and control flow only are held bit for bit: a walk against the same images launched one at a
time, the LEAN_NOSTORE toRGB image against the LEAN one, a second launch against the first; and at the 2 GB limit of the 32-bit
gather offsets the first and last image against their own B = 1 launches.

Measured on an MI355X (256 CUs; rel-L2 against the fp64 operator, the bounds of the same cases, max |diff| as a share of its limit):
    one item per workgroup, 32 cases    7.7e-8 .. 2.0e-7   (7.2e-7 .. 1.4e-6)    max |diff| / limit <= 0.38   (y_pre, rgb: the same range)
    walks of 2 and 3 items, 27 cases    the same range     (7.2e-7 .. 2.0e-6)    rel-L2 / bound <= 0.23
    the 2 GB edge, last image           1.6e-7 (7.2e-7), max |diff| 0.20 of its limit; plain and x2: first and last image bit for bit their B = 1 launches
    walk against one launch per image, LEAN_NOSTORE against LEAN, a second launch: bit for bit equal in every case.
The whole file runs in 12 s, the slowest case in 0.6 s.  No case found a fault."""
import contextlib
import importlib

import pytest
import torch
import torch.nn.functional as F

import wino_cases as W

pytestmark = pytest.mark.gpu
SENTINEL = 0x7FC5A5A5            # a NaN no arithmetic produces: an element the launch left out fails every comparison
GUARD = 4096                     # floats on either side: four planes of the 16 x 64 cases


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    return importlib.import_module("speak-hack_amd")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Guarded:
    """A contiguous fp32 view of ``shape`` between two guard bands, 16-byte aligned (``off``: 4 bytes past that)."""

    def __init__(self, shape, dev, off=False):
        n = 1
        for s in shape:
            n *= s
        self.n, self.start = n, GUARD + (1 if off else 0)
        self.bits = torch.full((n + 2 * GUARD + 4,), SENTINEL, dtype=torch.int32, device=dev)
        self.view = self.bits.view(torch.float32)[self.start:self.start + n].view(shape)
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (4 if off else 0)

    def reset(self):
        self.bits.fill_(SENTINEL)

    def guards_intact(self):
        return bool((self.bits[:self.start] == SENTINEL).all()) and bool((self.bits[self.start + self.n:] == SENTINEL).all())


@contextlib.contextmanager
def guarded_workspace(ops, device, nbytes):
    """``ops._workspace`` serves a guarded buffer of exactly ``nbytes`` to the launches inside."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    before = ops._workspaces.get(key)
    g = Guarded((nbytes // 4,), device) if nbytes > 0 else None
    if g is not None:
        ops._workspaces[key] = g.view
    try:
        yield g
    finally:
        torch.cuda.synchronize()
        if before is not None:
            ops._workspaces[key] = before
        else:
            ops._workspaces.pop(key, None)


class Run:
    """One case on the device at batch B: operands, guarded outputs, launches of any range of its images."""

    def __init__(self, pkg, dev, n_cu, c, B):
        ops = pkg.ops
        self.c, self.ops, self.dev, self.n_cu, self.B = c, ops, dev, n_cu, B
        o, G, Cout, H, W_ = c["opts"], c["G"], c["Cout"], c["H"], c["W"]
        t = W.inputs(c, B)
        self.t = {k: v.to(dev) for k, v in t.items() if k not in ("w", "x")}
        gx = Guarded(tuple(t["x"].shape), dev, c["misalign_x"])
        gx.view.copy_(t["x"])
        self.x = gx.view
        ws = [w.to(dev) for w in t["w"]]
        if G == 1:
            self.wp = ops.pack_conv_weight_wino(ws[0])
        else:
            n = pkg._lib.lib().spk_conv2d_packed_bytes_wino(c["Cin"], Cout) // 4
            self.wp = torch.empty(G * n, device=dev)
            ops.pack_conv_weights_wino_into(ws, [self.wp[i * n:(i + 1) * n] for i in range(G)])
        self.scale_dev = torch.tensor([W.SCALE_DEV], device=dev) if "scale_dev" in o else None
        shape = (B, G * Cout, H, W_)
        self.out = {n: Guarded({"y": shape, "pre": shape, "rgb": (B, 3, H, W_)}[n], dev) for n in W.outputs(c)}
        self.ws_bytes = int(pkg._lib.lib().spk_conv2d_wino_workspace_bytes(c["want"], B, c["Cin"], G * Cout, H, W_))

    def kwargs(self, b0, b1):
        """The arguments of ``ops.conv3x3_wino`` for images [b0, b1), written into the same images of the outputs."""
        c, t, o = self.c, self.t, self.c["opts"]
        on = lambda name: t[name][b0:b1] if name in t else None
        out_scale, _, slope, gain = W.scalars(c)
        view = lambda n: self.out[n].view[b0:b1] if n in self.out else None
        return dict(bias=t.get("bias"), noise_w=t.get("noise_w"), noise=on("noise"), style=on("style"), lrelu_slope=slope, out_scale=out_scale,
                    act_gain=gain, out=view("y"), out_pre=view("pre"), accumulate="accum" in o, out_scale_dev=self.scale_dev, batch_scale=on("bscale"),
                    demod=on("demod"), ksplit=c["want"], rgb=(t["rgb_w"], t["rgb_b"]) if "rgb" in o else None, rgb_out=view("rgb"),
                    store_out="nostore" not in o, groups=c["G"], upsample="x2" in o)

    def form(self, b0=0, b1=None):
        """``spk_conv2d_wino_form`` of the descriptor those arguments make."""
        b1 = self.B if b1 is None else b1
        kw = self.kwargs(b0, b1)
        rgb = kw.pop("rgb")
        kw.pop("store_out")
        if rgb is not None:
            kw.update(rgb_w=rgb[0].reshape(3, -1).contiguous(), rgb_bias=rgb[1])
        else:
            kw.pop("rgb_out")
        return self.ops.wino_launch_form(self.x[b0:b1], self.wp, self.c["Cout"], n_cu=self.n_cu, **kw)

    def prepare(self):
        for g in self.out.values():
            g.reset()
        if "accum" in self.c["opts"]:
            self.out["y"].view.copy_(self.t["y0"])

    def launch(self, b0, b1):
        self.ops.conv3x3_wino(self.x[b0:b1], self.wp, self.c["Cout"], **self.kwargs(b0, b1))

    def whole(self):
        """One launch of all images into freshly prepared outputs -> {name: tensor}; every guard band keeps its bits."""
        self.prepare()
        with guarded_workspace(self.ops, self.dev, self.ws_bytes) as ws:
            self.launch(0, self.B)
            torch.cuda.synchronize()
            assert ws is None or ws.guards_intact(), "workspace: written outside the buffer"
        for n, g in self.out.items():
            assert g.guards_intact(), f"{n}: written outside the tensor"
        return {n: g.view.clone() for n, g in self.out.items()}

    def one_by_one(self):
        """The same images, one launch each."""
        self.prepare()
        for b in range(self.B):
            self.launch(b, b + 1)
        torch.cuda.synchronize()
        for n, g in self.out.items():
            assert g.guards_intact(), f"{n}: written outside the tensor"
        return {n: g.view.clone() for n, g in self.out.items()}


def _hold(c, got, want):
    fig = W.figures(c, got, want)
    for what, (v, lim) in fig.items():            # the figures first, then the assertions
        print(f"{c['name']}: {what} {v:.2e} (limit {lim:.2e}, {v / lim:.3f} of it)")
    for what, (v, lim) in fig.items():
        assert v <= lim, (c["name"], what, v, lim)


@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c["name"])
def test_branch(pkg, dev, n_cu, c):
    L = pkg._lib
    B = W.batch_for(c, n_cu, L)
    run = Run(pkg, dev, n_cu, c, B)
    form = run.form()
    assert {k: form[k] for k in c["declares"]} == c["declares"], form      # the launch itself takes the declared form
    assert W.meets_walk(c, form), form
    print(f"{c['name']}: B {B}, grid {form['grid_x']} x {form['co_tiles']}, {form['items']} items, walks {form['walk_min']}..{form['walk_max']}")
    got = run.whole()
    _hold(c, got, W.reference(c, B))
    again = run.whole()
    for n in got:
        assert torch.equal(got[n], again[n]), f"{n}: a second identical launch differs"
    if c["walk"] > 1:
        assert run.form(0, 1)["walk_max"] == 1
        single = run.one_by_one()
        for n in got:
            assert torch.equal(got[n], single[n]), f"{n}: the walk differs from the same images launched one at a time"


@pytest.mark.parametrize("nostore,lean", W.NOSTORE_VS_LEAN)
def test_nostore_rgb_is_the_lean_rgb(pkg, dev, n_cu, nostore, lean):
    ca, cb = W.BY_NAME[nostore], W.BY_NAME[lean]
    B = W.batch_for(ca, n_cu, pkg._lib)
    assert B == W.batch_for(cb, n_cu, pkg._lib)
    a, b = Run(pkg, dev, n_cu, ca, B), Run(pkg, dev, n_cu, cb, B)
    assert (a.form()["epi"], b.form()["epi"]) == (W.LEAN_NOSTORE, W.LEAN)
    assert torch.equal(a.whole()["rgb"], b.whole()["rgb"])


def test_the_2gb_edge_of_the_gather_offsets(pkg, dev, n_cu):
    """x [127, 16, 512, 512] is 2^31 - 16 MB bytes: the last size the 32-bit offsets (bit 31 = out of range) serve.  The first and
    the last image equal their own B = 1 launches bit for bit, the last one is held to fp64; one image more is refused.  The same
    for the x2 form, whose limit is the INPUT tensor's (output 1024^2, 4 GB): first and last image only."""
    ops, L = pkg.ops, pkg._lib
    B, Cin, Cout, S = 127, 16, 8, 512
    assert B * Cin * S * S * 4 == 2 ** 31 - (16 << 20)
    x = torch.randn((B, Cin, S, S), device=dev, generator=torch.Generator(device=dev).manual_seed(31))
    w = W.recipe_tensor("wino.2gb.w", (Cout, Cin, 3, 3), (9 * Cin) ** -0.5)
    wp = ops.pack_conv_weight_wino(w.to(dev))
    assert ops.wino_supported(B, Cin, Cout, S, S) and not ops.wino_supported(B + 1, Cin, Cout, S, S)
    lib = L.lib()
    assert lib.spk_conv2d_wino_up_supported(B, Cin, Cout, 2 * S, 2 * S) and not lib.spk_conv2d_wino_up_supported(B + 1, Cin, Cout, 2 * S, 2 * S)
    for up in (False, True):
        y = ops.conv3x3_wino(x, wp, Cout, ksplit=1, upsample=up)
        first = ops.conv3x3_wino(x[:1], wp, Cout, ksplit=1, upsample=up)
        last = ops.conv3x3_wino(x[B - 1:], wp, Cout, ksplit=1, upsample=up)
        torch.cuda.synchronize()
        assert torch.equal(y[:1], first), f"up={up}: the first image differs from its own launch"
        assert torch.equal(y[B - 1:], last), f"up={up}: the last image differs from its own launch"
        if not up:
            xl = x[B - 1:].cpu()
            ref = F.conv2d(xl.double(), w.double(), padding=1)
            bound = max(4 * W.rel_l2(W.wino_conv32(xl, w), ref), (9 * Cin) ** 0.5 * 2.0 ** -24)
            err, worst = W.rel_l2(last.cpu(), ref), float((last.cpu().double() - ref).abs().max())
            print(f"2 GB edge, last image: rel-L2 {err:.2e} (bound {bound:.2e}), max|diff| {worst:.2e} (limit {W.MAX_FACTOR * bound * W.rms(ref):.2e})")
            assert bound <= W.TOL and err <= bound and worst <= W.MAX_FACTOR * bound * W.rms(ref)
        del y, first, last
    del x
    big = torch.empty((B + 1, Cin, S, S), device=dev)       # 2^31 bytes: never read, the launch refuses
    for up in (False, True):
        with pytest.raises(L.SpkError, match="2 GB|twice the input size"):
            ops.conv3x3_wino(big, wp, Cout, ksplit=1, upsample=up)
    del big
    torch.cuda.empty_cache()
