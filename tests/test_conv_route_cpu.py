"""The 3x3 stride-1 route table on the host (``ops.conv3x3_route``; no launch): which kernel -- bf16x3 (B), fp32 Winograd (W)
or the direct kernel with its tile config (a number) -- every 3x3 stride-1 conv of the project's workloads runs, layer by layer.
The expected strings are what the call sites decided inline before the route had one home; a change here is a change of
which kernel runs, never a refactor."""
import importlib

import pytest


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("speak-hack_amd").ops


def _nf(stage):
    return min(int(8192 / 2 ** stage), 512)


def _decoder(res_max):
    """(Cin, Cout, output resolution, x2) of SynthesisNetwork's 3x3 convs."""
    out, cin, r = [], 512, 8
    while r <= res_max:
        co = min(int(8192 / (2.0 ** (r.bit_length() - 2))), 512)
        out += [(cin, co, r, True), (co, co, r, False)]
        cin, r = co, r * 2
    return out


def _stylegan2():
    out, cin = [(512, 512, 4, False)], 512
    for r in range(3, 9):
        co = _nf(r - 1)
        out += [(cin, co, 2 ** r, True), (co, co, 2 ** r, False)]
        cin = co
    return out


DISC = [(_nf(s - 1), 2 ** s) for s in range(8, 2, -1)] + [(512, 4)]      # block conv1 per resolution + final_conv (B = 8)
TRUNK = [(64, 64), (128, 32), (256, 16), (512, 8)]                        # the stride-1 Bottleneck conv2 of ResNet-50 at 256^2

EXPECTED = {
    ("auto", "f32", "decoder256 forward"): "6 6 W W W W W W W W W W",
    ("auto", "f32", "decoder256 dgrad"): "6 6 W W W W W W W W W W",
    ("auto", "f32", "decoder512 forward"): "6 6 W W W W W W W W W W W W",
    ("auto", "f32", "decoder512 dgrad"): "6 6 W W W W W W W W W W W W",
    ("auto", "f32", "discriminator"): "W W W W W 6 6",
    ("auto", "f32", "decoder256 plan"): "6 6 W W W W W W W W W W",
    ("auto", "f32", "stylegan2 plan"): "6 6 6 W W W W W W W W W W",
    ("auto", "bf16x3", "decoder256 forward"): "6 6 W W B B B B B B B B",
    ("auto", "bf16x3", "decoder256 dgrad"): "6 6 W W B B B B B B B B",
    ("auto", "bf16x3", "decoder512 forward"): "6 6 W W B B B B B B B B B B",
    ("auto", "bf16x3", "decoder512 dgrad"): "6 6 W W B B B B B B B B B B",
    ("auto", "bf16x3", "discriminator"): "B B B B W 6 6",
    ("auto", "bf16x3", "decoder256 plan"): "6 6 W W B B B B B B B B",
    ("auto", "bf16x3", "stylegan2 plan"): "6 6 6 W W B B B B B B B B",
    ("auto", "f32", "stylegan2 forward"): "6 6 6 W W W W W W W W W W",
    ("auto", "f32", "stylegan2 dgrad"): "6 6 6 W W W W W W W W W W",
    ("auto", "f32", "trunk dgrad g6"): "W W W 6",
    ("auto", "f32", "trunk dgrad g3"): "W W W 6",
    ("auto", "f32", "trunk dgrad g1"): "W W W 6",
    ("direct", "f32", "decoder256 forward"): "6 6 4 4 4 4 4 4 5 4 5 5",
    ("direct", "f32", "decoder256 dgrad"): "6 6 4 4 4 4 4 4 4 4 5 5",
    ("direct", "f32", "decoder512 forward"): "6 6 6 6 4 4 4 4 4 4 5 5 7 7",
    ("direct", "f32", "decoder512 dgrad"): "6 6 6 6 4 4 4 4 4 4 5 5 5 7",
    ("direct", "f32", "discriminator"): "5 4 4 4 4 6 6",
    ("direct", "f32", "decoder256 plan"): "6 6 4 4 4 4 4 4 5 4 5 5",
    ("direct", "f32", "stylegan2 plan"): "6 6 6 4 4 4 4 4 4 5 4 5 5",
    ("direct", "bf16x3", "decoder256 forward"): "6 6 B B B B B B B B B B",
    ("direct", "bf16x3", "decoder256 dgrad"): "6 6 B B B B B B B B B B",
    ("direct", "bf16x3", "decoder512 forward"): "6 6 6 6 B B B B B B B B B B",
    ("direct", "bf16x3", "decoder512 dgrad"): "6 6 6 6 B B B B B B B B B B",
    ("direct", "bf16x3", "discriminator"): "B B B B B 6 6",
    ("direct", "bf16x3", "decoder256 plan"): "6 6 B B B B B B B B B B",
    ("direct", "bf16x3", "stylegan2 plan"): "6 6 6 B B B B B B B B B B",
    ("direct", "f32", "stylegan2 forward"): "6 6 6 4 4 4 4 4 4 5 4 5 5",
    ("direct", "f32", "stylegan2 dgrad"): "6 6 6 4 4 4 4 4 4 4 4 5 5",
    ("direct", "f32", "trunk dgrad g6"): "6 6 6 6",
    ("direct", "f32", "trunk dgrad g3"): "6 6 6 6",
    ("direct", "f32", "trunk dgrad g1"): "6 6 6 6",
}


def _rows(ops, what, precision):
    R = ops.conv3x3_route
    plan_p = dict(precision=precision)
    if what == "decoder256 forward":           # FusedConvFn / the eager decoder at the headline batch
        return [R(8, ci, co, r, r) for ci, co, r, up in _decoder(256)]
    if what == "decoder256 dgrad":
        return [R(8, co, ci, r, r) for ci, co, r, up in _decoder(256)]
    if what == "decoder512 forward":           # BASELINE config 5: SynthesisNetwork(512), batch 4
        return [R(4, ci, co, r, r) for ci, co, r, up in _decoder(512)]
    if what == "decoder512 dgrad":
        return [R(4, co, ci, r, r) for ci, co, r, up in _decoder(512)]
    if what == "discriminator":                # ConvBiasLReLUFn forward = _conv_dgrad's shapes (Cin == Cout)
        return [R(8, c, c, r, r) for c, r in DISC]
    if what == "decoder256 plan":              # plan.DecoderPlan: the plan's own precision, x2 layers with their input width
        return [R(8, ci, co, r, r, up_w=r // 2 if up else None, **plan_p) for ci, co, r, up in _decoder(256)]
    if what == "stylegan2 plan":
        return [R(8, ci, co, r, r, modulated=True, up_w=r // 2 if up else None, **plan_p) for ci, co, r, up in _stylegan2()]
    if what == "stylegan2 forward":            # ModConvFn / ModulatedConv2d: never the split-precision kernel
        return [R(8, ci, co, r, r, precision="f32", modulated=True, up_w=r // 2 if up else None) for ci, co, r, up in _stylegan2()]
    if what == "stylegan2 dgrad":
        return [R(8, co, ci, r, r, precision="f32", modulated=True) for ci, co, r, up in _stylegan2()]
    G = int(what[-1])                          # the trunks' grouped data gradients (6 passes of B/2 images, 3 of B, one)
    B = 4 if G == 6 else 8
    return [R(B, c, c, r, r, precision="f32", groups=G) for c, r in TRUNK]


def _code(route):
    kind, config = route
    assert (config == -1) == (kind != "direct"), route
    return {"wino": "W", "bf16x3": "B"}.get(kind, str(config))


@pytest.mark.parametrize("algo,precision,what", sorted(EXPECTED))
def test_route_table(ops, algo, precision, what):
    with ops.conv3x3_algo(algo), ops.train_conv_precision(precision):
        got = " ".join(_code(r) for r in _rows(ops, what, precision))
    assert got == EXPECTED[(algo, precision, what)]


def test_route_precision_argument_overrides_the_training_switch(ops):
    for ci, co, r, up in _decoder(256):
        with ops.train_conv_precision("bf16x3"):
            assert ops.conv3x3_route(8, ci, co, r, r, precision="f32") != ("bf16x3", -1)
            assert ops.conv3x3_route(8, ci, co, r, r) == ops.conv3x3_route(8, ci, co, r, r, precision="bf16x3")
            assert ops.train_bf16x3(8, ci, co, r, r) == (ops.conv3x3_route(8, ci, co, r, r)[0] == "bf16x3")
        assert ops.conv3x3_route(8, ci, co, r, r) == ops.conv3x3_route(8, ci, co, r, r, precision="f32")


def test_route_site_conditions(ops, monkeypatch):
    """The facts only a call site knows: a x2 layer's input width (Winograd reads whole 4-pixel rows of the materialised image),
    whether the caller can feed the Winograd kernel at all (the trunks' alignment), and the modulated conv's configs (+4)."""
    monkeypatch.setattr(ops, "use_wino", lambda *a, **k: True)
    monkeypatch.setattr(ops, "conv2d_pick_config", lambda *a: 1)
    assert ops.conv3x3_route(2, 64, 64, 32, 32, up_w=16) == ("wino", -1)
    assert ops.conv3x3_route(2, 64, 64, 32, 32, up_w=18) == ("direct", 1)
    assert ops.conv3x3_route(2, 64, 64, 32, 32, up_w=18, modulated=True) == ("direct", 5)
    assert ops.conv3x3_route(2, 64, 64, 32, 32, wino_ok=False) == ("direct", 1)
    monkeypatch.setattr(ops, "conv2d_pick_config", lambda *a: 6)
    assert ops.conv3x3_route(2, 64, 64, 32, 32, wino_ok=False, modulated=True) == ("direct", 6)
