"""The inputs of the GPU cases of tests/test_blend_gpu.py, built by name so that tests/test_blend_cpu.py can assert on the CPU what
those cases rely on (the margin condition, the variances, the distance of every S0 from ``min_weight``).  Shapes are those of
tests/test_align_gpu.py: 40 x 56 frames, generated images (16,16) and (12,20), 3..4 frames, its rows.  A case's reference is
computed once (``reference``) and shared; nobody writes into it."""
import functools

import numpy as np
import torch

import blend_ref as B
import sim_ref as R

H, W = 40, 56
NETS = [(16, 16), (12, 20)]
ANGLE_SCALE = [(0.3, 1.3), (-1.1, 0.6), (0.77, 2.3), (0.0, 1.0)]            # rotation, s < 1, s > 2, the identity
CENTRES = [(20.3, 27.6), (18.9, 30.2), (21.4, 25.1), (19.7, 28.4)]
MARGIN = 1e-6
MAX_GAIN, MIN_SIGMA, MIN_WEIGHT = 2.0, 1.0, 16.0                            # the defaults of ops.paste_colour_match


def frames(seed, *shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def source(seed, N, Hs, Ws, sigma=0.7):
    """Generated frames: most values inside (-1, 1), some beyond both ends."""
    return torch.randn(N, 3, Hs, Ws, generator=torch.Generator().manual_seed(seed)) * sigma


def rows_for(which, net):
    return torch.tensor([R.rows(CENTRES[i], ANGLE_SCALE[i][1] * net[1], ANGLE_SCALE[i][0], net) for i in which], dtype=torch.float64).float()


def matte_for(seed, frames_, Hs, Ws):
    """Random in [0, 1] with a patch of exact 0 and a patch of exact 1 per frame, values outside [0, 1] and one NaN."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(frames_, Hs, Ws, generator=g)
    for f in range(frames_):
        m[f, 1:7, 2 + f:9 + f] = 0.0
        m[f, Hs - 5:Hs - 1, Ws - 8:Ws - 3] = 1.0
        m[f, Hs // 2, 1] = -0.3
        m[f, Hs // 2 + 1, Ws - 2] = 1.4
    m[0, Hs // 2, Ws // 2] = float("nan")
    return m


# name -> how the case is made.  ``x``: "random" (sigma 0.7), "tenth" (sigma 2.5 scaled by 0.1: the gain meets max_gain),
# "constant" (a level per channel: var_q = 0).  ``matte``: None, "shared" [Hs,Ws], "frames" [N,Hs,Ws]; ``zero``: a frame whose
# matte is all zero; ``bad``: a frame whose row is NaN (device rows only).
SPECS = {
    "matte shared":        dict(net=(16, 16), which=(0, 1, 2), matte="shared", feather=0.0),
    "matte frames":        dict(net=(12, 20), which=(3, 2, 0), matte="frames", feather=2.5),
    "matte frames square": dict(net=(16, 16), which=(3, 2, 0), matte="frames", feather=0.0),
    "matte shared wide":   dict(net=(12, 20), which=(0, 1, 2), matte="shared", feather=2.5),
    "generic":             dict(net=(16, 16), which=(0, 1, 2, 3)),
    "generic wide":        dict(net=(12, 20), which=(3, 2, 0)),
    "gain cap":            dict(net=(16, 16), which=(0, 2, 3), x="tenth"),
    "constant":            dict(net=(12, 20), which=(0, 2, 3), x="constant"),
    "invalid and zero":    dict(net=(16, 16), which=(0, 3, 2, 0), matte="frames", zero=1, bad=2),
    "bgr":                 dict(net=(12, 20), which=(0, 1, 2), bgr=True),
    "strided":             dict(net=(16, 16), which=(2, 0, 3)),
    "feather and matte":   dict(net=(16, 16), which=(0, 2, 3), matte="shared", feather=2.5),
}
MATTE_CASES = [k for k in SPECS if k.startswith("matte ")]
COLOUR_CASES = [k for k in SPECS if not k.startswith("matte ")]
PASTE_COLOUR_CASES = ["generic", "bgr", "feather and matte", "gain cap"]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(x, bg, rows, matte, feather, bgr, net): CPU tensors"""
    spec = SPECS[name]
    seed = 100 + sorted(SPECS).index(name)
    net, which = spec["net"], spec["which"]
    N = len(which)
    kind = spec.get("x", "random")
    if kind == "constant":
        x = torch.tensor([0.2, -0.3, 0.5]).view(1, 3, 1, 1).expand(N, 3, *net).contiguous()
    else:
        x = source(seed, N, *net, sigma=2.5) * 0.1 if kind == "tenth" else source(seed, N, *net)
    rows = rows_for(which, net)
    if "bad" in spec:
        rows[spec["bad"], 0] = float("nan")
    matte = None
    if spec.get("matte"):
        matte = matte_for(seed + 50, N if spec["matte"] == "frames" else 1, *net)
        if "zero" in spec:
            matte[spec["zero"]] = 0.0
        if spec["matte"] == "shared":
            matte = matte[0]
    return dict(x=x, bg=frames(seed + 25, N, H, W, 3), rows=rows, matte=matte, feather=spec.get("feather", 0.0), bgr=spec.get("bgr", False),
                net=net, by_rule=[i for i in (spec.get("zero"), spec.get("bad")) if i is not None], kind=kind)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The model of a case without colour rows (``blend_ref.blend``), and its rows (``blend_ref.colour_rows``): computed once."""
    c = case(name)
    ref = B.blend(c["x"].numpy(), c["bg"].numpy(), c["rows"].numpy(), feather=c["feather"], swap_rb=c["bgr"],
                  matte=None if c["matte"] is None else c["matte"].numpy())
    ref["rows"], ref["var_q"], ref["var_b"] = B.colour_rows(ref["sums"], ref["valid"], MAX_GAIN, MIN_SIGMA, MIN_WEIGHT)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref
