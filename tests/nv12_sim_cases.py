"""The inputs of the GPU cases of tests/test_nv12_align_gpu.py, built by name so that tests/test_nv12_align_cpu.py can assert on the
CPU what those cases rely on (the margin condition, chroma blocks with 1, 2, 3 and 4 region pixels, the variances, the distance of
every S0 from ``min_weight``).  Shapes are those of tests/blend_cases.py -- 40 x 56 surfaces, generated images (16,16) and (12,20),
3..4 frames, its centres, angles and scales, its mattes and sources.  Surfaces are made from random RGB bytes through the fp64
``from_rgb`` of the case's standard, so that most pixels are in gamut; the case "raw bytes" has random Y, U and V bytes, much of
it out of gamut.  A case's reference is computed once (``reference``) and shared; nobody writes into it."""
import functools
import importlib

import numpy as np
import torch

import blend_cases as BC
import blend_ref as B
import nv12_sim_ref as M

H, W, PITCH, GUARD = 40, 56, 64, 256
NETS, ANGLE_SCALE, CENTRES, MARGIN = BC.NETS, BC.ANGLE_SCALE, BC.CENTRES, BC.MARGIN
MAX_GAIN, MIN_SIGMA, MIN_WEIGHT = BC.MAX_GAIN, BC.MIN_SIGMA, BC.MIN_WEIGHT         # the defaults of ops.paste_colour_match_nv12


@functools.lru_cache(maxsize=None)
def coeffs(standard="bt601", full_range=False):
    """``ops.yuv_coeffs`` as numpy fp64 -> (to_rgb [3,4], from_rgb [3,4]); host code, no device"""
    ops = importlib.import_module("speak-hack_amd").ops
    return tuple(t.numpy() for t in ops.yuv_coeffs(standard, full_range))


def surface_from_rgb(seed, N, h, w, standard="bt601", full_range=False):
    """Random RGB bytes through the fp64 ``from_rgb``: Y per pixel, (U, V) as the mean of the block.  -> uint8 (y [N,h,w], uv [N,h/2,w/2,2])"""
    F = coeffs(standard, full_range)[1]
    rgb = BC.frames(seed, N, h, w, 3).numpy().astype(np.float64)
    e = rgb @ F[:, :3].T + F[:, 3]
    y = np.rint(np.clip(e[..., 0], 0, 255)).astype(np.uint8)
    uv = np.rint(np.clip(M.blocks(e[..., 1:]).mean(3), 0, 255)).astype(np.uint8)
    return torch.from_numpy(y), torch.from_numpy(uv)


def surface_raw(seed, N, h, w):
    return BC.frames(seed, N, h, w), BC.frames(seed + 1, N, h // 2, w // 2, 2)


# ---- pitched planes between guard bytes ------------------------------------------------------------------------------------------
class Pitched:
    """The two planes on ``dev`` in rows of ``pitch`` bytes, every other byte of both buffers 0xA5: before the first frame, behind
    the last, and between the rows.  ``y`` [N,h,w] and ``uv`` [N,h/2,w/2,2] are views; ``intact()`` says the 0xA5 bytes still are."""

    def __init__(self, y, uv, dev, pitch=PITCH, guard=GUARD):
        N, h, w = y.shape
        self.raw, self.mask = [], []
        views = []
        for plane, rows in ((y, h), (uv.reshape(N, h // 2, w), h // 2)):
            raw = torch.full((guard + N * rows * pitch + guard,), 0xA5, dtype=torch.uint8, device=dev)
            view = raw[guard:guard + N * rows * pitch].view(N, rows, pitch)[:, :, :w]
            view.copy_(plane.to(dev))
            mask = torch.ones_like(raw, dtype=torch.bool)
            mask[guard:guard + N * rows * pitch].view(N, rows, pitch)[:, :, :w] = False
            self.raw.append(raw), self.mask.append(mask), views.append(view)
        self.y, self.uv = views[0], views[1].unflatten(2, (w // 2, 2))
        self.planes = (self.y, self.uv)

    def intact(self):
        return all(bool(torch.all(raw[mask] == 0xA5)) for raw, mask in zip(self.raw, self.mask))


# name -> how the case is made.  ``x``, ``matte``, ``zero``, ``bad``: as tests/blend_cases.py ("small": sigma 2.5 scaled by 0.07, the
# gain meets max_gain); ``surface``: "rgb" (through from_rgb) or "raw"; ``standard`` / ``full``: the colour of the case.
SPECS = {
    "generic 601":      dict(net=(16, 16), which=(0, 1, 2, 3)),
    "wide 709":         dict(net=(12, 20), which=(3, 2, 0), standard="bt709", feather=2.5),
    "full range":       dict(net=(16, 16), which=(0, 1, 2), full=True, matte="shared"),
    "matte frames 709": dict(net=(12, 20), which=(3, 2, 0), standard="bt709", full=True, matte="frames", feather=2.5),
    "raw bytes":        dict(net=(16, 16), which=(0, 2, 3), surface="raw", feather=2.5),
    "gain cap":         dict(net=(16, 16), which=(0, 2, 3), x="small"),
    "constant":         dict(net=(12, 20), which=(0, 2, 3), x="constant"),
    "invalid and zero": dict(net=(16, 16), which=(0, 3, 2, 0), matte="frames", zero=1, bad=2),
}
ROTATED = [k for k, v in SPECS.items() if any(ANGLE_SCALE[i][0] != 0.0 for i in v["which"])]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(x, y, uv, rows, matte, feather, net, colour (keywords standard= / full_range=), by_rule, kind): CPU tensors"""
    spec = SPECS[name]
    seed = 300 + sorted(SPECS).index(name)
    net, which = spec["net"], spec["which"]
    N = len(which)
    kind = spec.get("x", "random")
    if kind == "constant":
        x = torch.tensor([0.2, -0.3, 0.5]).view(1, 3, 1, 1).expand(N, 3, *net).contiguous()
    else:
        x = BC.source(seed, N, *net, sigma=2.5) * 0.07 if kind == "small" else BC.source(seed, N, *net)
    rows = BC.rows_for(which, net)
    if "bad" in spec:
        rows[spec["bad"], 0] = float("nan")
    matte = None
    if spec.get("matte"):
        matte = BC.matte_for(seed + 50, N if spec["matte"] == "frames" else 1, *net)
        if "zero" in spec:
            matte[spec["zero"]] = 0.0
        if spec["matte"] == "shared":
            matte = matte[0]
    colour = dict(standard=spec.get("standard", "bt601"), full_range=spec.get("full", False))
    y, uv = surface_raw(seed + 25, N, H, W) if spec.get("surface") == "raw" else surface_from_rgb(seed + 25, N, H, W, **colour)
    return dict(x=x, y=y, uv=uv, rows=rows, matte=matte, feather=spec.get("feather", 0.0), net=net, colour=colour,
                by_rule=[i for i in (spec.get("zero"), spec.get("bad")) if i is not None], kind=kind)


def model(c, colour_rows=None):
    """``nv12_sim_ref.paste_out`` of a case, with colour rows [N,3,2] or without"""
    to_rgb, from_rgb = coeffs(c["colour"]["standard"], c["colour"]["full_range"])
    return M.paste_out(c["x"].numpy(), c["y"].numpy(), c["uv"].numpy(), c["rows"].numpy(), from_rgb, to_rgb, feather=c["feather"],
                       matte=None if c["matte"] is None else c["matte"].numpy(), colour=colour_rows)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The model of a case without colour rows, and its rows (``blend_ref.colour_rows``): computed once."""
    ref = model(case(name))
    ref["rows"], ref["var_q"], ref["var_b"] = B.colour_rows(ref["sums"], ref["valid"], MAX_GAIN, MIN_SIGMA, MIN_WEIGHT)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref
