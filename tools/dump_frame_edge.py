"""Every output byte of the aligned video edge for one build of the tree, on the GPU -- both ways in, both pastes, the colour
statistics of both pixel formats, one ``reenact_video(align=, paste=True, matte=, colour_match=True, colour_smooth=2)`` and one
``LiveSession.step`` in two steps -- as raw bytes in one .npz.  Two builds whose files are equal array for array compute the same
thing on every case below.  Only ``ops.*`` / ``IRFD`` calls, so the same file runs against any commit that has them.

    python tools/dump_frame_edge.py --out new.npz
    python tools/dump_frame_edge.py --compare old.npz new.npz

The cases are those of the tests: every case of tests/blend_cases.py (40 x 56 packed frames) and tests/nv12_sim_cases.py (40 x 56
surfaces: on a pitched surface, as a packed ``[N,3H/2,W]`` buffer and as a pair of planes), each at feather 0 and 2.5, without a matte
and colour rows, with the case's matte (shared or per frame; without one, a shared ellipse), and with colour rows; the rows of
tests/test_align_gpu.py -- rotation, s < 1, s > 2, the identity, regions that leave the frame, a NaN row and a row with s = 100 from the
device -- on 40 x 56 and 64 x 80 frames, images 16 x 16 and 12 x 20, both channel orders, a strided slice at an odd address; and the
recipe-weight model of the model-level tests (128 -> 256 pixels)."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FEATHERS = (0, 2.5)


def raw(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().copy()


def dump_rgb(ops, dev, out):
    import blend_cases as BC
    import sim_ref as R
    for name in BC.SPECS:
        c = BC.case(name)
        order = dict(channel_order="bgr" if c["bgr"] else "rgb")
        x, rows = c["x"].to(dev), c["rows"].to(dev) if c["by_rule"] else c["rows"]
        bg = c["bg"].to(dev)
        if name == "strided":                                              # every other frame of a larger buffer, at an odd address
            big = BC.frames(77, 2 * bg.size(0), BC.H + 9, BC.W + 13, 3).to(dev)
            big[::2, 4:4 + BC.H, 5:5 + BC.W] = bg
            bg = big[::2, 4:4 + BC.H, 5:5 + BC.W]
        matte = c["matte"].to(dev) if c["matte"] is not None else ops.ellipse_matte(c["net"], device=dev)
        out[f"rgb/{name}/in"] = raw(ops.frames_from_u8_aligned(bg, c["net"], rows, **order))
        for f in FEATHERS:
            kw = dict(feather=f, **order)
            colour = ops.paste_colour_match(x, bg, rows, matte=matte, **kw)
            out[f"rgb/{name}/f{f}/match"] = raw(colour)
            out[f"rgb/{name}/f{f}/match_plain"] = raw(ops.paste_colour_match(x, bg, rows, **kw))
            out[f"rgb/{name}/f{f}/sums"] = raw(ops.paste_colour_sums(x, bg, rows, matte=matte, **kw))
            out[f"rgb/{name}/f{f}/sums_plain"] = raw(ops.paste_colour_sums(x, bg, rows, **kw))
            out[f"rgb/{name}/f{f}/paste"] = raw(ops.frames_paste_u8_aligned(x, bg, rows, **kw))
            out[f"rgb/{name}/f{f}/paste_matte"] = raw(ops.frames_paste_u8_aligned(x, bg, rows, matte=matte, **kw))
            out[f"rgb/{name}/f{f}/paste_colour"] = raw(ops.frames_paste_u8_aligned(x, bg, rows, colour=colour, **kw))
            out[f"rgb/{name}/f{f}/paste_both"] = raw(ops.frames_paste_u8_aligned(x, bg, rows, matte=matte, colour=colour, **kw))
            if name == "strided":                                          # in place through the strides: the whole buffer
                whole = big.clone()
                part = whole[::2, 4:4 + BC.H, 5:5 + BC.W]
                ops.frames_paste_u8_aligned(x, part, rows, out=part, **kw)
                out[f"rgb/{name}/f{f}/paste_in_place"] = raw(whole)
    # the rows of tests/test_align_gpu.py on two frame sizes: regions and footprints that leave the frame, invalid device rows
    for (H, W) in ((BC.H, BC.W), (64, 80)):
        for net in BC.NETS:
            leaving = torch.tensor([R.rows((H - 4.9, W - 5.7), 1.3 * net[1], 2.0, net), R.rows((2.2, 3.9), 2.3 * net[1], -0.4, net),
                                    R.rows((20.2, W + 34.4), 1.0 * net[1], 0.3, net), R.rows((20.3, 27.6), 1.25 * net[1], 0.3, net),
                                    R.rows((20.3, 27.6), 1.25 * net[1], 0.3, net)], dtype=torch.float64).float()
            leaving[3, 0] = float("nan")
            leaving[4, :2] = torch.tensor([0.0, 100.0])
            for tag, rows in (("rows", BC.rows_for((0, 1, 2, 3), net)), ("leaving", leaving.to(dev))):
                N = rows.size(0)
                u8, x = BC.frames(H + net[1], N, H, W, 3).to(dev), BC.source(W + net[0], N, *net).to(dev)
                for order in ("rgb", "bgr"):
                    key = f"align/{H}x{W}/{net[0]}x{net[1]}/{tag}/{order}"
                    out[f"{key}/in"] = raw(ops.frames_from_u8_aligned(u8, net, rows, channel_order=order, mean=(0.4, 0.5, 0.6), std=(0.2, 0.25, 0.5)))
                    for f in FEATHERS:
                        out[f"{key}/f{f}/paste"] = raw(ops.frames_paste_u8_aligned(x, u8, rows, feather=f, channel_order=order))


def dump_nv12(ops, dev, out):
    import nv12_sim_cases as NC
    for name in NC.SPECS:
        c = NC.case(name)
        x, rows = c["x"].to(dev), c["rows"].to(dev) if c["by_rule"] else c["rows"]
        matte = c["matte"].to(dev) if c["matte"] is not None else ops.ellipse_matte(c["net"], device=dev)
        N = x.size(0)
        packed = torch.cat([c["y"], c["uv"].reshape(N, NC.H // 2, NC.W)], 1).to(dev)
        forms = {"pitched": lambda: NC.Pitched(c["y"], c["uv"], dev).planes, "packed": lambda: packed.clone(),
                 "pair": lambda: (c["y"].to(dev), c["uv"].to(dev))}
        for form, make in forms.items():
            src = make()
            for order in ("rgb", "bgr"):
                out[f"nv12/{name}/{form}/in_{order}"] = raw(ops.frames_from_nv12_aligned(src, c["net"], rows, channel_order=order, **c["colour"]))
            for f in FEATHERS:
                kw = dict(feather=f, **c["colour"])
                key = f"nv12/{name}/{form}/f{f}"
                colour = ops.paste_colour_match_nv12(x, src, rows, matte=matte, **kw)
                out[f"{key}/match"] = raw(colour)
                out[f"{key}/match_plain"] = raw(ops.paste_colour_match_nv12(x, src, rows, **kw))
                out[f"{key}/sums"] = raw(ops.paste_colour_sums_nv12(x, src, rows, matte=matte, **kw))
                out[f"{key}/sums_plain"] = raw(ops.paste_colour_sums_nv12(x, src, rows, **kw))
                for tag, blend in (("paste", {}), ("paste_matte", dict(matte=matte)), ("paste_colour", dict(colour=colour)),
                                   ("paste_both", dict(matte=matte, colour=colour))):
                    out[f"{key}/{tag}"] = raw(ops.frames_paste_nv12_aligned(x, src, rows, **blend, **kw))
            if form == "pitched":                                          # in place through the pitch
                dst = make()
                ops.frames_paste_nv12_aligned(x, dst, rows, feather=2.5, matte=matte, out=dst, **c["colour"])
                out[f"nv12/{name}/{form}/paste_in_place_y"], out[f"nv12/{name}/{form}/paste_in_place_uv"] = raw(dst[0]), raw(dst[1])


def dump_model(ops, dev, out):
    import blend_cases as BC
    import landmark_ref as LR
    import model
    from oracle import irfd_ref as IR
    from oracle.weights_recipe import fill_state_dict
    m = model.IRFD()
    sd = IR.irfd_recipe_state_dict()
    sd.update({"Gd." + k: v for k, v in fill_state_dict(m.Gd.state_dict(), prefix="Gd.").items()})
    m.load_state_dict(sd, strict=False)
    m = m.to(dev).eval()
    size, T = 128, 3
    template, contour = [(44.0, 52.0), (84.0, 52.0), (64.0, 74.0), (48.0, 96.0), (80.0, 96.0)], [0, 1, 4, 3]
    ident, pose = BC.frames(31, 56, 72, 3).to(dev), BC.frames(32, T, 64, 80, 3).to(dev)
    rows = ops.similarity_rows([(30.3, 41.6), (33.9, 38.2), (28.4, 44.1)], [44.0, 52.0, 36.0], [0.2, -0.3, 0.1], size)
    matte = ops.ellipse_matte((256, 256), device=dev)
    out["model/reenact_video"] = raw(m.reenact_video(ident, pose, size=size, align=rows, channel_order="bgr", paste=True, feather=4, seed=7,
                                                     chunk=2, matte=matte, colour_match=True, colour_smooth=2))
    lm = torch.from_numpy((LR.apply(rows.numpy(), template) + np.random.default_rng(23).standard_normal((T, 5, 2)) / 3).astype(np.float32)).to(dev)
    s = m.live(ident, size=size, template=template, contour=contour, channel_order="bgr", track=dict(hold=2, beta=0.1),
               features=dict(hold=2, min_cutoff=2.0), feather=4, colour_match=True, colour_decay=0.8, seed=7, matte_softness=6.0, matte_grow=3.0)
    out["model/live_step"] = raw(torch.cat([s.step(pose[:1], lm[:1]), s.step(pose[1:], lm[1:])]))
    for n, state in (("lm", s.lm_state), ("feature", s.feature_state), ("colour", s.colour_state)):
        out[f"model/live_{n}_state"] = raw(state)


def compare(old_path, new_path):
    old, new = np.load(old_path), np.load(new_path)
    assert sorted(old.files) == sorted(new.files), sorted(set(old.files) ^ set(new.files))
    differ = [k for k in old.files if not np.array_equal(old[k], new[k])]
    print(f"{len(old.files)} arrays, {sum(old[k].size for k in old.files)} bytes compared: {len(differ)} differ")
    if differ:
        sys.exit("\n".join(differ))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", metavar="FILE.npz")
    ap.add_argument("--compare", nargs=2, metavar=("OLD", "NEW"))
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare)
    else:
        if not args.out:
            ap.error("--out FILE.npz or --compare OLD NEW")
        pkg = importlib.import_module("speak-hack_amd")
        pkg._lib.lib()
        dev, arrays = torch.device("cuda:0"), {}
        with torch.no_grad():
            dump_rgb(pkg.ops, dev, arrays)
            dump_nv12(pkg.ops, dev, arrays)
            dump_model(pkg.ops, dev, arrays)
        np.savez(args.out, **arrays)
        print(f"{args.out}: {len(arrays)} arrays, {sum(a.size for a in arrays.values())} bytes")
