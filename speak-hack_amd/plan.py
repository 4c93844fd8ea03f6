"""Launch plans: a module's inference forward as ONE call across the C boundary (include/spk.h, ``spk_launch_list``).

The reference's callers run a decoder pass as one Python call -- ``self.Gd(gen_input)`` at model.py:113-114,
``SynthesisNetwork.forward`` at styleganv1.py:593-610.  Behind that call sit ~25 kernel launches whose descriptors depend
only on (module, batch size, device): tile configs, packed weights, split-K scratch, the intermediate activations.  Issued
one by one, every launch rebuilt its 35-field descriptor and re-queried config / workspace in Python (~50 us each: 5.7 ms
per B=8 step against 3.8 ms of GPU work).  A plan builds all of that ONCE and keeps it; a call patches the handful of
pointers that change (input, explicit noise, the fresh output tensor) and hands the array to ``spk_launch_list`` -- the
same kernels with the same arguments as the one-by-one path.

What a plan owns: the packed conv weights (re-packed in place when a parameter's version counter moves, e.g. after an
optimizer step or ``load_state_dict``), two ping-pong activation buffers (each layer's output is read only by the next
launch, all on one stream), the style / modulation vectors, the noise buffer (one device draw per call, as
``SynthesisNetwork.forward`` does) and the split-K scratch.  The RESULT is a fresh tensor per call, so callers may keep
outputs of earlier calls.  Plans are per (batch, device, stream) and used only when no gradient is required; training
goes through the autograd Functions.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib as L
from . import frames as FR
from . import ops

LRELU = 0.2
FUSE_TORGB = os.environ.get("SPK_FUSE_TORGB", "1") != "0"     # toRGB inside the last Winograd launch's epilogue (SPK_EPI_TORGB)
MAX_PLANS = 4        # per module: (batch, device, stream, entry) combinations kept


def _sig(params):
    return tuple((p.data_ptr(), p._version) for p in params)


class LaunchPlan:
    def __init__(self, device):
        self.device = device
        self.ops = []            # (kind, ctypes struct)
        self.keep = []           # tensors / ctypes arrays the descriptors point into
        self._array = None
        self._refreshers = []    # callables re-deriving plan-owned copies of parameters (packed weights, expanded constants)
        self._params = []
        self._where = []         # per tracked parameter: (module, attribute name) it was found under at build time
        self._stamp = None
        self.captured = False    # a hipGraph recorded this plan's launches: its buffers must outlive the plan cache
        self.ws = None
        self._ws_bytes = 0
        self._up_scratch, self._up_users = None, []   # the x2 image of the Winograd x2 layers (one scratch buffer) and its users

    # ---- building ----------------------------------------------------------------------------------
    def buf(self, *shape):
        t = torch.empty(shape, device=self.device, dtype=torch.float32)
        self.keep.append(t)
        return t

    def add(self, kind, desc):
        self.ops.append((kind, desc))
        return desc

    def track(self, *params):
        self._params.extend(params)

    def conv(self, x, weight, Cout, *, bias=None, noise_w=None, noise=None, style=None, upsample=False, up_fir=False, slope=None,
             out, out_scale=1.0, batch_scale=None, demod=None, act_gain=1.0, precision="f32"):
        """One fused 3x3 stride-1 conv launch on the kernel ``ops.conv3x3_route`` picks for ``precision``, weights packed here."""
        B, Cin, Hs, Ws = x.shape
        H, W = (2 * Hs, 2 * Ws) if upsample else (Hs, Ws)
        kind, cfg = ops.conv3x3_route(B, Cin, Cout, H, W, precision=precision, modulated=batch_scale is not None,
                                      up_w=Ws if upsample else None)
        up_op = None
        if kind == "wino" and upsample and ops.wino_fuse_x2(B, Cin, Cout, H, W, up_fir, modulated=batch_scale is not None):
            pass      # the interpolation is part of the kernel's input transform: the descriptor below carries both flags
        elif kind == "wino" and upsample:
            # the upfirdn2d form, a modulated conv, SPK_WINO_FUSE_X2=0: the layer first writes its upsampled input (one HBM-bound
            # launch: the separate nn.Upsample of styleganv1.py:621,624)
            need = B * Cin * H * W                    # one scratch image for all x2 layers: launches are stream-ordered
            if self._up_scratch is None or self._up_scratch.numel() < need:
                self._up_scratch = self.buf(need)
                for a_, n_ in self._up_users:           # earlier, smaller users move into the larger buffer
                    a_.y = self._up_scratch.data_ptr()
                    n_.x = self._up_scratch.data_ptr()
            xu = self._up_scratch[:need].view(B, Cin, H, W)
            up_op = self.add(L.OP_UPSAMPLE2X, L.Upsample2xArgs(x=x.data_ptr(), y=xu.data_ptr(), planes=B * Cin, Hin=Hs, Win=Ws,
                                                               zero_border=1 if up_fir else 0))
            x, upsample = xu, False
        key = cfg if kind == "direct" else kind
        packed = ops.empty_image(key, Cin, Cout, self.device)
        self.keep.append(packed)
        self._refreshers.append(lambda w=weight, p=packed, k=key: ops.pack_image(w.detach(), k, out=p))
        self.track(weight)
        d, ws_bytes = ops.conv_desc(x, packed, Cout, flags={"wino": L.CONV_WINOGRAD, "bf16x3": L.CONV_BF16X3}.get(kind, 0), out=out,
                                    bias=bias, noise_w=noise_w, noise=noise, style=style, upsample=upsample, up_fir=up_fir,
                                    lrelu_slope=slope, out_scale=out_scale, batch_scale=batch_scale, demod=demod, act_gain=act_gain,
                                    config=cfg)
        self._ws_bytes = max(self._ws_bytes, ws_bytes)      # (plan-wide split-K scratch, attached in ``finish``)
        if up_op is not None:
            self._up_users.append((up_op, d))
        return self.add(L.OP_CONV2D, d)

    def fc(self, x, lin_weight, lin_bias, wmul, bmul, slope, out):
        self.track(lin_weight, *([lin_bias] if lin_bias is not None else []))
        O, I = lin_weight.shape
        return self.add(L.OP_FC, L.FcArgs(x=x.data_ptr(), x_stride=x.stride(0), w=L.dptr(lin_weight, "weight"),
                                           bias=L.dptr(lin_bias, "bias"), out=out.data_ptr(), out_stride=out.stride(0),
                                           B=x.shape[0], I=I, O=O, wmul=float(wmul), bmul=float(bmul), slope=float(slope)))

    def fc_grouped(self, items, B):
        """``items``: (x tensor or None (patched per call), x_stride, weight, bias, wmul, bmul, slope, out)."""
        arr = (L.FcGroup * len(items))()
        for g, (x, xs, weight, bias, wmul, bmul, slope, out) in zip(arr, items):
            self.track(weight, *([bias] if bias is not None else []))
            O, I = weight.shape
            g.x, g.x_stride, g.w, g.bias = (x.data_ptr() if x is not None else None), xs, L.dptr(weight, "weight"), L.dptr(bias, "bias")
            g.out, g.out_stride, g.I, g.O = out.data_ptr(), out.stride(0), I, O
            g.wmul, g.bmul, g.slope = float(wmul), float(bmul), float(slope)
        self.keep.append(arr)
        self.add(L.OP_FC_GROUPED, L.FcGroupedArgs(groups=C.addressof(arr), n_groups=len(items), B=B))
        return arr

    def finish(self, *owners):
        """``owners``: the modules whose parameters the plan reads -- every tracked parameter is looked up in them so that
        ``valid_for`` can tell a re-assigned parameter (``m.weight = nn.Parameter(...)``, ``load_state_dict(assign=True)``, a
        parametrization swap) from the one whose storage the descriptors point at."""
        loc = {}
        for owner in owners:
            for m in owner.modules():
                for n, q in m._parameters.items():
                    if q is not None:
                        loc.setdefault(id(q), (m, n))
        self._where = [loc.get(id(q)) for q in self._params]
        if self._ws_bytes:
            self.ws = self.buf((self._ws_bytes + 3) // 4)
            for kind, d in self.ops:
                if kind == L.OP_CONV2D:
                    d.workspace, d.workspace_bytes = self.ws.data_ptr(), self.ws.numel() * 4
        self._array = (L.Op * len(self.ops))()
        for slot, (kind, d) in zip(self._array, self.ops):
            slot.kind, slot.desc = kind, C.addressof(d)
        self.refresh(force=True)

    # ---- per call ----------------------------------------------------------------------------------
    def refresh(self, force=False):
        """Parameters are read by pointer; what the plan DERIVED from them (packed weights, expanded constants) is rebuilt
        in place when any tracked parameter's version counter moved."""
        stamp = _sig(self._params)
        if force or stamp != self._stamp:
            with torch.no_grad():
                for f in self._refreshers:
                    f()
            self._stamp = stamp

    def valid_for(self):
        """Pointers baked into the descriptors must still be the storage of the parameters the modules hold NOW: the
        tracked Parameter object is still the one registered under its module attribute, and it has not moved."""
        if self._stamp is None:
            return False
        for a, q, w in zip(self._stamp, self._params, self._where):
            if a[0] != q.data_ptr() or (w is not None and w[0]._parameters.get(w[1]) is not q):
                return False
        return True

    def launch(self, kind_mask=L.ALL_OPS):
        L.check(L.lib().spk_launch_list(C.addressof(self._array), len(self.ops), int(kind_mask) & 0xFFFFFFFF, L.stream_ptr()),
                "spk_launch_list")


# ---------------------------------------------------------------------------------------------------------------------
class DecoderPlan(LaunchPlan):
    """``SynthesisNetwork.forward`` (styleganv1.py:593-610), optionally preceded by ``StyleGenerator``'s mapping stack and
    truncation (styleganv1.py:528-543): 8 FC launches (with the mapping), one grouped launch for the 13+ style affines,
    the constant prologue, 2 fused conv launches per block, toRGB.  ``output="uint8"``: the fp32 frame goes to a plan-owned
    buffer and one more op (``SPK_OP_FRAMES_TO_U8``) quantises it from ``value_range`` into the uint8 [B,R,R,3] frames
    ``run`` returns (``swap_rb``: B, G, R order) -- what ``ops.frames_to_u8`` makes of the fp32 result, bit for bit.
    ``output="nv12"``: the same buffer and one ``SPK_OP_FRAMES_TO_NV12`` instead, which converts it from ``value_range`` with the
    colour matrix of ``standard`` / ``full_range`` into the uint8 [B,3R/2,R] NV12 surfaces ``run`` returns -- ``ops.frames_to_nv12``
    of the fp32 result, bit for bit.  ``output="i420"``: one ``SPK_OP_FRAMES_TO_I420`` instead, into packed uint8 [B,3R/2,R] I420
    surfaces -- the ``R`` rows of Y, then the ``R^2 / 4`` bytes of U, then those of V, what ``ops.i420_planes`` takes --
    ``ops.frames_to_i420`` of the fp32 result, bit for bit.  ``output="rgb32"``: one ``SPK_OP_FRAMES_TO_RGB32`` instead, into a contiguous
    uint8 [B,R,R,4] tensor, the colour bytes in the order of ``swap_rb`` behind ``alpha_first`` and the fourth byte ``alpha`` (0 .. 255)
    -- ``ops.frames_to_rgb32`` of the fp32 result, bit for bit.
    ``seeded=True``: the list starts with ``SPK_OP_NOISE_FILL`` (csrc/noise.hip), which writes ``noise_flat`` from the
    ``seed`` / ``frame0`` each ``run`` patches into its descriptor -- the noise of ``ops.decoder_noise``, bit for bit, and the
    forward is the launch list alone (no ATen draw, the device generator untouched).  A seeded plan runs seeded calls only, an
    unseeded one (the default: built and run exactly as before) unseeded calls only.
    ``seeded="rows"``: the first op is ``SPK_OP_NOISE_FILL_ROWS`` instead, whose batch row ``b`` is the noise of ``(seed_rows[b],
    frame_rows[b])``: two device int64 ``[B]`` tables (``ops.noise_fill_rows``) whose pointers each ``run`` patches in -- the noise of
    ``ops.decoder_noise_rows``, bit for bit.  The kernel reads the tables, the host never does.  A rows-seeded plan runs calls with
    tables only, and the other two forms refuse them."""

    def __init__(self, synthesis, B, device, generator=None, precision="f32", output="f32", value_range=(-1, 1), swap_rb=False,
                 seeded=False, standard="bt601", full_range=False, alpha_first=False, alpha=255):
        super().__init__(device)
        if output not in ("f32", "uint8", "nv12", "i420", "rgb32"):
            raise ValueError(f"DecoderPlan: output must be 'f32', 'uint8', 'nv12' or 'i420', got {output!r} (or 'rgb32')")
        if output == "rgb32":
            alpha = FR.rgb32_alpha(alpha, "DecoderPlan")
            if alpha < 0:
                raise ValueError("DecoderPlan: alpha=None keeps the fourth bytes of a frame that exists, and a plan writes new frames")
        elif alpha_first or alpha != 255:
            raise ValueError("DecoderPlan: alpha_first / alpha apply to rgb32 output only")
        s = self.synthesis = synthesis
        self.precision = precision
        self.output = output
        if isinstance(seeded, str) and seeded != "rows":
            raise ValueError(f"DecoderPlan: seeded must be False, True or 'rows', got {seeded!r}")
        self.seed_rows = isinstance(seeded, str)
        self.seeded = bool(seeded) and not self.seed_rows
        self.B, self.with_mapping = B, generator is not None
        mods = [s.style_mod] + [m for layer in s.layers for m in (layer.style_mod1, layer.style_mod2)]
        if len(mods) > L.FC_MAX_GROUPS:
            raise L.SpkError("DecoderPlan: too many style affines for one grouped launch")
        # ---- mapping stack: w512 [B,512]; the truncation scale of rows < cutoff rides on the style FCs' multiplier ----
        psi = [1.0] * len(mods)
        self.feat_fc = None
        if generator is not None:
            w_in = None
            for i, fc in enumerate(generator.mapping):
                out = self.buf(B, fc.weight.shape[0])
                if i == 0:      # input pointer patched per call
                    self.feat_fc = self.add(L.OP_FC, L.FcArgs(x=None, x_stride=fc.weight.shape[1], w=L.dptr(fc.weight, "weight"),
                                                              bias=L.dptr(fc.bias, "bias"), out=out.data_ptr(), out_stride=out.stride(0),
                                                              B=B, I=fc.weight.shape[1], O=fc.weight.shape[0], wmul=float(fc.w_lrmul),
                                                              bmul=float(fc.b_lrmul), slope=LRELU))
                    self.track(fc.weight, fc.bias)
                else:
                    self.fc(w_in, fc.weight, fc.bias, fc.w_lrmul, fc.b_lrmul, LRELU, out)
                w_in = out
            self.w512 = w_in
            if generator.truncation_psi and generator.truncation_cutoff:
                psi = [generator.truncation_psi if j < generator.truncation_cutoff else 1.0 for j in range(len(mods))]
        # ---- the style affines: one grouped launch ----
        self.styles = [self.buf(B, m.linear.weight.shape[0]) for m in mods]
        items = []
        for j, (m, st) in enumerate(zip(mods, self.styles)):
            lin = m.linear
            if generator is not None:      # every row of the broadcast dlatents is w512 (scaled by psi_j)
                items.append((self.w512, self.w512.stride(0), lin.weight, lin.bias, lin.w_lrmul * psi[j], lin.b_lrmul, LRELU, st))
            else:                          # rows of the caller's w [B,L,512]: patched per call
                items.append((None, 0, lin.weight, lin.bias, lin.w_lrmul, lin.b_lrmul, LRELU, st))
        self.style_groups = self.fc_grouped(items, B)
        # ---- noise: one flat buffer, one device draw per call ----
        shapes = s.noise_shapes(B)
        sizes = [sh[0] * sh[2] * sh[3] for sh in shapes]
        self.noise_flat = self.buf(sum(sizes))
        self.noise_views = [t.view(sh) for t, sh in zip(self.noise_flat.split(sizes), shapes)]
        self.noise_fill = None
        if self.seeded:        # the draw is the FIRST op of the list; seed / frame0 / frame_step are patched per call
            self.noise_fill = ops.noise_fill_args(self.noise_flat.data_ptr(), [sh[2] * sh[3] for sh in shapes], B)
            self.ops.insert(0, (L.OP_NOISE_FILL, self.noise_fill))
        elif self.seed_rows:   # the same place in the list; the two table pointers are patched per call
            self.noise_fill = ops.noise_fill_rows_args(self.noise_flat.data_ptr(), [sh[2] * sh[3] for sh in shapes], B)
            self.ops.insert(0, (L.OP_NOISE_FILL_ROWS, self.noise_fill))
        # ---- prologue (styleganv1.py:596-599) ----
        C0 = s.const_input.shape[1]
        pp = [self.buf(B * max(self._act_floats(s)))  for _ in range(2)]
        x = pp[0][:B * C0 * 16].view(B, C0, 4, 4)
        self.track(s.const_input, s.bias, s.noise_input1.weight)
        self.noise_ops = []          # (descriptor, field) whose noise pointer follows an explicit-noise argument
        d = self.add(L.OP_BIAS_NOISE_STYLE, L.BiasNoiseStyleArgs(
            x=L.dptr(s.const_input, "const_input"), x_batch_stride=0 if B > 1 else C0 * 16, bias=L.dptr(s.bias, "bias"),
            noise_w=L.dptr(s.noise_input1.weight, "noise_w"), noise=self.noise_views[0].data_ptr(), style=self.styles[0].data_ptr(),
            style_stride=self.styles[0].stride(0), y=x.data_ptr(), B=B, C=C0, HW=16))
        self.noise_ops.append(d)
        # ---- blocks ----
        cur = 0
        for i, layer in enumerate(s.layers):
            for half, (conv, nmod) in enumerate(((layer.conv1, layer.noise1), (layer.conv2, layer.noise2))):
                Cout = conv.weight.shape[0]
                up = half == 0
                H = x.shape[2] * (2 if up else 1)
                y = pp[1 - cur][:B * Cout * H * H].view(B, Cout, H, H)
                k = 1 + 2 * i + half
                self.track(conv.bias, nmod.weight)
                # the LAST conv (64 channels at full resolution): fp32 Winograd with toRGB in its epilogue beats the bf16x3 kernel + a toRGB pass
                last_conv = i == len(s.layers) - 1 and half == 1 and FUSE_TORGB and Cout <= 64 and s.to_rgb.weight.shape[0] == 3 and \
                    ops.conv3x3_route(B, x.shape[1], Cout, H, H, precision="f32")[0] == "wino" and ops.wino_ksplit(B, x.shape[1], Cout, H, H) == 1
                d = self.conv(x, conv.weight, Cout, bias=conv.bias, noise_w=nmod.weight, noise=self.noise_views[k],
                              style=self.styles[k], upsample=up, slope=LRELU, out=y, precision="f32" if last_conv else precision)
                self.noise_ops.append(d)
                x, cur = y, 1 - cur
        # ---- toRGB (styleganv1.py:607) ----
        self.track(s.to_rgb.weight, s.to_rgb.bias)
        O, Cc = s.to_rgb.weight.shape[:2]
        self.out_shape = (B, O, x.shape[2], x.shape[3])
        last = d                    # the last block's conv2 launch
        self.rgb_fused = None
        if (FUSE_TORGB and O == 3 and Cc <= 64 and (last.flags & L.CONV_WINOGRAD)
                and ops.wino_ksplit(B, last.Cin, Cc, x.shape[2], x.shape[3]) == 1):
            # the 1x1 rides in that launch's epilogue (SPK_EPI_TORGB): the last activation is neither written nor read back
            last.flags |= L.EPI_TORGB
            last.rgb_w, last.rgb_bias, last.rgb_channels = L.dptr(s.to_rgb.weight, "weight"), L.dptr(s.to_rgb.bias, "bias"), 3
            last.y, last.ksplit = None, 1
            self.rgb_fused = last
        else:
            self.torgb = self.add(L.OP_TORGB, L.ToRGBArgs(x=x.data_ptr(), w=L.dptr(s.to_rgb.weight, "weight"), mod=None,
                                                          bias=L.dptr(s.to_rgb.bias, "bias"), skip=None, y=None, B=B, C=Cc, O=O,
                                                          H=x.shape[2], W=x.shape[3], in_scale=1.0))
        self.to_u8 = self.to_nv12 = self.to_i420 = self.to_rgb32 = None
        if output != "f32":
            if O != 3:
                raise L.SpkError(f"DecoderPlan: {output} frames need 3 output channels, toRGB has {O}")
            lo, k = ops.quant_range(value_range)
            self.rgb_buf = self.buf(*self.out_shape)
            if self.rgb_fused is not None:
                self.rgb_fused.rgb_y = self.rgb_buf.data_ptr()
            else:
                self.torgb.y = self.rgb_buf.data_ptr()
        if output in ("nv12", "i420"):
            code, full = FR.yuv_standard(standard, full_range)
            Ho, Wo = x.shape[2], x.shape[3]
            if swap_rb:
                raise ValueError("DecoderPlan: swap_rb applies to uint8 output only")
        if output == "i420":                                              # packed surfaces: a chroma plane is Ho / 2 rows of Wo / 2 bytes
            self.to_i420 = self.add(L.OP_FRAMES_TO_I420, L.FramesToI420Args(
                x=self.rgb_buf.data_ptr(), y=None, u=None, v=None, y_image_stride=3 * Ho // 2 * Wo, y_row_stride=Wo,
                u_image_stride=3 * Ho // 2 * Wo, u_row_stride=Wo // 2, v_image_stride=3 * Ho // 2 * Wo, v_row_stride=Wo // 2, N=B, H=Ho, W=Wo,
                standard=code, full_range=full, lo=lo, k=k, reserved=0))
        if output == "nv12":
            self.to_nv12 = self.add(L.OP_FRAMES_TO_NV12, L.FramesToNv12Args(
                x=self.rgb_buf.data_ptr(), y=None, uv=None, y_image_stride=3 * Ho // 2 * Wo, y_row_stride=Wo, uv_image_stride=3 * Ho // 2 * Wo,
                uv_row_stride=Wo, N=B, H=Ho, W=Wo, standard=code, full_range=full, lo=lo, k=k, reserved=0))
        if output == "uint8":
            self.to_u8 = self.add(L.OP_FRAMES_TO_U8, L.FramesToU8Args(x=self.rgb_buf.data_ptr(), y=None, N=B, H=x.shape[2], W=x.shape[3],
                                                                       swap_rb=1 if swap_rb else 0, lo=lo, k=k))
        if output == "rgb32":                                             # contiguous frames: a row is 4 Wo bytes
            Ho, Wo = x.shape[2], x.shape[3]
            self.to_rgb32 = self.add(L.OP_FRAMES_TO_RGB32, L.FramesToRgb32Args(
                x=self.rgb_buf.data_ptr(), y=None, image_stride=4 * Ho * Wo, row_stride=4 * Wo, N=B, H=Ho, W=Wo, swap_rb=1 if swap_rb else 0,
                alpha_first=1 if alpha_first else 0, alpha=alpha, lo=lo, k=k))
        self.finish(*([synthesis] + ([generator] if generator is not None else [])))

    @staticmethod
    def _act_floats(s):
        """Per-sample float counts of every activation the ping-pong buffers must hold."""
        sizes = [s.const_input.shape[1] * 16]
        res = 4
        for layer in s.layers:
            res *= 2
            sizes.append(layer.out_channels * res * res)
        return sizes

    def run(self, x, noises=None, kind_mask=L.ALL_OPS, *, seed=None, frame0=0, fixed_noise=False, seed_rows=None, frame_rows=None):
        """``x``: features [B,input_dim] (plan built with the generator) or dlatents w [B,L,512].  A seeded plan takes ``seed``
        (0 <= seed < 2**64), ``frame0`` (row b is frame ``frame0 + b``) and ``fixed_noise`` (every row is frame ``frame0``) and
        patches them into the noise op's descriptor, as pointers are patched; ``seed`` together with ``noises`` is a
        ``ValueError``.  A hipGraph capture of a seeded run bakes ``seed`` and ``frame0`` into the graph, as it bakes addresses:
        every replay draws the noise of the captured call.  A rows-seeded plan takes ``seed_rows`` and ``frame_rows`` instead (device
        int64 ``[B]``, as ``ops.noise_fill_rows`` takes them) and nothing else about the noise."""
        if (seed_rows is None) != (frame_rows is None):
            raise ValueError("DecoderPlan.run: seed_rows and frame_rows go together")
        if seed_rows is not None:
            if not self.seed_rows:
                raise ValueError("DecoderPlan.run: seed_rows / frame_rows given to a plan that was not built with seeded='rows'")
            if seed is not None or noises is not None or fixed_noise:
                raise ValueError("DecoderPlan.run: a rows-seeded call takes its noise from the tables alone (no seed, fixed_noise or noises)")
            ops.check_rows_tables("DecoderPlan.run", seed_rows, frame_rows, self.B)
            if seed_rows.device != self.device or frame_rows.device != self.device:
                raise L.SpkError(f"DecoderPlan.run: tables on {seed_rows.device} / {frame_rows.device}, the plan on {self.device}")
        elif self.seed_rows:
            raise ValueError("DecoderPlan.run: a rows-seeded plan needs seed_rows and frame_rows")
        if seed is not None and noises is not None:
            raise ValueError("DecoderPlan.run: pass either seed or noises, not both")
        if self.seeded != (seed is not None):
            raise ValueError("DecoderPlan.run: a seeded plan needs a seed (and no explicit noise)" if self.seeded else
                             "DecoderPlan.run: seed given to an unseeded plan (build it with seeded=True)")
        self.refresh()
        self.captured = self.captured or torch.cuda.is_current_stream_capturing()
        if self.with_mapping:
            if x.dim() != 2 or x.stride(1) != 1:
                raise L.SpkError("DecoderPlan: features must be [B,input_dim] with unit inner stride")
            if not x.is_cuda or x.dtype != torch.float32:
                raise L.SpkError(f"features: expected a float32 HIP tensor, got {x.dtype} on {x.device} (no CPU path)")
            self.feat_fc.x, self.feat_fc.x_stride = x.data_ptr(), x.stride(0)
        else:
            if not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() or x.size(1) < len(self.styles):
                raise L.SpkError("DecoderPlan: w must be a contiguous float32 HIP tensor [B, >= num style layers, 512]")
            base, row, bs = x.data_ptr(), x.stride(1) * 4, x.stride(0)
            for j, g in enumerate(self.style_groups):
                g.x, g.x_stride = base + j * row, bs
        if self.seeded:
            a = self.noise_fill         # (the 13 noise pointers stay on noise_views: a seeded plan never sees explicit noise)
            a.seed, a.frame0 = ops.check_seed(seed, frame0)
            a.frame_step = 0 if fixed_noise else 1
        elif self.seed_rows:
            self.noise_fill.seeds_dev, self.noise_fill.frames_dev = seed_rows.data_ptr(), frame_rows.data_ptr()
        elif noises is None:
            self.noise_flat.normal_()
            for d, nv in zip(self.noise_ops, self.noise_views):
                d.noise = nv.data_ptr()
        else:
            if len(noises) != len(self.noise_ops):
                raise ValueError(f"expected {len(self.noise_ops)} noise tensors, got {len(noises)}")
            for d, nz, nv in zip(self.noise_ops, noises, self.noise_views):
                if nz.numel() != nv.numel():
                    raise L.SpkError(f"noise must be {tuple(nv.shape)}, got {tuple(nz.shape)}")
                d.noise = L.dptr(nz, "noise")
        if self.to_u8 is not None:
            Bo, _, Ho, Wo = self.out_shape
            y = torch.empty((Bo, Ho, Wo, 3), device=self.device, dtype=torch.uint8)
            self.to_u8.y = y.data_ptr()
        elif self.to_nv12 is not None:
            Bo, _, Ho, Wo = self.out_shape
            y = torch.empty((Bo, 3 * Ho // 2, Wo), device=self.device, dtype=torch.uint8)      # packed surfaces: rows Ho.. are the UV plane
            self.to_nv12.y, self.to_nv12.uv = y.data_ptr(), y.data_ptr() + Ho * Wo
        elif self.to_i420 is not None:
            Bo, _, Ho, Wo = self.out_shape
            y = torch.empty((Bo, 3 * Ho // 2, Wo), device=self.device, dtype=torch.uint8)      # packed surfaces: Y rows, then U, then V
            a = self.to_i420
            a.y, a.u, a.v = y.data_ptr(), y.data_ptr() + Ho * Wo, y.data_ptr() + Ho * Wo + Ho * Wo // 4
        elif self.to_rgb32 is not None:
            Bo, _, Ho, Wo = self.out_shape
            y = torch.empty((Bo, Ho, Wo, 4), device=self.device, dtype=torch.uint8)
            self.to_rgb32.y = y.data_ptr()
        else:
            y = torch.empty(self.out_shape, device=self.device, dtype=torch.float32)
            if self.rgb_fused is not None:
                self.rgb_fused.rgb_y = y.data_ptr()
            else:
                self.torgb.y = y.data_ptr()
        self.launch(kind_mask)
        return y


_retired = []        # plans a hipGraph has recorded, dropped from their cache: kept alive (the graph holds raw addresses)


def _drop(plan):
    if plan is not None and plan.captured:
        _retired.append(plan)


def plan_for(owner, key, build):
    """Per-module plan cache (``owner.__dict__['_plans']``): at most MAX_PLANS entries, least recently used dropped; an
    entry whose baked parameter pointers went stale (``.to()``, re-assigned parameters) is rebuilt.  A plan whose launches
    were recorded into a hipGraph is never freed when it leaves the cache -- its packed weights, activation and noise
    buffers stay where the graph's kernels will read and write them (as ``ops._workspace`` retires outgrown scratch).  Such
    a graph replays the weights as they were packed at ITS capture: re-capture after an optimizer step."""
    cache = owner.__dict__.setdefault("_plans", {})
    key = key + (ops.CONV3X3_ALGO, ops.WINO_FUSE_X2)
    plan = cache.pop(key, None)
    if plan is None or not plan.valid_for():
        _drop(plan)
        plan = build()
        if torch.cuda.is_current_stream_capturing():
            # built inside a stream capture: its buffers belong to that graph's memory pool and its packing launches were
            # recorded into the graph -- correct, but not something to keep for later eager calls.  Warm the stream up
            # before capturing (as bench.py does) to capture a plain launch list.
            return plan
    cache[key] = plan                      # re-insert: most recently used last
    while len(cache) > MAX_PLANS:
        _drop(cache.pop(next(iter(cache))))
    return plan


class StyleGAN2Plan(LaunchPlan):
    """Inference forward of the build-defined StyleGAN2 variant (stylegan2.StyleGAN2Generator): PixelNorm, the 8-layer
    style MLP, every modulation affine in two grouped launches, the 13 demodulation vectors in one, then per resolution
    two modulated MFMA convs (upfirdn2d x2 folded into the first one's staging) and ONE toRGB launch that also upsamples
    and adds the skip image."""

    def __init__(self, gen, B, device, precision="f32"):
        super().__init__(device)
        from .stylegan2 import SQRT2, StyledConv
        self.B = B
        self.precision = precision
        # ---- PixelNorm + style MLP ----
        self.pn = self.add(L.OP_PIXELNORM, L.PixelNormArgs(x=None, y=None, B=B, C=gen.input_dim, HW=1, eps=1e-8, sqrt_form=0))
        wn = self.buf(B, gen.input_dim)
        self.pn.y = wn.data_ptr()
        w = wn
        for lin in gen.style:
            out = self.buf(B, lin.weight.shape[0])
            if lin.activation:
                self.fc(w, lin.weight, lin.bias, lin.scale * SQRT2, lin.lr_mul * SQRT2, 0.2, out)
            else:
                self.fc(w, lin.weight, lin.bias, lin.scale, lin.lr_mul, 1.0, out)
            w = out
        # ---- modulations (every one is an affine of the same w) and demodulation vectors ----
        layers = [gen.conv1, gen.to_rgb1] + [m for i in range(len(gen.to_rgbs)) for m in (gen.convs[2 * i], gen.convs[2 * i + 1], gen.to_rgbs[i])]
        mods = [m.conv.modulation for m in layers]
        svec = [self.buf(B, m.weight.shape[0]) for m in mods]
        items = [(w, w.stride(0), m.weight, m.bias, m.scale, m.lr_mul, 1.0, s) for m, s in zip(mods, svec)]
        for k in range(0, len(items), L.FC_MAX_GROUPS):
            self.fc_grouped(items[k:k + L.FC_MAX_GROUPS], B)
        s_of = {id(m): s for m, s in zip(layers, svec)}
        styled = [m for m in layers if isinstance(m, StyledConv)]
        dvec = {id(m): self.buf(B, m.conv.out_channel) for m in styled}
        for k in range(0, len(styled), L.DEMOD_MAX_GROUPS):
            part = styled[k:k + L.DEMOD_MAX_GROUPS]
            arr = (L.DemodGroup * len(part))()
            for q, m in zip(arr, part):
                wt = m.conv.weight
                self.track(wt)
                # d[b,co] = rsqrt(scale^2 sum_ci s^2 (sum_k w^2) + eps): the tap sum depends on the weights only, so the plan
                # keeps n[co,ci] = sqrt(sum_k w[co,ci,k]^2) (refreshed with the parameter) and the demodulation launch reads
                # it as a one-tap kernel -- a ninth of the bytes of the 3x3 weights on every call
                wn = self.buf(wt.shape[0], wt.shape[1])
                self._refreshers.append(lambda src=wt, dst=wn: torch.sqrt(src.detach().pow(2).sum((2, 3)), out=dst))
                q.w, q.s, q.d = wn.data_ptr(), s_of[id(m)].data_ptr(), dvec[id(m)].data_ptr()
                q.Cin, q.Cout, q.taps, q.scale = wt.shape[1], wt.shape[0], 1, float(m.conv.scale)
            self.keep.append(arr)
            self.add(L.OP_DEMOD_GROUPED, L.DemodGroupedArgs(groups=C.addressof(arr), n_groups=len(part), B=B, eps=1e-8))
        # ---- noise ----
        shapes = [(B, 1, 4, 4)] + [(B, 1, 8 << i, 8 << i) for i in range(len(gen.to_rgbs)) for _ in range(2)]
        sizes = [sh[0] * sh[2] * sh[3] for sh in shapes]
        self.noise_flat = self.buf(sum(sizes))
        self.noise_views = [t.view(sh) for t, sh in zip(self.noise_flat.split(sizes), shapes)]
        self.noise_ops = []
        # ---- constant input, expanded over the batch (plan-owned copy, refreshed with the parameter) ----
        cin = gen.input.input
        x = self.buf(B, cin.shape[1], cin.shape[2], cin.shape[3])
        self._refreshers.append(lambda src=cin, dst=x: dst.copy_(src.detach().expand_as(dst)))
        self.track(cin)
        res_max = 4 << len(gen.to_rgbs)
        act = max([cin.shape[1] * 16] + [m.conv.out_channel * (8 << (i // 2)) ** 2 for i, m in enumerate(gen.convs)])
        pp = [self.buf(B * act) for _ in range(2)]
        cur = 0

        def styled_conv(m, x, k, cur):
            Cout = m.conv.out_channel
            H = x.shape[2] * (2 if m.upsample else 1)
            y = pp[cur][:B * Cout * H * H].view(B, Cout, H, H)
            nw = self.buf(Cout)                                   # the scalar noise weight, one copy per output channel
            self._refreshers.append(lambda src=m.noise.weight, dst=nw: dst.copy_(src.detach().expand_as(dst)))
            self.track(m.noise.weight, m.activate.bias)
            d = self.conv(x, m.conv.weight, Cout, bias=m.activate.bias, noise_w=nw, noise=self.noise_views[k], upsample=m.upsample,
                          up_fir=True, slope=0.2, out=y, out_scale=m.conv.scale, batch_scale=s_of[id(m)], demod=dvec[id(m)],
                          act_gain=SQRT2, precision=precision)
            self.noise_ops.append(d)
            return y

        def to_rgb(m, x, skip, y):
            wt = m.conv.weight
            self.track(wt, m.bias)
            return self.add(L.OP_TORGB, L.ToRGBArgs(x=x.data_ptr(), w=L.dptr(wt.reshape(wt.shape[0], wt.shape[1]), "weight"),
                                                    mod=s_of[id(m)].data_ptr(), bias=L.dptr(m.bias.view(-1), "bias"),
                                                    skip=skip.data_ptr() if skip is not None else None,
                                                    y=y.data_ptr() if y is not None else None, B=B, C=wt.shape[1], O=wt.shape[0],
                                                    H=x.shape[2], W=x.shape[3], in_scale=float(m.conv.scale)))

        x = styled_conv(gen.conv1, x, 0, cur)
        skip = self.buf(B, 3, 4, 4)
        self.torgb = to_rgb(gen.to_rgb1, x, None, skip if gen.to_rgbs else None)
        for i, rgb in enumerate(gen.to_rgbs):
            cur ^= 1
            x = styled_conv(gen.convs[2 * i], x, 1 + 2 * i, cur)
            cur ^= 1
            x = styled_conv(gen.convs[2 * i + 1], x, 2 + 2 * i, cur)
            last = i == len(gen.to_rgbs) - 1
            nxt = None if last else self.buf(B, 3, x.shape[2], x.shape[3])
            self.torgb = to_rgb(rgb, x, skip, nxt)
            skip = nxt
        self.out_shape = (B, 3, x.shape[2], x.shape[3])
        assert x.shape[2] == res_max
        self.finish(gen)

    def run(self, features, noises=None, kind_mask=L.ALL_OPS):
        self.refresh()
        self.captured = self.captured or torch.cuda.is_current_stream_capturing()
        self.pn.x = L.dptr(features, "features")
        if noises is None:
            self.noise_flat.normal_()
            for d, nv in zip(self.noise_ops, self.noise_views):
                d.noise = nv.data_ptr()
        else:
            if len(noises) != len(self.noise_ops):
                raise ValueError(f"expected {len(self.noise_ops)} noise tensors, got {len(noises)}")
            for d, nz, nv in zip(self.noise_ops, noises, self.noise_views):
                if nz.numel() != nv.numel():
                    raise L.SpkError(f"noise must be {tuple(nv.shape)}, got {tuple(nz.shape)}")
                d.noise = L.dptr(nz, "noise")
        y = torch.empty(self.out_shape, device=self.device, dtype=torch.float32)
        self.torgb.y = y.data_ptr()
        self.launch(kind_mask)
        return y


# ---------------------------------------------------------------------------------------------------------------------
def fold_conv_bn(weight, gamma, beta, running_mean, running_var, eps):
    """Eval-mode BatchNorm folded into the conv that feeds it: ``bn(conv(x, w)) == conv(x, w') + b'`` with
    ``s = gamma * rsqrt(running_var + eps)``, ``w' = w * s[co]``, ``b' = beta - running_mean * s``.  Pure torch in the
    tensors' own dtype and device (CPU tensors too) -> (w', b')."""
    s = gamma * torch.rsqrt(running_var + eps)
    return weight * s.view(-1, 1, 1, 1), beta - running_mean * s


class EncoderPlan(LaunchPlan):
    """One ``ResNet50Trunk`` (model.py:60-62) at one (B, H, W, device) in the reference's EVAL arithmetic -- running
    statistics in every BatchNorm, no buffer updated -- as one launch list of 55 ops.  In eval a BatchNorm is a constant
    per-channel affine, so it is folded into the weights and a bias (``fold_conv_bn``; the module's own parameters are left
    alone) and every activation is materialised post-ReLU: a plain input for every conv, hence Winograd for the 3x3 stride-1
    ones where ``ops.conv3x3_route`` picks it.  Stem 7x7 s2 (bias + ReLU) -> max-pool -> per Bottleneck conv1 1x1 (bias +
    ReLU), conv2 3x3 (bias + ReLU), downsample 1x1 (bias) on the first block of a layer, conv3 1x1 with
    ``relu(. + bias + identity)`` in its epilogue (``SPK_EPI_RESIDUAL``) -> global average pool.  The plan owns the folded,
    packed weights (re-derived when a conv weight, a BatchNorm parameter or a running statistic changes) and its activation
    buffers; a call allocates the returned features only."""

    def __init__(self, trunk, B, H, W, device):
        super().__init__(device)
        self.trunk, self.B, self.H, self.W = trunk, B, H, W
        size = ops.conv_out_size
        (conv0, bn0), blocks = trunk.conv_bn_pairs()
        # ---- shapes first: five buffers by role, each as large as its largest user ----
        H1, W1 = size(H, 7, 2), size(W, 7, 2)
        Hp, Wp = (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1
        need = {"stem": B * conv0.out_channels * H1 * W1, "io": B * conv0.out_channels * Hp * Wp, "t1": 0, "t2": 0, "down": 0}
        h, w = Hp, Wp
        for (c1, _), (c2, _), (c3, _), down in blocks:
            s = c2.stride[0]
            ho, wo = size(h, 3, s), size(w, 3, s)
            need["t1"] = max(need["t1"], B * c1.out_channels * h * w)
            need["t2"] = max(need["t2"], B * c2.out_channels * ho * wo)
            need["io"] = max(need["io"], B * c3.out_channels * ho * wo)
            if down is not None:
                need["down"] = max(need["down"], B * c3.out_channels * ho * wo)
            h, w = ho, wo
        stem_buf, t1_buf, t2_buf, down_buf = (self.buf(need[k]) for k in ("stem", "t1", "t2", "down"))
        pp = [self.buf(need["io"]) for _ in range(2)]          # block inputs / outputs ping-pong (the input is the residual)

        def view(buf, Cc, hh, ww):
            return buf[:B * Cc * hh * ww].view(B, Cc, hh, ww)

        # ---- ops ----
        x0 = torch.empty((B, 3, H, W), device=device, dtype=torch.float32)   # shape carrier; the input pointer is patched per call
        y = view(stem_buf, conv0.out_channels, H1, W1)
        self.stem = self.folded_conv(x0, conv0, bn0, y, relu=True)
        cur = view(pp[0], conv0.out_channels, Hp, Wp)
        self.add(L.OP_MAXPOOL3X3S2, L.MaxPool3x3s2Args(x=y.data_ptr(), in_scale=None, in_shift=None, y=cur.data_ptr(), B=B,
                                                        C=conv0.out_channels, Hin=H1, Win=W1))
        side = 0
        for (c1, b1), (c2, b2), (c3, b3), down in blocks:
            h, w = cur.shape[2:]
            s = c2.stride[0]
            ho, wo = size(h, 3, s), size(w, 3, s)
            t1 = view(t1_buf, c1.out_channels, h, w)
            self.folded_conv(cur, c1, b1, t1, relu=True)
            t2 = view(t2_buf, c2.out_channels, ho, wo)
            self.folded_conv(t1, c2, b2, t2, relu=True)
            identity = cur
            if down is not None:
                identity = view(down_buf, c3.out_channels, ho, wo)
                self.folded_conv(cur, down[0], down[1], identity, relu=False)
            out = view(pp[1 - side], c3.out_channels, ho, wo)
            self.folded_conv(t2, c3, b3, out, relu=True, residual=identity)
            cur, side = out, 1 - side
        self.feat_shape = (B, cur.shape[1], 1, 1)
        self.avg = self.add(L.OP_GLOBAL_AVGPOOL, L.GlobalAvgPoolArgs(x=cur.data_ptr(), y=None, planes=B * cur.shape[1],
                                                                     HW=cur.shape[2] * cur.shape[3]))
        self.finish(trunk)

    def folded_conv(self, x, conv, bn, out, *, relu, residual=None):
        """One conv launch on BatchNorm-folded weights: ``out = [relu](conv(x, w') + b' [+ residual])``."""
        B, Cin, Hs, Ws = x.shape
        Cout, k, stride = conv.out_channels, conv.kernel_size[0], conv.stride[0]
        H, W = out.shape[2:]
        if k == 3 and stride == 1:
            kind, cfg = ops.conv3x3_route(B, Cin, Cout, H, W, precision="f32")
        else:
            kind, cfg = "direct", ops.conv2d_pick_config(k, stride, B, Cin, Cout, H, W)
        key = cfg if kind == "direct" else kind
        n = L.lib().spk_conv2d_packed_bytes_wino(Cin, Cout) // 4 if kind == "wino" else L.lib().spk_conv2d_packed_floats(cfg, k, k, Cin, Cout)
        if n <= 0:
            raise L.SpkError(f"EncoderPlan: config {cfg} packs no {k}x{k} kernel of {Cin} -> {Cout} channels")
        packed, bias = self.buf(n), self.buf(Cout)
        tracked = [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        if bn.num_batches_tracked is not None:
            # a training forward of the trunk writes the running statistics from inside a kernel (no version bump); its
            # counter update is a torch op, so the counter's version tells
            tracked.append(bn.num_batches_tracked)

        def refresh(conv=conv, bn=bn, packed=packed, bias=bias, key=key):
            wf, bf = fold_conv_bn(conv.weight.detach(), bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)
            bias.copy_(bf)
            ops.pack_image(wf.contiguous(), key, out=packed)

        self._refreshers.append(refresh)
        self.track(*tracked)
        d, ws_bytes = ops.conv_desc(x, packed, Cout, k, stride, flags=L.CONV_WINOGRAD if kind == "wino" else 0, out=out, bias=bias,
                                    lrelu_slope=0.0 if relu else None, residual=residual, config=cfg)
        self._ws_bytes = max(self._ws_bytes, ws_bytes)
        return self.add(L.OP_CONV2D, d)

    def run(self, images, kind_mask=L.ALL_OPS):
        """images [B,3,H,W] -> features [B,2048,1,1] (a fresh tensor)."""
        if tuple(images.shape) != (self.B, 3, self.H, self.W):
            raise ValueError(f"EncoderPlan: built for {(self.B, 3, self.H, self.W)}, got {tuple(images.shape)}")
        self.refresh()
        self.captured = self.captured or torch.cuda.is_current_stream_capturing()
        images = images.contiguous()
        self.stem.x = L.dptr(images, "images")
        y = torch.empty(self.feat_shape, device=self.device, dtype=torch.float32)
        self.avg.y = y.data_ptr()
        self.launch(kind_mask)
        return y
