"""ResNet-50 trunk encoder -- the module ``IRFD._create_encoder`` builds at ``model.py:60-62``
(``nn.Sequential(*list(resnet50().children())[:-1])``), on the HIP kernels, forward and backward.

``ResNet50Trunk`` IS an ``nn.Sequential`` whose children sit at torchvision's indices (0 conv1,
1 bn1, 2 relu, 3 maxpool, 4-7 layer1..4, 8 avgpool), so its ``state_dict`` keys are the reference's
(``Ei.0.weight``, ``Ei.1.running_mean``, ``Ei.4.0.conv1.weight``, ``Ei.5.0.downsample.0.weight`` ...)
and ``IRFD.apply(_init_weights)`` (model.py:48-54) finds the same ``nn.Conv2d`` modules.  The
children only hold parameters/buffers; ``forward`` runs the whole trunk MI355X-style:

* every conv is one launch of the MFMA implicit-GEMM kernel; its epilogue accumulates the
  BatchNorm batch sums (train mode) -- no statistics pass over the activation;
* BatchNorm + ReLU are never materialised: ``bn_finalize`` turns the sums into a per-channel affine
  that the *consumer* conv (or the max-pool) applies while staging its input;
* only each block's output (bn3 + identity + ReLU) is written, by one HBM-bound pass.

Backward (``TrunkFn``) has the reference's ``torch.utils.checkpoint`` semantics (model.py:84-90): the
forward keeps only the input image; backward re-runs the forward (which, exactly as the reference's
re-entrant checkpoint does, updates the BatchNorm running statistics a second time), then walks the
blocks in reverse: BatchNorm(+ReLU) backward as a two-pass reduce/apply pair on the raw conv output,
data gradients on the forward MFMA kernel with transpose-flipped weights (stride 2: zero-dilated
gradient), weight gradients on the MFMA wgrad kernel with the BatchNorm+ReLU of the input re-formed
in its staging.  The residual sum is folded into the data-gradient epilogue (accumulate flag).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops

LAYERS = (3, 4, 6, 3)
WIDTHS = (64, 128, 256, 512)
EXPANSION = 4



def _wgrad_aside(side, dr, launch):
    """``launch()`` (a weight-gradient launch reading ``dr``) on the stream ``side``, behind everything queued on the current
    stream so far; None: in order on the current stream.  ``dr`` is a temporary of the backward: the allocator must not hand
    its memory out again before the side stream is done with it.  The caller joins ``side`` before it returns gradients."""
    if side is None:
        return launch()
    side.wait_stream(torch.cuda.current_stream(dr.device))
    with torch.cuda.stream(side):
        ops.side_stream_delay()
        dw = launch()
    dr.record_stream(side)
    return dw


class Bottleneck(nn.Module):
    """Parameter holder with torchvision's Bottleneck attribute names (v1.5: stride on conv2)."""

    def __init__(self, inplanes, width, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, width * EXPANSION, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(width * EXPANSION)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, width * EXPANSION, 1, stride=stride, bias=False),
                                            nn.BatchNorm2d(width * EXPANSION))
        self.stride = stride


class _StatsPool:
    """Zeroed fp64 pages per forward, sliced per BatchNorm (a few memsets instead of 53).  ``total`` = the sums of one
    copy of every BatchNorm; the high-resolution layers take several copies (``ops.stats_slots``), so the pool grows by
    pages when the first one is used up."""

    PAGE = 1 << 21               # doubles (16 MiB)

    def __init__(self, device, total):
        self.device = device
        self.buf = torch.zeros(max(total, self.PAGE), device=device, dtype=torch.float64)
        self.pos = 0
        self.counters = []       # num_batches_tracked buffers of the BatchNorms this pass went through

    def take(self, n):
        if self.pos + n > self.buf.numel():
            self.buf = torch.zeros(max(n, self.PAGE), device=self.device, dtype=torch.float64)
            self.pos = 0
        out = self.buf[self.pos:self.pos + n]
        self.pos += n
        return out


_PENDING_BN = "_pending_bn_grads"      # key (never a Parameter) under which per-image BatchNorm gradients wait for their fold


class _ConvBN:
    """The same conv + BatchNorm position of G >= 1 trunks as ONE launch (G > 1: a grouped launch, the channels of the groups
    side by side).  BatchNorm is per channel, so statistics, the folded affine, the residual add, the pools and the BatchNorm
    backward need nothing new for G > 1: they simply see G*C channels.  G = 1 reads and updates the BatchNorm's own tensors;
    G > 1 reads ``flat`` = (gamma, beta, running_mean, running_var) of the G BatchNorms concatenated, provided per pass by
    ``GroupedTrunks``."""

    def __init__(self, members, shared_input=False):
        """``members``: the (conv, bn) pairs of the trunks, repeated once per image.  ``shared_input``: every group reads the
        same input channels."""
        self.convs, self.bns = [c for c, _ in members], [b for _, b in members]
        self.G = len(members)
        self.T = len({id(c) for c in self.convs})        # distinct trunks: the first T members
        self.k, self.stride = self.convs[0].kernel_size[0], self.convs[0].stride[0]
        self.shared_input = shared_input and self.G > 1
        self.packed = ops.PackedConvWeight()
        self.flat = None

    def _weights(self):
        return [c.weight for c in self.convs]

    def _per_trunk(self, t):
        """``t`` (the distinct trunks' parts side by side along dim 0) as one tensor per trunk."""
        return (t,) if self.T == 1 else t.view(self.T, -1, *t.shape[1:]).unbind(0)

    def _bn_tensors(self):
        bn = self.bns[0]
        return self.flat if self.G > 1 else (bn.weight, bn.bias, bn.running_mean, bn.running_var)

    def fwd(self, x, in_affine, training, stats_pool, keep):
        """-> record {y: raw conv output, affine: (scale, shift) its consumer applies, ...}."""
        conv, bn, G = self.convs[0], self.bns[0], self.G
        B, _, H, W = x.shape
        Cin, Cout = conv.in_channels, conv.out_channels
        Ho, Wo = ops.conv_out_size(H, self.k, self.stride), ops.conv_out_size(W, self.k, self.stride)
        cfg = ops.conv2d_pick_config(self.k, self.stride, B, Cin, Cout, Ho, Wo)
        stats = stats_pool.take(ops.stats_slots(cfg, self.k, self.stride, B, Cin, Cout, Ho, Wo) * 2 * G * Cout) if training else None
        y = ops.conv2d_fused(x, self.packed.get(self._weights(), cfg), Cout, self.k, self.stride, in_affine=in_affine,
                             stats=stats, config=cfg, groups=G, shared_input=self.shared_input)
        gamma, beta, rm, rv = self._bn_tensors()
        if training:
            momentum = bn.momentum
            if momentum is None:
                if G > 1:
                    raise NotImplementedError("grouped encoders: cumulative-average BatchNorm (momentum=None) is not supported")
                if bn.num_batches_tracked is not None:
                    bn.num_batches_tracked += 1                  # cumulative average: the count is needed right now
                momentum = 1.0 / float(bn.num_batches_tracked)
            else:
                # distinct counters only; the pass bumps them together at its end, by the number of images it carries
                stats_pool.counters.extend(b.num_batches_tracked for b in self.bns[:self.T] if b.num_batches_tracked is not None)
            fin = ops.bn_finalize(stats, B * Ho * Wo, gamma, beta, rm, rv, momentum, bn.eps, save=keep)
        else:
            fin = ops.bn_finalize(None, 1, gamma, beta, rm, rv, 0.0, bn.eps, save=keep)
        rec = {"y": y, "affine": (fin[0], fin[1])}
        if keep:
            rec.update(x=x, in_affine=in_affine, mean=fin[2], invstd=fin[3], training=training)
            if training:
                rec.update(stats=stats[:2 * G * Cout], count=B * Ho * Wo, momentum=momentum)   # copy 0 = the totals now
        return rec

    def second_update(self, rec, counters, replay):
        """The running-statistics update the reference's re-entrant checkpoint performs a second time when it re-runs
        the forward inside backward (model.py:84-90): same batch sums, same arithmetic, without recomputing the conv.
        Queued on ``replay``: every BatchNorm of the pass is updated by one launch (``ops.bn_replay_running``)."""
        if not rec.get("training") or "stats" not in rec:
            return
        counters.extend(b.num_batches_tracked for b in self.bns[:self.T] if b.num_batches_tracked is not None)
        replay.append((rec["momentum"], rec["stats"], rec["count"], *self._bn_tensors()[2:]))

    def put_bn_grads(self, grads, dg, db):
        if self.G == self.T:
            for bn, g, b in zip(self.bns, self._per_trunk(dg), self._per_trunk(db)):
                grads[bn.weight], grads[bn.bias] = g, b
        else:       # several images per trunk: folded for all layers at once at the end of the pass (flush_bn_grads)
            grads.setdefault(_PENDING_BN, []).append((self, dg, db))

    @staticmethod
    def flush_bn_grads(grads):
        """Sum the per-image BatchNorm gradients of every layer of the pass with ONE concatenation and ONE reduction
        (they were two tiny reductions per layer: 106 launches per pass)."""
        pend = grads.pop(_PENDING_BN, None)
        if not pend:
            return
        imgs = pend[0][0].G // pend[0][0].T
        flat = torch.cat([t.view(imgs, -1) for _, dg, db in pend for t in (dg, db)], 1).sum(0)
        off = 0
        for m, dg, db in pend:
            T, n = m.T, dg.numel() // m.G
            for which in range(2):
                part = flat[off:off + T * n].view(T, n)
                off += T * n
                for q in range(T):
                    bn = m.bns[q]
                    grads[bn.weight if which == 0 else bn.bias] = part[q]

    def bn_bwd(self, rec, g, mask_mode, mask_src=None, want_dz=False, **kw):
        """Gradient w.r.t. the raw conv output + BatchNorm parameter gradients."""
        return ops.bn_backward(g, rec["y"], rec["affine"], rec["mean"], rec["invstd"], mask_mode, mask_src,
                               want_dz=want_dz, batch_stats=rec["training"], **kw)

    def conv_bwd(self, rec, dr, grads, need_dx, dx_out=None, accumulate=False, dilate=True, half=None, side=None):
        """Weight gradients (into ``grads``) and, if asked, the gradient w.r.t. the conv's (staged) input.  ``dilate=False``
        (a strided 1x1): that gradient stays at the conv's output size; ``half``: such a tensor, added at the even pixels."""
        conv, G, T = self.convs[0], self.G, self.T
        Cout, Cin = conv.out_channels, conv.in_channels
        x = rec["x"]
        B, _, H, W = x.shape
        dw = _wgrad_aside(side, dr, lambda: ops.conv2d_wgrad(dr, x, Cout, Cin, self.k, self.stride, in_affine=rec["in_affine"],
                                                             groups=G, shared_input=self.shared_input, fold=G // T))
        for c, dw_q in zip(self.convs, self._per_trunk(dw)):
            grads[c.weight] = dw_q
        if not need_dx:
            return None
        aligned = dr.data_ptr() % 16 == 0 and (dx_out is None or dx_out.data_ptr() % 16 == 0)
        if (self.k == 3 and self.stride == 1 and half is None
                and ops.conv3x3_route(B, Cout, Cin, H, W, precision="f32", groups=G, wino_ok=aligned and not self.shared_input)[0] == "wino"):
            # fp32 Winograd F(2x2, 3x3) data gradient, the G trunks as groups of one launch (ops.CONV3X3_ALGO)
            return ops.conv3x3_wino(dr.contiguous(), self.packed.get_wino(self._weights(), transpose_flip=True), Cin, groups=G,
                                    out=dx_out, accumulate=accumulate)
        cfg, tf = ops.dgrad_plan(self.k, self.stride, B, Cout, Cin, (H, W), dr.shape[-2:], dx_out, accumulate)
        if half is not None and (cfg not in ops.GEMM2_CONFIGS or W % 4):
            dx_out, accumulate, half = ops.dilate2x(half, H, W), True, None     # the form that cannot add it in its epilogue
            cfg, tf = ops.dgrad_plan(self.k, self.stride, B, Cout, Cin, (H, W), dr.shape[-2:], dx_out, accumulate)
        return ops.conv2d_dgrad(dr, self.packed.get(self._weights(), cfg, transpose_flip=tf), Cin, self.k, self.stride,
                                (H, W), cfg, out=dx_out, accumulate=accumulate, groups=G, dilate=dilate, accum_half=half)


class GroupedTrunks:
    """G trunks of one architecture that see the same image -- IRFD's Ei, Ee, Ep (model.py:84-90) -- run as ONE network
    of grouped launches: a third of the launches, three times the work per launch (the 8x8 .. 32x32 layers of a single
    ResNet-50 at batch 8 cannot fill 256 CUs).  Feature order = trunk order: [B, G*2048, 1, 1].  Parameters stay where
    they are (each trunk's own modules, so ``state_dict`` and checkpoints are unchanged); per pass the BatchNorm vectors
    are gathered into flat tensors with four ``torch.cat`` calls and the running statistics written back with two
    ``torch._foreach_copy_`` calls.  One trunk and one image (what ``ResNet50Trunk.forward`` runs) is the plain network:
    every layer reads and updates its BatchNorm directly."""

    def __init__(self, trunks, images=1):
        """``images`` = 2: one pass takes TWO images (``group(x_s, x_t)``): the network then has 2*G groups -- every
        trunk once per image -- so BatchNorm statistics stay per (trunk, image) exactly as in two separate passes (they
        are per channel, and the groups are separate channels); parameter gradients of a trunk's two groups add, and the
        running statistics receive the two momentum updates in the reference's order (x_s, then x_t)."""
        self.trunks = list(trunks)
        self.images = int(images)
        self.groups = len(self.trunks) * self.images
        self._plan = None

    @property
    def recompute(self):
        """See ``TrunkFn``: the trunks' own flag.  Two images per pass keep their activations (a recomputation would replay
        the running-statistics updates in the forward's image order, not the checkpoint's)."""
        return self.images == 1 and all(t.recompute for t in self.trunks)

    @property
    def training(self):
        return self.trunks[0].training

    def train(self, mode=True):
        for t in self.trunks:
            t.train(mode)
        return self

    def parameters(self):
        for t in self.trunks:
            yield from t.parameters()

    # -- launch plan: built lazily so that parameter replacement (.to(), load_state_dict) is honoured
    def _build_plan(self):
        rep = self.images
        stems, blocks = zip(*(t.conv_bn_pairs() for t in self.trunks))
        stem = _ConvBN(list(stems) * rep, shared_input=(rep == 1))
        blocks = [tuple(_ConvBN([b[i] for b in parts] * rep) if parts[0][i] is not None else None for i in range(4))
                  for parts in zip(*blocks)]
        self._stats_total = rep * sum(2 * m.num_features for t in self.trunks for m in t.modules() if isinstance(m, nn.BatchNorm2d))
        self._plan = (stem, blocks)
        self._members = [stem] + [c for blk in blocks for c in blk if c is not None]

    def _load_flats(self):
        ms = self._members
        cat = lambda get: torch.cat([get(bn).detach() for m in ms for bn in m.bns])
        flats = [cat(lambda bn: bn.weight), cat(lambda bn: bn.bias), cat(lambda bn: bn.running_mean), cat(lambda bn: bn.running_var)]
        pos = 0
        for m in ms:
            n = m.G * m.bns[0].num_features
            m.flat = tuple(f[pos:pos + n] for f in flats)
            pos += n
        self._flat_running = (flats[2], flats[3])

    def _store_running(self, first_image_first=True):
        ms = self._members
        sizes = [bn.num_features for m in ms for bn in m.bns]
        for k, get in ((0, lambda bn: bn.running_mean), (1, lambda bn: bn.running_var)):
            parts = list(self._flat_running[k].split(sizes))
            if self.images == 1:
                torch._foreach_copy_([get(bn) for m in ms for bn in m.bns], parts)
                continue
            # Each group's slice holds (1-m)*r0 + m*mu of ITS image, both computed from the same r0.  Two momentum
            # updates in sequence (image a, then image b) give (1-m)*[(1-m)*r0 + m*mu_a] + m*mu_b
            #   = (1-m)*slice_a + slice_b - (1-m)*r0.
            bufs, a, b, pos = [], [], [], 0
            for m in ms:
                T = m.T
                for q in range(T):
                    bufs.append(get(m.bns[q]))
                    s_img, t_img = parts[pos + q], parts[pos + T + q]
                    a.append(s_img if first_image_first else t_img)
                    b.append(t_img if first_image_first else s_img)
                pos += m.G
            keep = 1.0 - ms[0].bns[0].momentum
            torch._foreach_mul_(bufs, -keep)
            torch._foreach_add_(bufs, b)
            torch._foreach_add_(bufs, a, alpha=keep)

    def _run(self, x, keep):
        """Forward; with ``keep`` also returns what backward needs (raw conv outputs, block outputs, statistics)."""
        if self._plan is None:
            self._build_plan()
        if self.groups > 1:
            self._load_flats()
        stem, blocks = self._plan
        training = self.training
        x = x.contiguous()
        pool = _StatsPool(x.device, self._stats_total) if training else None
        s = stem.fwd(x, None, training, pool, keep)
        cur = ops.maxpool3x3s2(s["y"], s["affine"][0], s["affine"][1])      # bn1 + relu folded into the pool's loads
        recs = {"stem": s, "blocks": []} if keep else None
        for c1, c2, c3, down in blocks:
            r1 = c1.fwd(cur, None, training, pool, keep)                      # block input is materialised (post-ReLU)
            r2 = c2.fwd(r1["y"], r1["affine"], training, pool, keep)
            r3 = c3.fwd(r2["y"], r2["affine"], training, pool, keep)
            rd = down.fwd(cur, None, training, pool, keep) if down is not None else None
            a3 = r3["affine"]
            if rd is not None:
                out = ops.bn_add_relu(r3["y"], a3[0], a3[1], rd["y"], rd["affine"][0], rd["affine"][1], relu=True)
            else:
                out = ops.bn_add_relu(r3["y"], a3[0], a3[1], cur, None, None, relu=True)
            if keep:
                recs["blocks"].append((r1, r2, r3, rd, out))
            cur = out
        if pool is not None and pool.counters:
            torch._foreach_add_(pool.counters, self.images)   # 53 one-element kernels -> one fused launch
        feat = ops.global_avgpool(cur)
        if training and self.groups > 1:
            self._store_running()
        return feat, recs

    def _second_bn_update(self, recs):
        if self.groups > 1:
            self._load_flats()
        stem, blocks = self._plan
        counters, replay = [], []
        stem.second_update(recs["stem"], counters, replay)
        for (c1, c2, c3, down), (r1, r2, r3, rd, _) in zip(blocks, recs["blocks"]):
            c1.second_update(r1, counters, replay)
            c2.second_update(r2, counters, replay)
            c3.second_update(r3, counters, replay)
            if down is not None:
                down.second_update(rd, counters, replay)
        for mom in sorted({m for m, *_ in replay}):          # one launch for all BatchNorms (per momentum value: one)
            ops.bn_replay_running([it[1:] for it in replay if it[0] == mom], mom)
        if counters:
            torch._foreach_add_(counters, self.images)
        if self.groups > 1:
            self._store_running(first_image_first=False)     # the checkpoint re-runs the later call (x_t) first

    def _backward(self, recs, dfeat):
        """dfeat [B,G*2048,1,1] -> {parameter: gradient}."""
        side = ops.side_stream(dfeat.device)           # the weight gradients' stream (joined before the gradients are returned)
        if side is not None and torch.cuda.is_current_stream_capturing():
            side = None                                # a stream capture stays on the capturing stream
        stem, blocks = self._plan
        grads = {}
        g, per_plane, g_scale = dfeat.view(dfeat.size(0), -1).contiguous(), True, None
        for (c1, c2, c3, down), (r1, r2, r3, rd, out) in zip(reversed(blocks), reversed(recs["blocks"])):
            if per_plane:                      # last block: gradient of the global average pool, one value per plane
                g_scale = 1.0 / (out.shape[2] * out.shape[3])
            # out = relu(bn3(r3) + identity): mask from the block output; dz also feeds the identity branch
            dr3, dg, db, dz = c3.bn_bwd(r3, g, ops.MASK_TENSOR, mask_src=out, want_dz=True,
                                        g_scale=g_scale if per_plane else 1.0, g_per_plane=per_plane)
            c3.put_bn_grads(grads, dg, db)
            dv2 = c3.conv_bwd(r3, dr3, grads, need_dx=True, side=side)
            dr2, dg, db = c2.bn_bwd(r2, dv2, ops.MASK_RECOMPUTE)
            c2.put_bn_grads(grads, dg, db)
            dv1 = c2.conv_bwd(r2, dr2, grads, need_dx=True, side=side)
            dr1, dg, db = c1.bn_bwd(r1, dv1, ops.MASK_RECOMPUTE)
            c1.put_bn_grads(grads, dg, db)
            if down is None:
                # d(block input) = dz (identity) + conv1's data gradient, summed in the conv epilogue
                g = c1.conv_bwd(r1, dr1, grads, need_dx=True, dx_out=dz, accumulate=True, side=side)
            else:
                drd, dg, db = down.bn_bwd(rd, dz, ops.MASK_NONE)
                down.put_bn_grads(grads, dg, db)
                if down.stride == 2:
                    # the downsample conv reads the even pixels only: its data gradient stays at ITS output size and conv1's
                    # data gradient adds it at the even pixels in its own epilogue -- no dilated copy, no read of one
                    t = down.conv_bwd(rd, drd, grads, need_dx=True, dilate=False, side=side)
                    g = c1.conv_bwd(r1, dr1, grads, need_dx=True, half=t, side=side)
                else:
                    g = down.conv_bwd(rd, drd, grads, need_dx=True, side=side)
                    g = c1.conv_bwd(r1, dr1, grads, need_dx=True, dx_out=g, accumulate=True, side=side)
            per_plane = False
        # stem: max-pool adjoint (bn1+relu re-formed on the fly), BatchNorm backward, 7x7 weight gradient
        s = recs["stem"]
        dv0 = ops.maxpool3x3s2_bwd(s["y"], g, s["affine"][0], s["affine"][1])
        dr0, dg, db = stem.bn_bwd(s, dv0, ops.MASK_RECOMPUTE)
        stem.put_bn_grads(grads, dg, db)
        stem.conv_bwd(s, dr0, grads, need_dx=False, side=side)       # the image itself takes no gradient
        _ConvBN.flush_bn_grads(grads)
        if side is not None:
            torch.cuda.current_stream(dfeat.device).wait_stream(side)     # every weight gradient is complete behind this point
        return grads

    def __call__(self, *xs):
        if len(xs) != self.images:
            raise ValueError(f"GroupedTrunks: expected {self.images} image batch(es), got {len(xs)}")
        # one image: every group reads the same three channels; two: each group gets its own copy (3 channels, negligible)
        x = xs[0] if self.images == 1 else torch.cat([x for x in xs for _ in self.trunks], dim=1)
        return TrunkFn.apply(x, self, torch.is_grad_enabled(), *self.parameters())


class TrunkFn(torch.autograd.Function):
    """The trunks under the reference's ``checkpoint(E, x)`` (model.py:84-90).

    ``trunk.recompute`` True: forward keeps the input only, backward re-runs the forward, then back-propagates -- the
    reference's memory-saving schedule.  False (default here: 288 GB of HBM, ~1 GB of activations per B=8 pass): the
    forward keeps the raw conv outputs, backward uses them directly and replays only the checkpoint's visible side
    effect, the second running-statistics update of every BatchNorm.  Gradients and buffers are identical either way;
    the stored form saves one encoder forward per pass."""

    @staticmethod
    def forward(ctx, x, trunk, grad_mode, *params):
        need = grad_mode and any(ctx.needs_input_grad)
        if need and not trunk.recompute:
            y, ctx.recs = trunk._run(x, keep=True)
            ctx.trunk, ctx.training = trunk, trunk.training
            return y
        y = trunk._run(x, keep=False)[0]
        if need:
            ctx.trunk, ctx.training, ctx.recs = trunk, trunk.training, None
            ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dfeat):
        trunk = ctx.trunk
        if ctx.recs is not None:
            recs, ctx.recs = ctx.recs, None
            if ctx.training:
                trunk._second_bn_update(recs)
        else:
            (x,) = ctx.saved_tensors
            was_training = trunk.training
            trunk.train(ctx.training)
            try:
                _, recs = trunk._run(x, keep=True)          # the checkpoint recomputation
            finally:
                trunk.train(was_training)
        grads = trunk._backward(recs, dfeat.contiguous())
        return (None, None, None) + tuple(grads.get(p) for p in trunk.parameters())


class ResNet50Trunk(nn.Sequential):
    """The parameters of one trunk; ``forward`` runs them as a one-trunk ``GroupedTrunks``."""

    recompute = False        # see TrunkFn: keep activations (default) or re-run the forward inside backward

    def __init__(self):
        layers = []
        inplanes = 64
        for li, (nblk, width) in enumerate(zip(LAYERS, WIDTHS)):
            blocks = []
            for bi in range(nblk):
                blocks.append(Bottleneck(inplanes, width, 2 if (bi == 0 and li > 0) else 1, bi == 0))
                inplanes = width * EXPANSION
            layers.append(nn.Sequential(*blocks))
        super().__init__(nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
                         nn.MaxPool2d(3, stride=2, padding=1), *layers, nn.AdaptiveAvgPool2d(1))
        # torchvision's ResNet.__init__ init: kaiming-normal fan_out convs, BN weight 1 / bias 0
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def conv_bn_pairs(self):
        """-> ((stem conv, bn), [per Bottleneck: (conv1, bn1), (conv2, bn2), (conv3, bn3), downsample pair or None])."""
        blocks = [((b.conv1, b.bn1), (b.conv2, b.bn2), (b.conv3, b.bn3), tuple(b.downsample) if b.downsample is not None else None)
                  for li in range(4) for b in self[4 + li]]
        return (self[0], self[1]), blocks

    def forward(self, x):
        group = self.__dict__.get("_group")        # (not a submodule: it only runs this trunk's own parameters)
        if group is None:
            group = self.__dict__["_group"] = GroupedTrunks([self])
        return group(x)
