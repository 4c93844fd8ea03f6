"""``IRFD.live``: a reenactment SESSION for a feed whose next frame does not exist yet -- a camera, a call, or a long video pushed
through a few frames at a time.  ``IRFD.reenact_video`` takes a clip that is in memory: it runs ``Ei`` on every call and smooths the
landmarks, the matte's contour and the colour statistics with windows over frames ``t - r ... t + r``.  A session runs ``Ei`` once,
keeps ``fi``, and steadies the same three things with the causal filters of csrc/causal_filter.hip, whose state lives in device
tensors on the session: ``step`` reads no device value on the host, and ``N`` frames in one ``step`` and the same frames in any split
of steps give the same bytes.  Packed RGB only; a session over NV12 surfaces is a follow-up."""
from __future__ import annotations

import torch

from . import _lib as L
from . import frames as FR


def _filter_params(what, name, params, group, rate):
    """``track=`` / ``features=``: None, or a dict over the keys of ``frames.FILTER_DEFAULTS`` -> None, or the keywords of
    ``causal_filter`` checked on the host"""
    if params is None:
        return None
    if not isinstance(params, dict) or set(params) - set(FR.FILTER_DEFAULTS):
        raise ValueError(f"{what}: {name} must be None or a dict over {sorted(FR.FILTER_DEFAULTS)}, got {params!r}")
    p = dict(FR.FILTER_DEFAULTS)
    p.update(params)
    group, rate, p["min_cutoff"], p["beta"], p["d_cutoff"], p["hold"] = FR.check_filter_params(f"{what}: {name}", group, rate, **p)
    return dict(group=group, rate=rate, **p)


class LiveSession:
    """What ``IRFD.live`` returns (its docstring has the arguments).  ``step`` takes the next frames of the feed; ``frames`` counts
    the frames seen so far; ``reset()`` forgets them.  The filter states are device tensors of the session (``lm_state``,
    ``feature_state``, ``colour_state``)."""

    def __init__(self, model, identity_u8, *, size, template, contour, channel_order, identity_align, rate, track, features, feather,
                 matte_softness, matte_grow, colour_match, colour_decay, seed, noise, offset):
        from .irfd import _check_noise
        what = "live"
        self.size = FR._out_size(size, what)
        FR._channel_swap(channel_order)
        self.channel_order = channel_order
        if template is None:
            raise ValueError(f"{what}: a template is needed: the tracked landmarks as (u, v) in the network image"
                             + (" (contour= takes its fallback outline from it)" if contour is not None else ""))
        try:
            K = template.size(0) if isinstance(template, torch.Tensor) else len(template)
        except TypeError:
            raise ValueError(f"{what}: template must be [K,2] points (u, v), got {type(template).__name__}") from None
        if not 2 <= K <= FR.LANDMARKS_MAX:
            raise ValueError(f"{what}: template must be [K,2] points (u, v) with 2 <= K <= {FR.LANDMARKS_MAX}, got K = {K}")
        template, _, self.offset = FR._check_fit(torch.empty(1, K, 2), template, None, offset, what)
        self.K = K
        self.contour = None if contour is None else FR._check_contour(contour, K, what)
        self.rate = FR._finite(rate, "rate", what, positive=True)
        self.track = _filter_params(what, "track", track, 2, self.rate)
        self.features = _filter_params(what, "features", features, 1, self.rate)
        self.feather = FR.check_feather(feather, what)
        self.softness, self.grow = FR._finite(matte_softness, "matte_softness", what, positive=True), FR._finite(matte_grow, "matte_grow", what)
        if not isinstance(colour_match, bool):
            raise ValueError(f"{what}: colour_match must be a bool, got {colour_match!r}")
        self.colour_match = colour_match
        self.colour_decay = FR._finite(colour_decay, "colour_decay", what)
        if not 0.0 <= self.colour_decay <= 1.0:
            raise ValueError(f"{what}: colour_decay must be in [0, 1], got {self.colour_decay}")
        _check_noise(what, noise, seed, None, 0)
        self.seed, self.fixed_noise = seed, noise == "fixed"
        if not isinstance(identity_u8, torch.Tensor) or identity_u8.dim() not in (3, 4) or identity_u8.size(-1) != 3 or \
                (identity_u8.dim() == 4 and identity_u8.size(0) != 1):
            got = tuple(identity_u8.shape) if isinstance(identity_u8, torch.Tensor) else type(identity_u8).__name__
            raise ValueError(f"{what}: identity_u8 must be [H,W,3] or [1,H,W,3], got {got}")
        if identity_align is not None:                                     # host rows: checked here, before any launch
            identity_align = FR.Aligned.parse(identity_align, 1, size, identity_u8.device, f"{what}: identity_align")
        # ---- the arguments are in order: the device
        if identity_align is None:
            ident = FR.frames_from_u8(identity_u8, size, channel_order=channel_order)
        else:
            ident = FR.frames_from_u8_aligned(identity_u8, size, identity_align.rows, channel_order=channel_order)
        self.model, self.device = model, ident.device
        self.fi = model.encode(ident, "Ei")                                # once per session
        if template.is_cuda and template.device != self.device:
            raise L.SpkError(f"{what}: template on {template.device}, the identity image on {self.device}")
        self._template_host = None if template.is_cuda else template
        self.template = template.to(self.device).contiguous()
        self.lm_state = None if self.track is None else FR.causal_filter_state(2 * K, 2, self.device)
        self.feature_state = None if self.features is None else FR.causal_filter_state(2 * self.fi.numel(), 1, self.device)
        self.colour_state = torch.zeros(FR.COLOUR_SUMS, device=self.device, dtype=torch.float64) if colour_match else None
        self._nan = torch.full((), float("nan"), device=self.device)
        self._generated = {}                                               # per generated width: (the rows' scale, the fallback outline)
        self.frames = 0

    def reset(self):
        """Empties the filter states and the frame counter: the next ``step`` is the first of a feed.  ``fi`` stays."""
        for s in (self.lm_state, self.feature_state, self.colour_state):
            if s is not None:
                s.zero_()
        self.frames = 0

    def _for_generated(self, Hs, Ws):
        """The network image has ``size`` pixels where the generated one has ``Hs x Ws``: -> (the factor of a row's ``(a, c)`` as a
        device tensor, or None when it is 1; the template's contour in generated pixels), made once per session; the factor is
        ``Aligned.chunk``'s"""
        if Hs * self.size[1] != Ws * self.size[0]:
            raise ValueError(f"live: generated frames must have the shape of the network input, got {Hs} x {Ws} for {self.size}")
        if Ws not in self._generated:
            scale, fallback = FR.generated_row_scale(self.size, Ws, self.device), None
            if self.contour is not None:
                FR._matte_size((Hs, Ws), "live")
                points = self.template if self._template_host is None else self._template_host
                fallback = (points[self.contour] * torch.tensor(Ws / self.size[1], dtype=torch.float32).to(points.device)).to(self.device)
            self._generated[Ws] = (scale, fallback)
        return self._generated[Ws]

    @torch.no_grad()
    def step(self, frames_u8, landmarks, *, weights=None, emotion_u8=None, inplace=False):
        """The next ``N`` frames of the feed: ``frames_u8`` uint8 ``[N,H,W,3]`` on the device, ``landmarks`` device float32
        ``[N,K,2]`` as the tracker left them (``weights``: its confidences, in the forms of ``ops.causal_filter``), ``emotion_u8``: the
        frames ``Ee`` sees (None: ``frames_u8``; cropped with the same rows).  -> uint8 ``[N,H,W,3]``: the frames with the generated
        face pasted in (``inplace=True``: ``frames_u8`` itself, which then needs packed pixels); a frame whose landmarks give no
        transform -- lost for longer than ``hold`` frames, or never seen -- passes through untouched."""
        what = "live.step"
        if not isinstance(frames_u8, torch.Tensor) or frames_u8.dim() != 4 or frames_u8.size(3) != 3 or frames_u8.size(0) < 1:
            got = tuple(frames_u8.shape) if isinstance(frames_u8, torch.Tensor) else type(frames_u8).__name__
            raise ValueError(f"{what}: frames must be [N,H,W,3], got {got}")
        N = frames_u8.size(0)
        if not isinstance(landmarks, torch.Tensor) or tuple(landmarks.shape) != (N, self.K, 2):
            got = tuple(landmarks.shape) if isinstance(landmarks, torch.Tensor) else type(landmarks).__name__
            raise ValueError(f"{what}: landmarks must be [{N},{self.K},2], {self.K} points per frame as the template has, got {got}")
        if emotion_u8 is not None and (not isinstance(emotion_u8, torch.Tensor) or tuple(emotion_u8.shape) != tuple(frames_u8.shape)):
            raise ValueError(f"{what}: emotion_u8 must match the frames {tuple(frames_u8.shape)}")
        if not isinstance(inplace, bool):
            raise ValueError(f"{what}: inplace must be a bool, got {inplace!r}")
        if self.track is None:
            _, weights, _ = FR._check_fit(landmarks, self.template, weights, self.offset, what)
        if inplace and not FR.packed_pixels(frames_u8):
            raise L.SpkError(f"{what}: inplace needs packed pixels and rows / frames that do not overlap, got strides {frames_u8.stride()}")
        model, order = self.model, dict(channel_order=self.channel_order)
        # 1, 2: the landmarks steadied, and the rows fitted to them; a held point keeps its last weight, an expired one has none
        if self.track is not None:
            landmarks, weights = FR.causal_filter(landmarks, self.lm_state, weights=weights, **self.track)
        rows = FR._fit(landmarks, self.template, weights, self.offset, what)
        # 3, 4: the crops, Ee and Ep
        pose = FR.frames_from_u8_aligned(frames_u8, self.size, rows, **order)
        emo = pose if emotion_u8 is None else FR.frames_from_u8_aligned(emotion_u8, self.size, rows, **order)
        fe, fp = model.encode(emo, "Ee"), model.encode(pose, "Ep")
        fi = self.fi.expand(N, -1, -1, -1)
        if self.features is None:
            gin = model._prepare_generator_input(fi, fe, fp)
        else:
            # 5: emotion and pose steadied; the features of a frame without a transform (a crop of nothing) take no part
            f = torch.cat([fe.view(N, -1), fp.view(N, -1)], 1)
            f = torch.where(torch.isfinite(rows).all(1, keepdim=True), f, self._nan)
            f, _ = FR.causal_filter(f, self.feature_state, out=f, **self.features)
            gin = torch.cat([fi.reshape(N, -1), f], 1)
        # 6: the decoder; frame t of the feed has noise index t
        seeded = None if self.seed is None else dict(seed=self.seed, frame0=0 if self.fixed_noise else self.frames, fixed_noise=self.fixed_noise)
        y = model._decode_eval(gin, None, "f32", "rgb", seeded)
        # 7 - 9: matte, colour rows and the paste, with the rows scaled to the generated size
        Hs, Ws = y.shape[2:]
        scale, fallback = self._for_generated(Hs, Ws)
        if scale is not None:
            rows = rows * scale
        matte = None
        if self.contour is not None:
            matte = FR._matte(landmarks, rows, Hs, Ws, self.contour, self.softness, self.grow, self.offset, fallback, *FR._check_smooth(0, None, what),
                              what)
        out = frames_u8 if inplace else frames_u8.clone(memory_format=torch.contiguous_format)
        colour = None
        if self.colour_match:                                              # the statistics read the background before the paste writes it
            sums = FR.paste_colour_sums(y, out, rows, matte=matte, feather=self.feather, **order)
            colour = FR.colour_rows_causal(sums, self.colour_state, self.colour_decay)
        FR.frames_paste_u8_aligned(y, out, rows, feather=self.feather, out=out, matte=matte, colour=colour, **order)
        self.frames += N
        return out
