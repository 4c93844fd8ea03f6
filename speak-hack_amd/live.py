"""``IRFD.live``: a reenactment SESSION for a feed whose next frame does not exist yet -- a camera, a call, or a long video pushed
through a few frames at a time.  ``IRFD.reenact_video`` takes a clip that is in memory: it runs ``Ei`` on every call and smooths the
landmarks, the matte's contour and the colour statistics with windows over frames ``t - r ... t + r``.  A session runs ``Ei`` once,
keeps ``fi``, and steadies the same three things with the causal filters of csrc/causal_filter.hip, whose state lives in device
tensors on the session: ``step`` reads no device value on the host, and ``N`` frames in one ``step`` and the same frames in any split
of steps give the same bytes.  The feed is packed RGB, (``pixel_format="nv12"``) NV12 surfaces as a hardware decoder leaves them or
(``pixel_format="i420"``) the three planes of a software decoder or a WebRTC frame buffer, or (``pixel_format="rgb32"``) four bytes per pixel
as a capture surface or an interop texture holds them: the pixel format decides which launchers read and write the frames
(``_Rgb24Edge`` / ``_Nv12Edge`` / ``_I420Edge`` / ``_Rgb32Edge``), and nothing else.

``IRFD.live_room``: S such feeds at once -- a server with several calls -- as ONE batch per tick (``LiveRoom``): the frames of a tick
are the batch rows of the same launches a session makes, with the state of every feed, its frame counter and its seed on the device."""
from __future__ import annotations

import torch

from . import _lib as L
from . import frames as FR
from . import ops


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


def _check_identity(what, name, identity_u8):
    """One identity photo: [H,W,3] or [1,H,W,3]"""
    if not isinstance(identity_u8, torch.Tensor) or identity_u8.dim() not in (3, 4) or identity_u8.size(-1) != 3 or \
            (identity_u8.dim() == 4 and identity_u8.size(0) != 1):
        got = tuple(identity_u8.shape) if isinstance(identity_u8, torch.Tensor) else type(identity_u8).__name__
        raise ValueError(f"{what}: {name} must be [H,W,3] or [1,H,W,3], got {got}")


class _Rgb24Edge:
    """What a step asks of packed uint8 frames in ``channel_order``: a tensor ``[N,H,W,3]``, or a ``FrameTable``"""
    surfaces, table, noun, shape, channels = False, FR.FrameTable, "frames [H,W,3]", "[{},H,W,3]", 3
    way_in, sums, paste, clone = (staticmethod(f) for f in (FR.frames_from_u8_aligned, FR.paste_colour_sums, FR.frames_paste_u8_aligned,
                                                            FR.clone_frames))

    def __init__(self, channel_order, standard, full_range):
        self.args = dict(channel_order=channel_order)

    def count(self, frames):
        return len(frames)

    def writable(self, what, frames):
        if not FR.packed_pixels(frames):
            raise L.SpkError(f"{what}: inplace needs packed pixels and rows / frames that do not overlap, got strides {frames.stride()}")

    def present(self, table):
        return table.frames

    def ready(self, what, name, frames, device):                          # a packed tensor takes exactly the path it always took
        pass


class _Rgb32Edge(_Rgb24Edge):
    """The same of RGB32 frames in one of the four orders of ``frames.RGB32_ORDERS``: a tensor ``[N,H,W,4]``, or an ``Rgb32Table``.
    The fourth byte of a pixel is neither read into the network nor changed by the paste."""
    table, noun, shape, channels = FR.Rgb32Table, "frames [H,W,4]", "[{},H,W,4]", 4
    way_in, sums, paste, clone = (staticmethod(f) for f in (FR.frames_from_rgb32_aligned, FR.paste_colour_sums_rgb32,
                                                            FR.frames_paste_rgb32_aligned, FR.clone_rgb32))

    def writable(self, what, frames):
        if not FR.rgb32_pixels(frames):
            raise L.SpkError(f"{what}: inplace needs pixels that are aligned 32-bit words (a data pointer and strides that are multiples of 4) "
                             f"and rows / frames that do not overlap, got strides {frames.stride()} at {frames.data_ptr():#x}")

    def ready(self, what, name, frames, device):
        """What the launchers would refuse of a tensor of frames, asked before the first launch of a step"""
        if not frames.is_cuda or frames.dtype != torch.uint8 or frames.device != device:
            raise L.SpkError(f"{what}: {name}: expected a uint8 HIP tensor on {device}, got {frames.dtype} on {frames.device} (no CPU path)")


class _Nv12Edge:
    """The same of NV12 surfaces in the colour of ``standard`` / ``full_range``: a pair of planes ``(y [N,H,W], uv [N,H/2,W/2,2])`` as
    ``ops.nv12_planes`` opened them, or a ``SurfaceTable``.  The way in makes R, G, B planes, as ``Nv12.network_input`` does."""
    surfaces, table, noun, shape = True, FR.SurfaceTable, "NV12 surfaces", "[{},3H/2,W]"
    way_in, sums, paste, clone = (staticmethod(f) for f in (FR.frames_from_nv12_aligned, FR.paste_colour_sums_nv12,
                                                            FR.frames_paste_nv12_aligned, FR.clone_surfaces))
    planes_of, strides_of, form = staticmethod(FR.nv12_planes), staticmethod(FR.nv12_strides), "a pair of planes"

    def __init__(self, channel_order, standard, full_range):
        self.args = dict(standard=standard, full_range=full_range)

    def plane_tuple(self, frames, S):
        """The planes of ``S`` surfaces as one tuple, and not a sequence of surfaces"""
        return FR.plane_pair(frames)

    def count(self, frames):
        return len(frames) if isinstance(frames, self.table) else frames[0].size(0)

    def writable(self, what, frames):
        if isinstance(frames, self.table):
            frames.check_written()
        else:
            self.strides_of(*frames, f"{what}: inplace", written=True)

    def present(self, table):
        return table.planes

    def open(self, what, name, surfaces, N=None):
        """``[N,3H/2,W]`` or a tuple of planes -> the planes, their shape and dtype checked on the host (``N``: the count they must have)"""
        try:
            planes = self.planes_of(surfaces)
        except ValueError as e:
            raise ValueError(f"{what}: {name}: {e}") from None
        if N is not None and planes[0].size(0) != N:
            raise ValueError(f"{what}: {name} must be [{N},3H/2,W] or {self.form}, one surface per feed, got {planes[0].size(0)} surfaces")
        return planes

    def ready(self, what, name, planes, device):
        """What the launchers would refuse of a tuple of planes, asked before the first launch of a step"""
        self.strides_of(*planes, f"{what}: {name}", written=False)
        if any(p.device != device for p in planes):
            raise L.SpkError(f"{what}: {name} on {planes[0].device}, the identity image on {device}")


class _I420Edge(_Nv12Edge):
    """The same of I420 surfaces: a triple of planes ``(y [N,H,W], u [N,H/2,W/2], v [N,H/2,W/2])`` as ``ops.i420_planes`` opened
    them, or a ``PlanarTable``"""
    table, noun = FR.PlanarTable, "I420 surfaces"
    way_in, sums, paste, clone = (staticmethod(f) for f in (FR.frames_from_i420_aligned, FR.paste_colour_sums_i420,
                                                            FR.frames_paste_i420_aligned, FR.clone_planar))
    planes_of, strides_of, form = staticmethod(FR.i420_planes), staticmethod(FR.i420_strides), "a triple of planes"

    def plane_tuple(self, frames, S):                                     # three 2-D planes are ONE frame: a room of one feed only
        return FR.plane_triple(frames, one=S == 1)


_EDGES = {"rgb24": _Rgb24Edge, "nv12": _Nv12Edge, "i420": _I420Edge, "rgb32": _Rgb32Edge}


class _Live:
    """What a session and a room share: the arguments of ``IRFD.live`` checked on the host, ``Ei`` on one photo, and the body of a
    step over a batch of frames.  The two differ in what a batch row is -- the next frame of one feed, or this tick's frame of the
    next feed -- and so in how the three filters, ``fi`` and the noise index are laid over the rows: ``_steady``,
    ``_steady_features``, ``_fi``, ``_seeded`` and ``_colour_rows``."""

    def _configure(self, what, model, *, size, template, contour, channel_order, rate, track, features, feather, matte_softness, matte_grow,
                   colour_match, colour_decay, offset, pixel_format, standard, full_range):
        self.size = FR._out_size(size, what)
        if pixel_format == "rgb32":                                        # the identity photo: the colour order with the alpha dropped
            self.channel_order = FR.rgb32_order(channel_order)[0]
        else:
            FR._channel_swap(channel_order)
            self.channel_order = channel_order
        if pixel_format not in _EDGES:
            raise ValueError(f"{what}: pixel_format must be 'rgb24' or 'nv12' or 'i420' or 'rgb32', got {pixel_format!r}")
        if pixel_format in ("rgb24", "rgb32") and (standard != "bt601" or full_range):
            raise ValueError(f"{what}: standard / full_range apply to pixel_format='nv12' only, and to 'i420'")
        FR.yuv_standard(standard, full_range)
        self.pixel_format, self.edge = pixel_format, _EDGES[pixel_format](channel_order, standard, full_range)
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
        self.model = model
        return template

    def _place_template(self, what, template):
        if template.is_cuda and template.device != self.device:
            raise L.SpkError(f"{what}: template on {template.device}, the identity image on {self.device}")
        self._template_host = None if template.is_cuda else template
        self.template = template.to(self.device).contiguous()
        self._nan = torch.full((), float("nan"), device=self.device)
        self._generated = {}                                               # per generated width: (the rows' scale, the fallback outline)

    def _encode_identity(self, identity_u8, identity_align):
        """``Ei`` on one photo at batch 1 (``identity_align``: None, or parsed ``Aligned`` rows): -> fi [1,2048,1,1]"""
        if identity_align is None:
            ident = FR.frames_from_u8(identity_u8, self.size, channel_order=self.channel_order)
        else:
            ident = FR.frames_from_u8_aligned(identity_u8, self.size, identity_align.rows, channel_order=self.channel_order)
        return self.model.encode(ident, "Ei")

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

    def _check_step(self, what, frames_u8, emotion_u8, inplace):
        """-> ``emotion_u8`` as the body takes it: beside a table of frames, a table of the same sizes per feed; beside a pair of NV12
        planes, a pair of the same size.  With NV12 planes, what the launchers would refuse of them is asked here, before a launch."""
        edge = self.edge
        if isinstance(frames_u8, edge.table):
            if emotion_u8 is not None:
                emotion_u8 = self._table(what, "emotion_u8", emotion_u8)
                if emotion_u8.sizes != frames_u8.sizes:
                    raise ValueError(f"{what}: emotion_u8 must match the frames feed by feed: sizes {emotion_u8.sizes}, the frames' {frames_u8.sizes}")
        elif edge.surfaces:
            if emotion_u8 is not None:
                emotion_u8 = edge.open(what, "emotion_u8", emotion_u8)
                if emotion_u8[0].shape != frames_u8[0].shape:
                    raise ValueError(f"{what}: emotion_u8 must match the surfaces: {tuple(emotion_u8[0].shape)}, the frames' {tuple(frames_u8[0].shape)}")
        elif emotion_u8 is not None and (not isinstance(emotion_u8, torch.Tensor) or tuple(emotion_u8.shape) != tuple(frames_u8.shape)):
            raise ValueError(f"{what}: emotion_u8 must match the frames {tuple(frames_u8.shape)}")
        if not isinstance(inplace, bool):
            raise ValueError(f"{what}: inplace must be a bool, got {inplace!r}")
        if not isinstance(frames_u8, edge.table):
            edge.ready(what, "frames", frames_u8, self.device)
            if emotion_u8 is not None:
                edge.ready(what, "emotion_u8", emotion_u8, self.device)
        return emotion_u8

    def _body(self, what, frames_u8, landmarks, weights, emotion_u8, inplace):
        """The steps of one ``step`` over the ``N`` rows of ``frames_u8`` -- a tensor ``[N,H,W,3]`` or a ``FrameTable`` of ``N`` frames;
        with NV12, a pair of planes or a ``SurfaceTable`` (``emotion_u8``: the same form) -- after the host checks: ``landmarks`` [N,K,2]
        and ``weights`` as the filter (``track``) or else the fit takes them.  The ONE routine of both pixel formats: ``edge`` says
        which launchers read and write the frames and how they are cloned."""
        edge = self.edge
        if inplace:
            edge.writable(what, frames_u8)
        N = edge.count(frames_u8)
        model, order = self.model, edge.args
        # 1, 2: the landmarks steadied, and the rows fitted to them; a held point keeps its last weight, an expired one has none
        if self.track is not None:
            landmarks, weights = self._steady(landmarks, weights)
        rows = FR._fit(landmarks, self.template, weights, self.offset, what)
        # 3, 4: the crops, Ee and Ep
        pose = edge.way_in(frames_u8, self.size, rows, **order)
        emo = pose if emotion_u8 is None else edge.way_in(emotion_u8, self.size, rows, **order)
        fe, fp = model.encode(emo, "Ee"), model.encode(pose, "Ep")
        fi = self._fi(N)
        if self.features is None:
            gin = model._prepare_generator_input(fi, fe, fp)
        else:
            # 5: emotion and pose steadied; the features of a frame without a transform (a crop of nothing) take no part
            f = torch.cat([fe.view(N, -1), fp.view(N, -1)], 1)
            f = torch.where(torch.isfinite(rows).all(1, keepdim=True), f, self._nan)
            self._steady_features(f)
            gin = torch.cat([fi.reshape(N, -1), f], 1)
        # 6: the decoder; frame t of a feed has noise index t
        y = model._decode_eval(gin, None, "f32", "rgb", self._seeded())
        # 7 - 9: matte, colour rows and the paste, with the rows scaled to the generated size
        Hs, Ws = y.shape[2:]
        scale, fallback = self._for_generated(Hs, Ws)
        if scale is not None:
            rows = rows * scale
        matte = None
        if self.contour is not None:
            matte = FR._matte(landmarks, rows, Hs, Ws, self.contour, self.softness, self.grow, self.offset, fallback, *FR._check_smooth(0, None, what),
                              what)
        out = frames_u8 if inplace else edge.clone(frames_u8)
        colour = None
        if self.colour_match:                                              # the statistics read the background before the paste writes it
            sums = edge.sums(y, out, rows, matte=matte, feather=self.feather, **order)
            colour = self._colour_rows(sums)
        edge.paste(y, out, rows, feather=self.feather, out=out, matte=matte, colour=colour, **order)
        return out


class LiveSession(_Live):
    """What ``IRFD.live`` returns (its docstring has the arguments).  ``step`` takes the next frames of the feed; ``frames`` counts
    the frames seen so far; ``reset()`` forgets them.  The filter states are device tensors of the session (``lm_state``,
    ``feature_state``, ``colour_state``)."""

    def __init__(self, model, identity_u8, *, size, template, contour, channel_order, identity_align, rate, track, features, feather,
                 matte_softness, matte_grow, colour_match, colour_decay, seed, noise, offset, pixel_format="rgb24", standard="bt601",
                 full_range=False):
        from .irfd import _check_noise
        what = "live"
        template = self._configure(what, model, size=size, template=template, contour=contour, channel_order=channel_order, rate=rate, track=track,
                                   features=features, feather=feather, matte_softness=matte_softness, matte_grow=matte_grow,
                                   colour_match=colour_match, colour_decay=colour_decay, offset=offset, pixel_format=pixel_format,
                                   standard=standard, full_range=full_range)
        _check_noise(what, noise, seed, None, 0)
        self.seed, self.fixed_noise = seed, noise == "fixed"
        _check_identity(what, "identity_u8", identity_u8)
        if identity_align is not None:                                     # host rows: checked here, before any launch
            identity_align = FR.Aligned.parse(identity_align, 1, size, identity_u8.device, f"{what}: identity_align")
        # ---- the arguments are in order: the device
        self.fi = self._encode_identity(identity_u8, identity_align)       # once per session
        self.device = self.fi.device
        self._place_template(what, template)
        K = self.K
        self.lm_state = None if self.track is None else FR.causal_filter_state(2 * K, 2, self.device)
        self.feature_state = None if self.features is None else FR.causal_filter_state(2 * self.fi.numel(), 1, self.device)
        self.colour_state = torch.zeros(FR.COLOUR_SUMS, device=self.device, dtype=torch.float64) if colour_match else None
        self.frames = 0

    def reset(self):
        """Empties the filter states and the frame counter: the next ``step`` is the first of a feed.  ``fi`` stays."""
        for s in (self.lm_state, self.feature_state, self.colour_state):
            if s is not None:
                s.zero_()
        self.frames = 0

    # ---- a batch row is the next frame of the feed: the filters walk the rows in order
    def _steady(self, landmarks, weights):
        return FR.causal_filter(landmarks, self.lm_state, weights=weights, **self.track)

    def _steady_features(self, f):
        FR.causal_filter(f, self.feature_state, out=f, **self.features)

    def _fi(self, N):
        return self.fi.expand(N, -1, -1, -1)

    def _seeded(self):
        return None if self.seed is None else dict(seed=self.seed, frame0=0 if self.fixed_noise else self.frames, fixed_noise=self.fixed_noise)

    def _colour_rows(self, sums):
        return FR.colour_rows_causal(sums, self.colour_state, self.colour_decay)

    @torch.no_grad()
    def step(self, frames_u8, landmarks, *, weights=None, emotion_u8=None, inplace=False):
        """The next ``N`` frames of the feed: ``frames_u8`` uint8 ``[N,H,W,3]`` on the device, ``landmarks`` device float32
        ``[N,K,2]`` as the tracker left them (``weights``: its confidences, in the forms of ``ops.causal_filter``), ``emotion_u8``: the
        frames ``Ee`` sees (None: ``frames_u8``; cropped with the same rows).  -> uint8 ``[N,H,W,3]``: the frames with the generated
        face pasted in (``inplace=True``: ``frames_u8`` itself, which then needs packed pixels); a frame whose landmarks give no
        transform -- lost for longer than ``hold`` frames, or never seen -- passes through untouched.

        ``pixel_format="nv12"``: ``frames_u8`` is the next ``N`` surfaces, one uint8 tensor ``[N,3H/2,W]`` or a pair of planes
        (``ops.nv12_planes``), and ``emotion_u8`` takes the same form and size.  -> a packed clone ``[N,3H/2,W]`` with the face pasted
        in; ``inplace=True``: the input itself, whose frames must not overlap.  What the launchers would refuse of the surfaces (a
        device, a pixel stride, frames that overlap) is refused before the first launch: the states stay as they were.

        ``pixel_format="i420"``: the same with ``ops.i420_planes`` in place of ``ops.nv12_planes`` -- one contiguous packed tensor
        ``[N,3H/2,W]`` or a triple of planes ``(y, u, v)`` of any pitches -- and the Y, U and V bytes of the NV12 session on the
        interleaved surfaces.

        ``pixel_format="rgb32"``: ``frames_u8`` (and ``emotion_u8``) is uint8 ``[N,H,W,4]`` in the session's ``channel_order``
        (``"rgba"``, ``"bgra"``, ``"argb"``, ``"abgr"``), read in place where its pixels are aligned 32-bit words
        (``ops.frames_from_rgb32_aligned``), else through a copy.  -> a contiguous clone ``[N,H,W,4]`` with the face pasted in;
        ``inplace=True``: the input itself, which then needs aligned pixels and frames that do not overlap.  The colour bytes are
        those of the rgb24 session on the stripped feed; the fourth byte of every pixel is what it was."""
        what = "live.step"
        given = frames_u8
        if self.edge.surfaces:
            frames_u8 = self.edge.open(what, "frames", frames_u8)
            N = frames_u8[0].size(0)
        elif not isinstance(frames_u8, torch.Tensor) or frames_u8.dim() != 4 or frames_u8.size(3) != self.edge.channels or frames_u8.size(0) < 1:
            got = tuple(frames_u8.shape) if isinstance(frames_u8, torch.Tensor) else type(frames_u8).__name__
            raise ValueError(f"{what}: frames must be [N,H,W,{self.edge.channels}], got {got}")
        else:
            N = frames_u8.size(0)
        if not isinstance(landmarks, torch.Tensor) or tuple(landmarks.shape) != (N, self.K, 2):
            got = tuple(landmarks.shape) if isinstance(landmarks, torch.Tensor) else type(landmarks).__name__
            raise ValueError(f"{what}: landmarks must be [{N},{self.K},2], {self.K} points per frame as the template has, got {got}")
        emotion_u8 = self._check_step(what, frames_u8, emotion_u8, inplace)
        if self.track is None:
            _, weights, _ = FR._check_fit(landmarks, self.template, weights, self.offset, what)
        out = self._body(what, frames_u8, landmarks, weights, emotion_u8, inplace)
        self.frames += N
        return given if inplace else out


class LiveRoom(_Live):
    """What ``IRFD.live_room`` returns (its docstring has the arguments): ``S`` feeds stepped together, one frame per feed per tick,
    in the launches of ONE session step at batch ``S``.  Slot ``s`` is a ``LiveSession`` of its own: its landmark state, its ``fi`` and
    its noise are to the bit those of a session that saw the frames of slot ``s`` one at a time, and its frames are that session's as
    the chunks of ``reenact_video`` are each other's -- the encoders and the decoder run at batch ``S`` where the session runs them at
    batch 1, which is the same image once quantised except where a value sits on a rounding boundary (DESIGN 4.2k has the counts).
    Everything a feed remembers is on the device:

      ``fi``             float32 ``[S,2048,1,1]``, row ``s`` bit for bit the ``fi`` of a session on photo ``s`` (``Ei`` at batch 1);
      ``lm_state``       float64 ``[S K, 6]``: the landmark filter's groups, slot ``s`` in rows ``s K ... (s + 1) K - 1``;
      ``feature_state``  float64 ``[S 4096, 4]``, slot after slot;
      ``colour_state``   float64 ``[S,13]``;
      ``frames``         int64 ``[S]``: the ticks each slot has seen since its reset (all 0 with ``noise="fixed"``), the frame index of
                         its noise; advanced on the device;
      ``seeds``          int64 ``[S]``: the 64-bit patterns of the seeds (``ops.seed_rows``), or None without a seed.

    A slot with nothing to show in a tick is given NaN landmarks: it is a session's lost frame, held up to ``hold`` ticks and then
    passed through untouched, and its counter advances as a session's does.  The feeds' frames may be one tensor or S buffers of S
    sizes, packed RGB or NV12 surfaces (``step``).  Out of scope: stepping a subset of the slots, several frames per feed per tick."""

    def __init__(self, model, identities_u8, *, size, template, contour, channel_order, identity_align, rate, track, features, feather,
                 matte_softness, matte_grow, colour_match, colour_decay, seed, noise, offset, pixel_format="rgb24", standard="bt601",
                 full_range=False):
        from .irfd import _check_noise
        what = "live_room"
        template = self._configure(what, model, size=size, template=template, contour=contour, channel_order=channel_order, rate=rate, track=track,
                                   features=features, feather=feather, matte_softness=matte_softness, matte_grow=matte_grow,
                                   colour_match=colour_match, colour_decay=colour_decay, offset=offset, pixel_format=pixel_format,
                                   standard=standard, full_range=full_range)
        if isinstance(identities_u8, torch.Tensor):
            if identities_u8.dim() != 4:
                raise ValueError(f"{what}: identities_u8 must be a sequence of S photos [H,W,3] or a tensor [S,H,W,3], got {tuple(identities_u8.shape)}")
            photos = list(identities_u8.unbind(0))
        else:
            try:
                photos = list(identities_u8)
            except TypeError:
                raise ValueError(f"{what}: identities_u8 must be a sequence of S photos [H,W,3] or a tensor [S,H,W,3], got "
                                 f"{type(identities_u8).__name__}") from None
        S = self.S = len(photos)
        if S < 1:
            raise ValueError(f"{what}: a room needs at least one feed, got S = {S} identity photos")
        for s, photo in enumerate(photos):
            _check_identity(what, f"identities_u8[{s}]", photo)
            if photo.device != photos[0].device:
                raise ValueError(f"{what}: identities_u8[{s}] on {photo.device}, identities_u8[0] on {photos[0].device}")
        if seed is None or isinstance(seed, int):
            _check_noise(what, noise, seed, None, 0)
            seeds = None if seed is None else [seed] * S
        else:
            try:
                seeds = list(seed)
            except TypeError:
                raise ValueError(f"{what}: seed must be None, one integer or {S} of them, got {type(seed).__name__}") from None
            if len(seeds) != S:
                raise ValueError(f"{what}: seed must be one integer or one per feed ({S}), got {len(seeds)}")
            for v in seeds:
                _check_noise(what, noise, v, None, 0)
                if v is None:
                    raise ValueError(f"{what}: a sequence of seeds holds {S} integers, got None among them")
        self.fixed_noise = noise == "fixed"
        aligns = self._parse_aligns(what, identity_align, photos)
        # ---- the arguments are in order: the device
        self.fi = torch.cat([self._encode_identity(p, a) for p, a in zip(photos, aligns)])       # Ei at batch 1, as a session runs it
        self.device = self.fi.device
        self._place_template(what, template)
        K, F = self.K, 2 * self.fi[0].numel()
        self.lm_state = None if self.track is None else FR.causal_filter_state(S * 2 * K, 2, self.device)
        self.feature_state = None if self.features is None else FR.causal_filter_state(S * F, 1, self.device)
        self.colour_state = torch.zeros((S, FR.COLOUR_SUMS), device=self.device, dtype=torch.float64) if colour_match else None
        self.frames = torch.zeros(S, device=self.device, dtype=torch.int64)
        self.seeds = None if seeds is None else ops.seed_rows(seeds, self.device)

    def _parse_aligns(self, what, identity_align, photos):
        if identity_align is None:
            return [None] * len(photos)
        try:
            aligns = list(identity_align)
        except TypeError:
            raise ValueError(f"{what}: identity_align must be None or one per photo ({len(photos)}), got {type(identity_align).__name__}") from None
        if len(aligns) != len(photos):
            raise ValueError(f"{what}: identity_align must be None or one per photo ({len(photos)}), got {len(aligns)}")
        return [None if a is None else FR.Aligned.parse(a, 1, self.size, p.device, f"{what}: identity_align[{s}]")
                for s, (a, p) in enumerate(zip(aligns, photos))]

    def _slot(self, what, slot):
        if isinstance(slot, bool) or not isinstance(slot, int) or not 0 <= slot < self.S:
            raise ValueError(f"{what}: slot must be an integer in [0, {self.S}), got {slot!r}")
        return slot

    def _states(self):
        """The per-feed state tensors, each viewed with the slots in front"""
        return [t.view(self.S, -1) for t in (self.lm_state, self.feature_state, self.colour_state, self.frames) if t is not None]

    def reset(self, slot=None):
        """Empties the filter states and the frame counter of ``slot`` (None: of every slot): its next tick is the first of a feed.
        ``fi`` stays; no other slot is touched, and no device value is read."""
        if slot is not None:
            slot = self._slot("live_room.reset", slot)
        for t in self._states():
            (t if slot is None else t[slot]).zero_()

    @torch.no_grad()
    def set_identity(self, slot, identity_u8, identity_align=None):
        """A new call in ``slot``: ``Ei`` on ``identity_u8`` ([H,W,3] or [1,H,W,3]; ``identity_align``: as ``IRFD.live``) into ``fi[slot]``,
        and the slot reset.  No other slot's state or output changes."""
        what = "live_room.set_identity"
        slot = self._slot(what, slot)
        _check_identity(what, "identity_u8", identity_u8)
        if identity_align is not None:
            identity_align = FR.Aligned.parse(identity_align, 1, self.size, identity_u8.device, f"{what}: identity_align")
        fi = self._encode_identity(identity_u8, identity_align)
        if fi.device != self.device:
            raise L.SpkError(f"{what}: the photo on {fi.device}, the room on {self.device}")
        self.fi[slot].copy_(fi[0])
        self.reset(slot)

    # ---- a batch row is this tick's frame of the next feed: one frame of S times the components, every feed with its own groups
    def _steady(self, landmarks, weights):
        S, K = self.S, self.K
        y, wy = FR.causal_filter(landmarks.reshape(1, S * K * 2), self.lm_state, weights=weights, **self.track)
        return y.view(S, K, 2), wy.view(S, K)

    def _steady_features(self, f):
        flat = f.view(1, -1)
        FR.causal_filter(flat, self.feature_state, out=flat, **self.features)

    def _fi(self, N):
        return self.fi

    def _seeded(self):
        return None if self.seeds is None else dict(seed_rows=self.seeds, frame_rows=self.frames)

    def _colour_rows(self, sums):
        return FR.colour_rows_causal_feeds(sums.view(1, self.S, FR.COLOUR_SUMS), self.colour_state, self.colour_decay).view(self.S, 3, 2)

    def _weights(self, what, weights):
        """``weights``: None, or per feed ``[S,K]``, or one ``[K]`` set for every feed; host numbers or a device float32 tensor ->
        None or a float32 tensor ``[S K]``, where it came from (not read)"""
        if weights is None:
            return None
        S, K = self.S, self.K
        if isinstance(weights, torch.Tensor) and weights.is_cuda:
            if weights.dtype != torch.float32 or tuple(weights.shape) not in ((K,), (S, K)):
                raise ValueError(f"{what}: device weights must be a float32 tensor [{K}] or [{S},{K}], got {weights.dtype} {tuple(weights.shape)}")
        else:
            try:
                weights = torch.as_tensor(weights).to(torch.float64).to(torch.float32)
            except (ValueError, TypeError, RuntimeError) as e:
                raise ValueError(f"{what}: weights must be [{K}] or [{S},{K}] numbers: {e}") from None
            if tuple(weights.shape) not in ((K,), (S, K)):
                raise ValueError(f"{what}: weights must be [{K}] numbers for every feed or [{S},{K}], one set per feed, got {tuple(weights.shape)}")
        return weights.expand(S, K).reshape(S * K)

    @torch.no_grad()
    def step(self, frames_u8, landmarks, *, weights=None, emotion_u8=None, inplace=False):
        """One tick: ``frames_u8`` uint8 ``[S,H,W,3]`` on the device, this tick's frame of every feed; ``landmarks`` device float32
        ``[S,K,2]`` (NaN for a feed with nothing to show); ``weights``: the tracker's confidences per feed ``[S,K]``, or one ``[K]`` set
        for all feeds, host numbers or a device float32 tensor; ``emotion_u8``: the frames ``Ee`` sees (None: ``frames_u8``).  ->
        uint8 ``[S,H,W,3]`` (``inplace=True``: ``frames_u8`` itself).  The steps are ``LiveSession.step``'s with the feeds as the batch;
        the number of launches does not depend on ``S``, and no device value is read on the host.

        ``frames_u8`` may also be a list or tuple of ``S`` tensors ``[H_s,W_s,3]`` -- every feed in a buffer of its own, of its own
        size, pixels packed, any row pitch -- or an ``ops.FrameTable`` of ``S`` frames, and ``emotion_u8`` then a list, tensor or table
        with the same size per feed.  The launches are those above with the three ``_table`` entry points of csrc/frame_table.hip in
        place of the strided three, plus one upload of ``24 S`` bytes per table; landmarks are in each feed's own frame coordinates.
        ``inplace=True`` writes into the caller's buffers (which must not share bytes) and returns the list; ``inplace=False`` clones
        every frame first -- ``S`` copies, the one cost of a tick that grows with ``S``, and a second table (host check and upload)
        over the clones -- and returns a list of new tensors.

        ``pixel_format="nv12"``: ``frames_u8`` is ``[S,3H/2,W]`` or a pair of planes (``ops.nv12_planes``) -- the strided NV12
        launchers; -> a packed clone ``[S,3H/2,W]``, or in place the input itself -- or a list / tuple of ``S`` surfaces of ``S``
        sizes (each a ``[3H/2,W]`` tensor of any even pitch or a pair of plane views, a region of interest included) or an
        ``ops.SurfaceTable``: the three ``_nv12_sim_table`` entry points of csrc/frame_table_nv12.hip plus one upload of ``40 S`` bytes
        per table.  ``inplace=True`` returns the list itself (no two planes may share bytes); ``inplace=False`` makes ``S`` packed
        clones and a second table over them, and returns a list of new tensors.

        ``pixel_format="i420"``: ``frames_u8`` is a contiguous packed ``[S,3H/2,W]`` tensor or a triple of planes ``(y [S,H,W],
        u [S,H/2,W/2], v [S,H/2,W/2])`` (``ops.i420_planes``) -- the strided I420 launchers -- or a list / tuple of ``S`` surfaces of
        ``S`` sizes (each a contiguous packed ``[3H/2,W]`` tensor or a triple of plane views of any pitch, odd ones included; a region
        of interest at even luma offsets is such a triple) or an ``ops.PlanarTable``: the three ``_i420_sim_table`` entry points of
        csrc/frame_table_i420.hip plus one upload of ``56 S`` bytes per table.  The returns are NV12's; the bytes and every state are
        those of the NV12 room on the interleaved surfaces.

        ``pixel_format="rgb32"``: ``frames_u8`` is ``[S,H,W,4]`` -- the strided RGB32 launchers -- or a list / tuple of ``S`` tensors
        ``[H_s,W_s,4]`` (pixels aligned 32-bit words, any row pitch that is a multiple of 4: a region of interest at any pixel
        offset of a wider surface is one) or an ``ops.Rgb32Table``: the three ``_rgb32_sim_table`` entry points of
        csrc/frame_table_rgb32.hip plus one upload of ``24 S`` bytes per table.  The returns are rgb24's; the colour bytes and every
        state are those of the rgb24 room on the stripped feeds, and no fourth byte changes."""
        what = "live_room.step"
        S, K = self.S, self.K
        given = frames_u8
        if self.edge.surfaces:
            if isinstance(frames_u8, self.edge.table) or (isinstance(frames_u8, (list, tuple)) and not self.edge.plane_tuple(frames_u8, S)):
                frames_u8 = self._table(what, "frames", frames_u8)
            else:
                frames_u8 = self.edge.open(what, "frames", frames_u8, S)
        elif isinstance(frames_u8, (list, tuple, self.edge.table)):
            frames_u8 = self._table(what, "frames", frames_u8)
        elif not isinstance(frames_u8, torch.Tensor) or frames_u8.dim() != 4 or frames_u8.size(3) != self.edge.channels or frames_u8.size(0) != S:
            got = tuple(frames_u8.shape) if isinstance(frames_u8, torch.Tensor) else type(frames_u8).__name__
            raise ValueError(f"{what}: frames must be [{S},H,W,{self.edge.channels}], one frame per feed, got {got}")
        if not isinstance(landmarks, torch.Tensor) or tuple(landmarks.shape) != (S, K, 2):
            got = tuple(landmarks.shape) if isinstance(landmarks, torch.Tensor) else type(landmarks).__name__
            raise ValueError(f"{what}: landmarks must be [{S},{K},2], {K} points per feed as the template has, got {got}")
        emotion_u8 = self._check_step(what, frames_u8, emotion_u8, inplace)
        weights = self._weights(what, weights)
        if self.track is None and weights is not None:                     # the fit takes them per frame
            weights = weights.view(S, K)
        out = self._body(what, frames_u8, landmarks, weights, emotion_u8, inplace)
        if not self.fixed_noise:
            self.frames.add_(1)
        if isinstance(out, (FR.FrameTable, FR.Rgb32Table)):                # in place: the caller's own list, or the table's tensors
            return given if inplace and isinstance(given, list) else list(out.frames)
        if isinstance(out, (FR.SurfaceTable, FR.PlanarTable)):             # the same of surfaces, as they were given
            return given if inplace and isinstance(given, list) else list(out.surfaces)
        return given if inplace else out

    def _table(self, what, name, frames):
        """This tick's frames of the ``S`` feeds in buffers of their own: a list / tuple of ``S`` tensors ``[H_s,W_s,3]``, a tensor
        ``[S,H,W,3]`` or a ``FrameTable`` -> a ``FrameTable`` of ``S`` frames on the room's device, none of them absent (a feed that
        sits out is given NaN landmarks); with NV12, ``S`` surfaces, ``[S,3H/2,W]``, a pair of planes or a ``SurfaceTable`` -> a
        ``SurfaceTable``"""
        S, edge = self.S, self.edge
        if not isinstance(frames, edge.table):
            if not isinstance(frames, (list, tuple, torch.Tensor)):
                raise ValueError(f"{what}: {name} must be a list of {S} {edge.noun}, a tensor {edge.shape.format(S)} or a {edge.table.__name__}, "
                                 f"got {type(frames).__name__}")
            pair = edge.surfaces and edge.plane_tuple(frames, S)           # one tuple of planes: its count is its planes'
            if not pair and len(frames) != S:
                raise ValueError(f"{what}: {name} must hold one frame per feed ({S}), got {len(frames)}")
            if not pair and not isinstance(frames, torch.Tensor) and any(f is None for f in frames):
                raise ValueError(f"{what}: {name} must hold a frame for every feed, got None among them (give a feed that sits out NaN landmarks)")
            frames = edge.table(frames)
        if len(frames) != S:
            raise ValueError(f"{what}: {name} must hold one frame per feed ({S}), got a table of {len(frames)}")
        if any(f is None for f in edge.present(frames)):
            raise ValueError(f"{what}: {name} must hold a frame for every feed, got an absent one (give a feed that sits out NaN landmarks)")
        if frames.device != self.device:
            raise L.SpkError(f"{what}: {name} on {frames.device}, the room on {self.device}")
        return frames
