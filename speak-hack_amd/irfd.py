"""``IRFD`` (model.py:28-126): three ResNet-50 trunk encoders (identity / emotion / pose), the
StyleGAN decoder ``Gd`` on their concatenated 6144-d latent, the discriminator ``D`` and the
emotion classifier ``Cm`` -- same attributes, methods, ``forward`` signature and 10-tuple result.

What differs from the reference, all on the host side and none in the arithmetic:
  * the per-forward debug work is gone: 12 ``.item()`` host syncs (``_log_feature_stats``,
    model.py:72-73,93-95), ~15 eagerly formatted DEBUG strings and two PNG files written to the CWD
    (``_visualize_feature_maps``, model.py:75-78,117-118).  ``IRFD.debug_side_effects = True``
    restores the statistics logging for anyone who wants it;
  * ``torch.utils.checkpoint`` (model.py:84-90) only changes *when* encoder activations exist, not
    their values; here the forward keeps no encoder activation beyond each block's output either
    way (BatchNorm/ReLU are folded into the consumers), and the backward pass recomputes.
The encoders are built with torchvision's own init (no download: ``resnet50(pretrained=True)`` at
model.py:61 needs the network, and ``self.apply(_init_weights)`` at model.py:48 re-initialises every
conv anyway, discarding the pretrained conv weights -- SURVEY.md 3.1 (iii)).
"""
from __future__ import annotations

import collections
import logging

import torch
import torch.nn as nn

from . import _lib as L
from . import autograd as AG
from . import frames as FR
from . import ops
from . import plan as PL
from .decoder import StyleGenerator
from .discriminator import StyleDiscriminator
from .encoder import GroupedTrunks, ResNet50Trunk


def _check_noise(what, noise, seed, noises, frame0):
    """The noise arguments of ``reenact`` / ``reenact_video`` (``what``: the caller's prefix), checked before any launch."""
    if noise not in ("fresh", "fixed"):
        raise ValueError(f"{what}: noise must be 'fresh' or 'fixed', got {noise!r}")
    if seed is None and noise == "fixed":
        raise ValueError(f"{what}: noise='fixed' needs a seed")
    if seed is not None:
        if noises is not None:
            raise ValueError(f"{what}: pass either seed or noises, not both")
        ops.check_seed(seed, frame0, f"{what}: seed")


class IRFD(nn.Module):
    debug_side_effects = False
    # Ei, Ee, Ep run the same ResNet-50 on the same image: by default every layer of the three is ONE grouped launch
    # (encoder.GroupedTrunks); False runs them one after another as the reference does.  Same parameters, same results.
    group_encoders = True
    pair_decoder = True          # the two Gd calls of a forward as one pass over both batches (StyleGenerator.forward_pair)

    def __init__(self, max_resolution=256):
        super().__init__()
        self.Ei = self._create_encoder()   # identity
        self.Ee = self._create_encoder()   # emotion
        self.Ep = self._create_encoder()   # pose
        self.Gd = StyleGenerator(input_dim=6144)
        self.D = StyleDiscriminator()
        self.Cm = nn.Linear(2048, 8)
        self.max_resolution = max_resolution
        self.current_resolution = max_resolution
        self.logger = logging.getLogger(__name__)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, (nn.Conv2d, nn.Linear)):          # model.py:50-54
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)

    def adjust_for_resolution(self, resolution):
        self.current_resolution = resolution

    def _create_encoder(self):
        return ResNet50Trunk()

    def _prepare_generator_input(self, *features):
        return torch.cat([f.view(f.size(0), -1) for f in features], dim=1)

    def _log_feature_stats(self, tensor, name):
        if self.debug_side_effects and self.logger.isEnabledFor(logging.DEBUG):
            self.logger.debug("%s stats: mean=%.4f, std=%.4f, min=%.4f, max=%.4f", name, tensor.mean().item(),
                              tensor.std().item(), tensor.min().item(), tensor.max().item())

    def _emotion(self, fe):
        logits = AG.fc(fe.view(fe.size(0), -1), self.Cm.weight, self.Cm.bias, 1.0, 1.0, 1.0)
        return torch.softmax(logits, dim=1)

    # ---- inference entry points (inference.py:60-76: Ei(identity_image), Ep(pose_video), Ee(emotion_video), then generate) ----
    @torch.no_grad()
    def encode(self, images, which):
        """``images`` [B,3,H,W] -> features [B,2048,1,1] of the trunk ``which`` ("Ei" | "Ee" | "Ep") in eval arithmetic -- running
        statistics in every BatchNorm whatever ``self.training`` is, no buffer updated -- on the trunk's BatchNorm-folded launch
        plan (``plan.EncoderPlan``: one call across the C boundary)."""
        if which not in ("Ei", "Ee", "Ep"):
            raise ValueError(f"encode: which must be 'Ei', 'Ee' or 'Ep', got {which!r}")
        if images.dim() != 4 or images.size(1) != 3 or images.size(0) < 1:
            raise ValueError(f"encode: images must be [B,3,H,W], got {tuple(images.shape)}")
        if not images.is_cuda or images.dtype != torch.float32:
            raise L.SpkError(f"images: expected a float32 HIP tensor, got {images.dtype} on {images.device} (no CPU path)")
        trunk = getattr(self, which)
        B, _, H, W = images.shape
        key = (B, H, W, images.device, torch.cuda.current_stream(images.device).cuda_stream, "encoder")
        return PL.plan_for(trunk, key, lambda: PL.EncoderPlan(trunk, B, H, W, images.device)).run(images)

    @torch.no_grad()
    def reenact(self, identity_image, pose_frames, emotion_frames=None, *, noises=None, chunk=8, output="f32", channel_order="rgb",
                seed=None, noise="fresh", frame0=0, standard="bt601", full_range=False):
        """Talking-head frames: ``Gd(cat(Ei(identity).expand(T), Ee(emotion_frames), Ep(pose_frames)))`` in the feature order
        of ``_prepare_generator_input(fi, fe, fp)`` (model.py:64-69,107), in eval arithmetic whatever ``self.training`` is: no
        buffer update, no host-RNG draw, no swap, no style mixing, truncation as ``StyleGenerator.forward`` applies it in eval.
        ``identity_image`` [1,3,H,W]; ``pose_frames`` / ``emotion_frames`` [T,3,H,W] (None: the pose frames); ``noises``: the
        explicit list ``StyleGenerator.forward`` takes, for T frames (default: drawn on the device).  ``Ei`` runs once; the
        frames go through the encoder and decoder plans ``chunk`` at a time.  -> frames [T,3,R,R] fp32; with ``output="uint8"``
        uint8 [T,R,R,3] in ``channel_order`` ("rgb" | "bgr"), quantised from (-1, 1) by the last op of the decoder plan --
        ``ops.frames_to_u8`` of the fp32 result, bit for bit.  ``output="nv12"``: uint8 [T,3R/2,R] NV12 surfaces (rows ``R..`` are the
        interleaved UV plane) in the colour of ``standard`` ("bt601" | "bt709") / ``full_range``, converted by the last op of the
        decoder plan -- ``ops.frames_to_nv12`` of the fp32 result, bit for bit.  ``output="i420"``: packed uint8 [T,3R/2,R] I420
        surfaces in that colour -- the ``R`` rows of Y, then the ``R^2 / 4`` bytes of U, then those of V, what ``ops.i420_planes``
        takes -- ``ops.frames_to_i420`` of the fp32 result, bit for bit.  ``output="rgb32"``: uint8 [T,R,R,4] in ``channel_order``
        ("rgba" | "bgra" | "argb" | "abgr": ``ops.rgb32_order``; the default "rgb" raises) with the fourth byte 255, by the last op of
        the decoder plan -- ``ops.frames_to_rgb32`` of the fp32 result, bit for bit.

        ``seed`` (0 <= seed < 2**64; not together with ``noises``): reproducible noise, a function of (seed, frame index,
        layer, pixel) drawn inside the decoder's launch list (``ops.decoder_noise`` gives the same tensors explicitly); the
        device generator is not touched.  Frame ``t`` of the clip has frame index ``frame0 + t`` whatever ``chunk`` is, so
        frames ``[a, b)`` of a longer clip may be rendered elsewhere with ``frame0=a``.  ``noise="fixed"`` (needs a seed): every
        frame uses frame index ``frame0`` -- one noise image per layer held over the clip, as StyleGAN video pipelines do
        against boiling texture; ``"fresh"`` (default): new noise on every frame."""
        if output not in ("nv12", "i420") and (standard != "bt601" or full_range):
            raise ValueError("reenact: standard / full_range apply to nv12 output only, and to i420")
        out = [y for _, _, y in self._reenact_chunks(identity_image, pose_frames, emotion_frames, noises, chunk, output, channel_order,
                                                     seed, noise, frame0, (standard, full_range))]
        return out[0] if len(out) == 1 else torch.cat(out, 0)

    def _reenact_chunks(self, identity_image, pose_frames, emotion_frames, noises, chunk, output, channel_order, seed, noise, frame0,
                        colour=("bt601", False)):
        """``reenact``'s argument checks and chunk loop: yields ``(t0, t1, frames of [t0, t1))``."""
        if output not in ("f32", "uint8", "nv12", "i420", "rgb32"):
            raise ValueError(f"reenact: output must be 'f32', 'uint8', 'nv12' or 'i420', got {output!r} (or 'rgb32')")
        FR.yuv_standard(*colour)
        _check_noise("reenact", noise, seed, noises, frame0)
        if seed is None and frame0 != 0:
            raise ValueError("reenact: frame0 applies to seeded noise only")
        if output == "rgb32":                                              # one of the four orders of a 4-byte pixel: "rgb" is none of them
            FR.rgb32_order(channel_order)
        else:
            if channel_order not in ("rgb", "bgr"):
                raise ValueError(f"reenact: channel_order must be 'rgb' or 'bgr', got {channel_order!r}")
            if output != "uint8" and channel_order != "rgb":
                raise ValueError("reenact: channel_order applies to uint8 output only")
        if identity_image.dim() != 4 or identity_image.size(0) != 1 or identity_image.size(1) != 3:
            raise ValueError(f"reenact: identity_image must be [1,3,H,W], got {tuple(identity_image.shape)}")
        if pose_frames.dim() != 4 or pose_frames.size(1) != 3 or pose_frames.size(0) < 1:
            raise ValueError(f"reenact: pose_frames must be [T,3,H,W], got {tuple(pose_frames.shape)}")
        if emotion_frames is None:
            emotion_frames = pose_frames
        if tuple(emotion_frames.shape) != tuple(pose_frames.shape):
            raise ValueError(f"reenact: emotion_frames must match pose_frames {tuple(pose_frames.shape)}, got {tuple(emotion_frames.shape)}")
        T, chunk = pose_frames.size(0), int(chunk)
        if chunk < 1:
            raise ValueError("reenact: chunk must be >= 1")
        if noises is not None and any(n.size(0) != T for n in noises):
            raise ValueError(f"reenact: every noise tensor must carry {T} frames")
        fi = self.encode(identity_image, "Ei")
        for t0 in range(0, T, chunk):
            t1 = min(T, t0 + chunk)
            fe, fp = self.encode(emotion_frames[t0:t1], "Ee"), self.encode(pose_frames[t0:t1], "Ep")
            gin = self._prepare_generator_input(fi.expand(t1 - t0, -1, -1, -1), fe, fp)
            seeded = None if seed is None else dict(seed=seed, frame0=frame0 if noise == "fixed" else frame0 + t0, fixed_noise=noise == "fixed")
            yield t0, t1, self._decode_eval(gin, None if noises is None else [n[t0:t1] for n in noises], output, channel_order, seeded, colour)

    @torch.no_grad()
    def reenact_video(self, identity_u8, pose_u8, emotion_u8=None, *, size=256, crop=None, channel_order="rgb", noises=None, chunk=8,
                      seed=None, noise="fresh", frame0=0, paste=False, feather=0, inplace=False, pixel_format="rgb24", standard="bt601",
                      full_range=False, align=None, identity_align=None, matte=None, colour_match=False, colour_smooth=0, colour_sigma=None):
        """``reenact`` from and to video frames as a decoder and a video writer hold them (inference.py:29-33,46-58,78-86):
        uint8 HWC frames of any size on the device in, uint8 [T,R,R,3] out, both in ``channel_order`` ("bgr": ``cv2``'s).
        Nothing but ``ops.frames_from_u8`` -> ``reenact(output="uint8")``: ``identity_u8`` [H,W,3] or [1,H,W,3] is resized whole
        to ``size`` (``identity_align`` below: cropped); ``pose_u8`` / ``emotion_u8`` [T,H,W,3] are cropped to ``crop`` and resized; ``emotion_u8=None``: the pose
        frames, resized once.  ``crop``: ``(y0, x0, h, w)``, one box for all frames; a host sequence / CPU integer tensor
        ``[T,4]``, a tracker's box per frame, all of one size (``align=`` below: any size and angle per frame); or
        ``(boxes_yx, h, w)`` with a device int32 ``[T,2]`` tensor of origins (``ops.frames_from_u8``).  ``seed`` / ``noise`` / ``frame0``: as ``reenact``.

        ``paste=True``: the full frames back -- uint8 [T,H,W,3], the pose frames with every generated face resized to its box
        and pasted where the crop came from (``crop=None``: the whole frame), blended over ``feather`` pixels at the box's
        edge (``ops.frames_paste_u8``).  The result is one clone of ``pose_u8`` (``inplace=True``: ``pose_u8`` itself); each
        chunk's fp32 decoder result is pasted straight into its slice, one ``spk_frames_paste_u8`` launch per chunk, and
        per-frame boxes are taken per frame, so the result does not depend on ``chunk``.

        ``pixel_format="nv12"``: ``pose_u8`` / ``emotion_u8`` are NV12 as a hardware decoder leaves them -- one uint8 tensor
        ``[T,3H/2,W]`` (any row pitch; rows ``H..`` are the UV plane) or a pair ``(y [T,H,W], uv [T,H/2,W/2,2])``
        (``ops.nv12_planes``), in the colour of ``standard`` ("bt601" | "bt709") / ``full_range`` -- and so is the result:
        ``[T,3R/2,R]``, or with ``paste=True`` the pose surfaces with every face pasted back (``ops.frames_from_nv12``,
        ``reenact(output="nv12")``, ``ops.frames_paste_nv12``: one launch per chunk).  The identity image stays a uint8 HWC photo
        in ``channel_order``; ``crop`` keeps its three forms and may have an odd origin.

        ``pixel_format="i420"``: the same for I420 (``yuv420p``) as a software decoder leaves it -- one CONTIGUOUS packed uint8 tensor
        ``[T,3H/2,W]`` or a triple of planes ``(y [T,H,W], u [T,H/2,W/2], v [T,H/2,W/2])`` with any pitch, base and order in memory
        (``ops.i420_planes``; YV12 is the triple with the planes swapped) -- through ``ops.frames_from_i420``,
        ``reenact(output="i420")`` and ``ops.frames_paste_i420``: one ``spk_frames_paste_i420`` launch per chunk, in place into the
        decoder's own planes with ``inplace=True``, and no interleaving into scratch NV12 surfaces.  The Y, U and V bytes are those
        of ``pixel_format="nv12"`` on the interleaved clip.  The identity photo stays packed RGB.

        ``pixel_format="rgb32"``: ``pose_u8`` / ``emotion_u8`` are uint8 ``[T,H,W,4]`` as a capture surface, an interop texture or a
        compositor holds them, and ``channel_order`` is one of ``"rgba"``, ``"bgra"``, ``"argb"``, ``"abgr"`` (an ``X`` byte counts as
        the ``a``; the default ``"rgb"`` raises) -- through ``ops.frames_from_rgb32``, ``reenact(output="rgb32")`` and
        ``ops.frames_paste_rgb32``: one ``spk_frames_paste_rgb32`` launch per chunk and no strip of the fourth byte into a packed scratch
        clip.  Everything ``"rgb24"`` takes works -- ``crop`` in its three forms, ``paste``, ``feather``, ``inplace`` (the clip's pixels
        must be aligned 32-bit words: ``ops.rgb32_pixels``), ``align``, ``identity_align``, ``matte``, ``colour_match``,
        ``colour_smooth`` (the ``_rgb32`` launchers of the aligned edge) -- and the colour bytes are those of ``"rgb24"`` on the clip with
        the fourth byte stripped.  Without ``paste`` the result is ``[T,R,R,4]`` with the fourth byte 255; with ``paste`` every fourth
        byte of the result is the pose frame's.  The identity photo stays a packed ``[H,W,3]`` photo in the colour order with the alpha
        dropped (``rgba`` / ``argb``: ``rgb``; ``bgra`` / ``abgr``: ``bgr``).  ``standard`` / ``full_range`` are refused.

        ``align=sim`` (instead of ``crop``; both: ``ValueError``): an aligned crop per frame -- rows ``(a, c, tx, ty)`` of the
        similarity transform that maps the ``size`` network image into frame ``t`` (``ops.similarity_rows``; include/spk.h), any
        scale and angle per frame, as ``ops.similarity_from_landmarks`` fits them to a tracker's landmarks: a host sequence / CPU
        tensor ``[T,4]``, checked on the host and uploaded once; a device float32 ``[T,4]`` tensor, not read on the host; or an
        ``ops.LandmarkAlign`` -- the landmarks themselves, fitted (and smoothed over the whole clip) on the device once per call,
        before the chunk loop; the pose and the emotion frames share the rows.  ``pose_u8`` / ``emotion_u8`` go through
        ``ops.frames_from_u8_aligned``; with ``paste=True`` each chunk's fp32 result goes through ``ops.frames_paste_u8_aligned``
        into its slice, one ``spk_frames_paste_u8_sim`` launch per chunk, rows taken per frame, so the result does not depend on
        ``chunk``.  The generated image has ``R`` pixels where the network image has ``size``: the paste uses the rows with
        ``(a, c)`` scaled by ``size / R`` in fp32.  Packed RGB and RGB32 only: ``align`` with ``pixel_format="nv12"`` or ``"i420"`` raises
        ``ValueError`` (NV12 and I420 frames take crop boxes).

        ``identity_align``: the identity photo through an aligned crop as well, so that ``Ei`` sees a face framed as ``Ee`` / ``Ep``
        see theirs -- one row in either form above (``[1,4]``; host rows are checked before any launch) or an ``ops.LandmarkAlign``
        over one frame; the photo then goes through ``ops.frames_from_u8_aligned`` instead of being resized whole.  The photo is
        packed in both pixel formats, so this works with both.  ``None``: resized whole, as ever.

        ``matte`` / ``colour_match`` (both need ``align=``, ``paste=True`` and packed RGB; anything else: ``ValueError`` before any
        launch): a seamless paste.  ``matte``: a float32 ``[R,R]`` (one for the clip: ``ops.ellipse_matte``) or ``[T,R,R]`` tensor
        in the generated image's size where the frames are, multiplied into the blend weight so that only the face is pasted, not
        the generator's own background; or an ``ops.LandmarkMatte`` -- the outline through some of the tracked landmarks, by default
        those of ``align=LandmarkAlign(...)``, rasterised and smoothed over the clip on the device (``ops.matte_from_landmarks``): one
        ``spk_matte_from_landmarks`` launch per call, at the first chunk, from the rows the paste uses, then sliced per chunk as a
        ``[T,R,R]`` tensor is, so the result does not depend on ``chunk``.  ``colour_match=True``: per frame and channel the
        generated face is brought to the mean and standard deviation of the pixels it replaces (``ops.paste_colour_match``) -- each chunk makes one
        ``spk_paste_colour_match_sim`` call, then one ``spk_frames_paste_u8_sim_blend`` call (``ops.frames_paste_u8_aligned(matte=,
        colour=)``) with the rows the paste uses anyway.  The statistics are per frame and read the background before the paste, on
        the same stream: the result depends neither on ``chunk`` nor on ``inplace``.

        ``colour_smooth=r`` / ``colour_sigma`` (anything but ``0`` / ``None`` needs ``colour_match=True``; ``ValueError`` before any
        launch otherwise): the colour match without flicker.  The background under the matte changes from frame to frame, and rows
        made per frame follow it; with ``r > 0`` the 13 sums of the statistics are pooled over frames ``t - r ... t + r`` with
        weights ``exp(-d^2 / (2 colour_sigma^2))`` (``None``: ``max(r, 1) / 2``) before the row formula
        (``ops.colour_rows_from_sums``; a frame without usable statistics is bridged from its neighbours).  One float64 ``[T,13]``
        tensor per call; each chunk's sums go into its slice as soon as it is generated (``ops.paste_colour_sums``), and its paste
        LAGS: a generated chunk ``[t0, t1)`` is held until the sums of frames up to ``t1 - 1 + r`` exist, or the clip ends, and is
        then pasted with the rows of its own frames (one ``spk_colour_rows_window`` and one ``spk_frames_paste_u8_sim_blend`` call), so
        at most ``r + 2 chunk`` generated frames are held.  The statistics of frame ``j`` read frame ``j`` only, before its paste, and
        the paste of frame ``j`` writes frame ``j`` only: here too the result depends neither on ``chunk`` nor on ``inplace``.
        ``colour_smooth=0``: the calls the method always made."""
        if pixel_format not in FR.PIXEL_FORMATS:
            raise ValueError(f"reenact_video: pixel_format must be 'rgb24' or 'nv12' or 'i420' or 'rgb32', got {pixel_format!r}")
        if pixel_format in ("rgb24", "rgb32") and (standard != "bt601" or full_range):
            raise ValueError("reenact_video: standard / full_range apply to pixel_format='nv12' only, and to 'i420'")
        FR.yuv_standard(standard, full_range)
        feather = float(feather)
        if inplace and not paste:
            raise ValueError("reenact_video: inplace applies to paste=True only")
        if not paste and feather != 0:
            raise ValueError("reenact_video: feather applies to paste=True only")
        FR.check_feather(feather, "reenact_video")
        _check_noise("reenact_video", noise, seed, noises, frame0)
        if align is not None and crop is not None:
            raise ValueError("reenact_video: crop and align are two ways to say where the face is: give one")
        if align is not None and pixel_format not in ("rgb24", "rgb32"):
            raise ValueError("reenact_video: align applies to pixel_format='rgb24' only (NV12 frames take crop boxes)")
        if not isinstance(colour_match, bool):
            raise ValueError(f"reenact_video: colour_match must be a bool, got {colour_match!r}")
        if colour_smooth != 0 or colour_sigma is not None:
            if not colour_match:
                raise ValueError("reenact_video: colour_smooth / colour_sigma apply to colour_match=True only")
            colour_smooth, colour_sigma = FR._check_smooth(colour_smooth, colour_sigma, "reenact_video: colour_smooth")
        blend, landmark_matte = {}, None
        if matte is not None or colour_match:
            if align is None or not paste:
                raise ValueError("reenact_video: matte / colour_match apply to align= with paste=True only")
            if isinstance(matte, FR.LandmarkMatte):                        # made at the first chunk, when the generated size is known
                landmark_matte, matte = matte, None
            elif matte is not None and (not isinstance(matte, torch.Tensor) or matte.dtype != torch.float32 or matte.dim() not in (2, 3)):
                got = f"{matte.dtype} {tuple(matte.shape)}" if isinstance(matte, torch.Tensor) else type(matte).__name__
                raise ValueError(f"reenact_video: matte must be a float32 tensor [R,R] or [T,R,R] in the generated image's size, or an "
                                 f"ops.LandmarkMatte, got {got}")
            blend = dict(matte=matte, colour_match=colour_match)
        fmt = FR.PIXEL_FORMATS[pixel_format](channel_order, standard, full_range)
        if pixel_format == "rgb32":                                        # the identity photo stays packed: the colour order with the alpha dropped
            channel_order = FR.rgb32_order(channel_order)[0]
        if identity_align is not None:                                    # host rows: checked here, before any launch
            identity_align = FR.Aligned.parse(identity_align, 1, size, identity_u8.device, "reenact_video: identity_align")
        pose_in = pose_u8
        if align is not None:                                              # the transforms stand where a box would: checked / uploaded once
            pose_in, device, T, H, W = fmt.open(pose_u8, inplace)
            if matte is not None and matte.dim() == 3 and matte.size(0) != T:
                raise ValueError(f"reenact_video: a per-frame matte must carry {T} frames, got {tuple(matte.shape)}")
            if landmark_matte is not None:                                 # the carrier against align= and T: on the host, before any launch
                landmark_matte = landmark_matte.bind(align, T)
            crop = FR.Aligned.parse(align, T, size, device)
        elif crop is not None or paste or fmt.needs_box:
            pose_in, device, T, H, W = fmt.open(pose_u8, inplace)
            origins, h, w = FR.parse_boxes((0, 0, H, W) if crop is None else crop, T, H, W, "reenact_video: crop")
            if not isinstance(origins, tuple) and not origins.is_cuda and device.type == "cuda":
                origins = origins.to(device)                               # host boxes: checked above, uploaded once for both edges
            crop = (*origins, h, w) if isinstance(origins, tuple) else (origins, h, w)
        if identity_align is None:
            ident = FR.frames_from_u8(identity_u8, size, channel_order=channel_order)
        else:
            ident = FR.frames_from_u8_aligned(identity_u8, size, identity_align.rows, channel_order=channel_order)
        pose = fmt.network_input(pose_in, size, crop)
        emo = None if emotion_u8 is None else fmt.network_input(emotion_u8, size, crop)
        if not paste:
            return self.reenact(ident, pose, emo, noises=noises, chunk=chunk, output=fmt.output, seed=seed, noise=noise, frame0=frame0,
                                **fmt.args)
        result, out = (pose_u8, pose_in) if inplace else fmt.clone(pose_in)
        held, sums = collections.deque(), None                             # colour_smooth > 0: generated chunks whose paste lags
        for t0, t1, y in self._reenact_chunks(ident, pose, emo, noises, chunk, "f32", "rgb", seed, noise, frame0):
            where = crop.chunk(t0, t1, y) if align is not None else crop if len(crop) == 4 else (crop[0][t0:t1], h, w)
            if landmark_matte is not None:                                 # once per clip: the window sees every frame, whatever the chunk
                blend["matte"], landmark_matte = landmark_matte(crop.chunk(0, T, y), crop.size), None
            if colour_smooth == 0:
                fmt.paste(y, out, t0, t1, where, feather, **blend)
                continue
            if sums is None:                                               # the first chunk: the sums of the clip, one tensor per call
                sums = torch.empty((T, FR.COLOUR_SUMS), device=device, dtype=torch.float64)
            fmt.colour_sums(y, out, t0, t1, where, feather, blend["matte"], sums)
            held.append((t0, t1, y, where))
            while held and (held[0][1] + colour_smooth <= t1 or t1 == T):  # the sums of its last frame's window exist, or never will
                p0, p1, py, pwhere = held.popleft()
                rows = FR.colour_rows_from_sums(sums, colour_smooth, colour_sigma, start=p0, stop=p1)
                fmt.paste_matched(py, out, p0, p1, pwhere, feather, blend["matte"], rows)
        return result

    @torch.no_grad()
    def live(self, identity_u8, *, size=256, template, contour=None, channel_order="rgb", identity_align=None, rate=30.0,
             track=FR.FILTER_DEFAULTS, features=None, feather=0, matte_softness=4.0, matte_grow=0.0, colour_match=False, colour_decay=0.9,
             seed=None, noise="fresh", offset=0.0, pixel_format="rgb24", standard="bt601", full_range=False):
        """A reenactment session for a LIVE feed -- a camera or a call, where frame ``t + 1`` does not exist yet, or a long video
        pushed through a few frames at a time: ``reenact_video(align=LandmarkAlign(...), paste=True, ...)`` with the clip's windows
        replaced by causal filters whose state stays on the device (speak-hack_amd/live.py; csrc/causal_filter.hip).  Everything is
        checked on the host (``ValueError``) before a device is touched; then ``Ei`` runs ONCE, on ``identity_u8`` ([H,W,3] or
        [1,H,W,3], resized whole to ``size``, or cropped through ``identity_align``: as ``reenact_video``), and the session keeps
        ``fi``.  -> a ``LiveSession``; ``session.step(frames_u8 [N,H,W,3], landmarks [N,K,2] device float32, *, weights=None,
        emotion_u8=None, inplace=False)`` -> uint8 ``[N,H,W,3]``, the next ``N`` frames with the face pasted in.  Per ``step``:

          1. ``ops.causal_filter`` over the landmarks (``track``: a dict over ``min_cutoff``, ``beta``, ``d_cutoff``, ``hold``, the
             defaults of that launcher where a key is missing; None: the raw landmarks) -- a one-euro filter per landmark at ``rate``
             frames per second, which holds a landmark over a drop-out of up to ``hold`` frames;
          2. ``spk_sim_fit_landmarks`` of ``template`` ([K,2], the landmarks in the ``size`` network image; ``offset``: as
             ``ops.similarity_from_landmarks``) on the filtered points with the filter's weights: a held point counts as it last did;
          3. ``ops.frames_from_u8_aligned`` of the frames (and of ``emotion_u8``) with these rows;
          4. ``Ee`` and ``Ep``: two launch lists;
          5. with ``features`` (a dict as ``track``; None: off) the same filter with ``group=1`` over the emotion and pose features --
             the identity part is not touched -- in which a frame without a transform takes no part;
          6. the decoder, one launch list, with ``seed`` and frame index = the frames seen so far (``noise="fixed"``: index 0);
          7. with ``contour`` (landmark indices in outline order) ``ops.matte_from_landmarks(smooth=0, softness=matte_softness,
             grow=matte_grow)`` from the FILTERED points, the template's contour as fallback: the filter is the matte's steadiness;
          8. with ``colour_match`` ``ops.paste_colour_sums`` and ``ops.colour_rows_causal(decay=colour_decay)``;
          9. ``ops.frames_paste_u8_aligned(matte=, colour=, feather=)``: one launch.

        A frame whose row is not finite (the landmarks lost for more than ``hold`` frames) passes through untouched.  Nothing in
        ``step`` reads a device value on the host, and ``N`` frames in one step and the same frames in any split of steps give the
        same bytes.  With ``track=None``, ``features=None``, ``colour_decay=0`` and frames that all have landmarks, a ``step`` over a
        clip is ``reenact_video(align=LandmarkAlign(landmarks, template), paste=True, matte=LandmarkMatte(contour, smooth=0, ...),
        colour_match=True, ...)`` byte for byte.  ``session.reset()`` empties the filter states and the frame counter
        (``session.frames``); ``fi`` stays.  Several feeds at once: ``live_room``.

        ``pixel_format="nv12"``: the feed is NV12 as a hardware decoder leaves it, in the colour of ``standard`` ("bt601" | "bt709") /
        ``full_range`` (``ValueError`` with ``"rgb24"``, as ``reenact_video``).  ``step`` then takes the next ``N`` surfaces as one uint8
        tensor ``[N,3H/2,W]`` or a pair of planes (``ops.nv12_planes``), and ``emotion_u8`` in the same form and size; steps 3, 8 and 9
        are ``ops.frames_from_nv12_aligned`` (R, G, B planes), ``ops.paste_colour_sums_nv12`` and ``ops.frames_paste_nv12_aligned`` --
        no packed-RGB detour -- and everything else is untouched: the landmark filter never sees a pixel.  -> a packed uint8
        ``[N,3H/2,W]`` clone with the face pasted in, or with ``inplace=True`` the input itself (whose frames must not overlap).  The
        identity photo stays a packed photo in ``channel_order``.

        ``pixel_format="i420"`` (the name is exactly that): the feed is I420 as a software decoder or a WebRTC frame buffer holds it --
        three planes, each with a base and a pitch of its own -- in the colour of ``standard`` / ``full_range``.  ``step`` takes one
        contiguous packed tensor ``[N,3H/2,W]`` or a triple of planes (``ops.i420_planes``); steps 3, 8 and 9 are
        ``ops.frames_from_i420_aligned``, ``ops.paste_colour_sums_i420`` and ``ops.frames_paste_i420_aligned`` -- no interleaving into a
        scratch NV12 surface -- and the bytes and every state are those of the NV12 session on the interleaved surfaces.

        ``pixel_format="rgb32"``: the feed is four bytes per pixel as a capture surface, an interop texture or an ARGB buffer holds it,
        and ``channel_order`` is one of ``"rgba"``, ``"bgra"``, ``"argb"``, ``"abgr"`` (an ``X`` byte counts as the ``a``).  ``step`` takes
        uint8 ``[N,H,W,4]`` whose pixels are aligned 32-bit words (``ops.frames_from_rgb32_aligned``); steps 3, 8 and 9 are
        ``ops.frames_from_rgb32_aligned``, ``ops.paste_colour_sums_rgb32`` and ``ops.frames_paste_rgb32_aligned`` -- no strip of the
        alpha into scratch frames -- and the colour bytes and every state are those of the rgb24 session on the stripped feed; the
        fourth byte of every pixel is left as it was.  The identity photo stays a packed ``[H,W,3]`` photo in the colour order with the
        alpha dropped (``rgba`` / ``argb``: ``rgb``; ``bgra`` / ``abgr``: ``bgr``).  ``standard`` / ``full_range`` are refused."""
        from .live import LiveSession
        return LiveSession(self, identity_u8, size=size, template=template, contour=contour, channel_order=channel_order,
                           identity_align=identity_align, rate=rate, track=track, features=features, feather=feather,
                           matte_softness=matte_softness, matte_grow=matte_grow, colour_match=colour_match, colour_decay=colour_decay, seed=seed,
                           noise=noise, offset=offset, pixel_format=pixel_format, standard=standard, full_range=full_range)

    @torch.no_grad()
    def live_room(self, identities_u8, *, size=256, template, contour=None, channel_order="rgb", identity_align=None, rate=30.0,
                  track=FR.FILTER_DEFAULTS, features=None, feather=0, matte_softness=4.0, matte_grow=0.0, colour_match=False,
                  colour_decay=0.9, seed=None, noise="fresh", offset=0.0, pixel_format="rgb24", standard="bt601", full_range=False):
        """``live`` for ``S`` feeds at once -- a server with several calls -- stepped together as ONE batch per tick
        (speak-hack_amd/live.py: ``LiveRoom``).  The arguments are those of ``live``, with ``identities_u8`` a sequence of ``S`` photos
        of any sizes ([H,W,3] or [1,H,W,3] each) or a tensor ``[S,H,W,3]``; ``seed`` one integer or ``S`` of them; ``identity_align``
        None, or one entry (None or as ``live`` takes it) per photo.  Everything is checked on the host (``ValueError``) before a
        device is touched; then ``Ei`` runs once per photo at batch 1, as a session runs it.  -> a ``LiveRoom``;
        ``room.step(frames_u8 [S,H,W,3], landmarks [S,K,2], *, weights=None, emotion_u8=None, inplace=False)`` -> uint8 ``[S,H,W,3]``
        takes one frame per feed per tick and runs the nine steps of ``live`` with the feeds as the batch: 3 launch lists, 1 landmark
        filter (2 with ``features``), 1 fit, 1 crop, 1 matte, 1 sums, 1 ``spk_colour_rows_causal_feeds``, 1 paste, whatever ``S`` is; the
        decoder's noise row ``s`` is that of ``(seed[s], the ticks slot s has seen)``, read from device tables
        (``spk_noise_fill_rows``).  Slot ``s`` of a room is a session of its own (the networks run at batch ``S``: the same frames once
        quantised, as the chunks of ``reenact_video`` are); a feed with nothing to show in a tick is given NaN landmarks.
        ``room.reset(slot=None)`` and ``room.set_identity(slot, photo, identity_align=None)`` start a slot over without touching its
        neighbours.  The feeds' frames may also be ``S`` buffers of ``S`` sizes (``LiveRoom.step``).

        ``pixel_format="nv12"`` (``standard``, ``full_range``: as ``live``): ``room.step`` takes this tick's surfaces as ``[S,3H/2,W]`` or
        a pair of planes -- the strided NV12 launchers -- or as a list / tuple of ``S`` surfaces of ``S`` sizes or an
        ``ops.SurfaceTable``: the three ``_nv12_sim_table`` entry points of csrc/frame_table_nv12.hip plus one upload of ``40 S`` bytes per
        table, each feed's decoder surface read and written where it is.

        ``pixel_format="i420"``: the same for I420 -- ``[S,3H/2,W]`` packed and contiguous or a triple of planes, or a list / tuple of
        ``S`` surfaces of ``S`` sizes (packed tensors or triples of plane views) or an ``ops.PlanarTable``: the three ``_i420_sim_table``
        entry points of csrc/frame_table_i420.hip plus one upload of ``56 S`` bytes per table.

        ``pixel_format="rgb32"`` (``channel_order``: as ``live``): ``room.step`` takes ``[S,H,W,4]``, or a list / tuple of ``S`` frames
        ``[H_s,W_s,4]`` of ``S`` sizes (region-of-interest views at any pixel offset included) or an ``ops.Rgb32Table``: the three
        ``_rgb32_sim_table`` entry points of csrc/frame_table_rgb32.hip plus one upload of ``24 S`` bytes per table."""
        from .live import LiveRoom
        return LiveRoom(self, identities_u8, size=size, template=template, contour=contour, channel_order=channel_order,
                        identity_align=identity_align, rate=rate, track=track, features=features, feather=feather,
                        matte_softness=matte_softness, matte_grow=matte_grow, colour_match=colour_match, colour_decay=colour_decay, seed=seed,
                        noise=noise, offset=offset, pixel_format=pixel_format, standard=standard, full_range=full_range)

    def _decode_eval(self, gin, noises, output="f32", channel_order="rgb", seeded=None, colour=("bt601", False)):
        """``Gd`` in eval arithmetic without touching module state: its inference plan called directly; a decoder the plan
        does not serve runs its eval branch with every submodule's own ``training`` flag saved and put back.  ``seeded``: the
        ``seed`` / ``frame0`` / ``fixed_noise`` keywords of a seeded call (``StyleGenerator`` decoders), else None; or
        ``dict(seed_rows=, frame_rows=)``, device int64 ``[B]`` tables with one (seed, frame) per batch row (``ops.noise_fill_rows``)."""
        Gd = self.Gd
        seeded = seeded or {}
        if "seed_rows" in seeded and not (hasattr(Gd, "plan_serves") and Gd.plan_serves(gin)):
            if noises is not None:
                raise ValueError("pass either seed_rows and frame_rows or noises, not both")
            noises, seeded = ops.decoder_noise_rows(Gd.synthesis.noise_shapes(gin.size(0)), seeded["seed_rows"], seeded["frame_rows"]), {}
        if hasattr(Gd, "plan_serves") and Gd.plan_serves(gin):
            how = {"f32": {}, "uint8": dict(output=output, swap_rb=channel_order == "bgr"),
                   "nv12": dict(output=output, standard=colour[0], full_range=colour[1]),
                   "i420": dict(output=output, standard=colour[0], full_range=colour[1]),
                   "rgb32": dict(output=output, channel_order=channel_order)}[output]
            return Gd.plan_forward(gin, noises, **how, **seeded)
        flags = [(mod, mod.training) for mod in Gd.modules()]
        try:
            for mod, _ in flags:
                mod.training = False
            y = Gd(gin, noises, **seeded)
        finally:
            for mod, was in flags:
                mod.training = was
        if output == "nv12":
            return ops.frames_to_nv12(y, standard=colour[0], full_range=colour[1])
        if output == "i420":
            return ops.frames_to_i420(y, standard=colour[0], full_range=colour[1])
        if output == "rgb32":
            return ops.frames_to_rgb32(y, channel_order=channel_order)
        return y if output == "f32" else ops.frames_to_u8(y, channel_order=channel_order)

    def forward(self, x_s, x_t, swap_type=None, noises_s=None, noises_t=None):
        """-> (x_s_recon, x_t_recon, fi_s, fe_s, fp_s, fi_t, fe_t, fp_t, emotion_pred_s, emotion_pred_t).

        ``swap_type`` / ``noises_*`` are optional hooks for reproducible tests; by default the swap is
        drawn from the host RNG exactly as model.py:98 does and noise is drawn on the device."""
        if self.group_encoders:
            enc = self.__dict__.get("_enc_group")
            if enc is None or enc.trunks != [self.Ei, self.Ee, self.Ep]:
                enc = self.__dict__["_enc_group"] = GroupedTrunks([self.Ei, self.Ee, self.Ep], images=2)
            fi_s, fe_s, fp_s, fi_t, fe_t, fp_t = enc(x_s, x_t).split(2048, dim=1)
        else:
            fi_s, fe_s, fp_s = self.Ei(x_s), self.Ee(x_s), self.Ep(x_s)
            fi_t, fe_t, fp_t = self.Ei(x_t), self.Ee(x_t), self.Ep(x_t)
        self._log_feature_stats(fi_s, "Identity features")
        self._log_feature_stats(fe_s, "Emotion features")
        self._log_feature_stats(fp_s, "Pose features")
        if swap_type is None:
            swap_type = torch.randint(0, 3, (1,)).item()
        if swap_type == 0:
            fi_s, fi_t = fi_t, fi_s
        elif swap_type == 1:
            fe_s, fe_t = fe_t, fe_s
        else:
            fp_s, fp_t = fp_t, fp_s
        gin_s, gin_t = self._prepare_generator_input(fi_s, fe_s, fp_s), self._prepare_generator_input(fi_t, fe_t, fp_t)
        if self.pair_decoder and hasattr(self.Gd, "forward_pair"):
            # model.py:107-108's two decoder calls as one pass over both batches (decoder.StyleGenerator.forward_pair)
            x_s_recon, x_t_recon = self.Gd.forward_pair(gin_s, gin_t, noises_s, noises_t)
        else:
            x_s_recon = self.Gd(gin_s, noises_s)
            x_t_recon = self.Gd(gin_t, noises_t)
        return (x_s_recon, x_t_recon, fi_s, fe_s, fp_s, fi_t, fe_t, fp_t, self._emotion(fe_s), self._emotion(fe_t))
