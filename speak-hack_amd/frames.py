"""The video-frame edge of the inference path: uint8 frames as a video decoder / writer holds them on the device, in and out of the
network -- packed RGB (csrc/frame_io.hip), NV12 (csrc/frame_nv12.hip), and packed RGB through a similarity transform per frame
(csrc/frame_sim.hip: aligned crops; csrc/frame_blend.hip: their paste with a face matte and a colour match; csrc/frame_sim_nv12.hip:
all of that on NV12 surfaces; csrc/frame_table.hip: on frames in buffers and of sizes of their own; csrc/frame_table_nv12.hip: on
NV12 surfaces in planes, of pitches and of sizes of their own; csrc/frame_sim_rgb32.hip, csrc/frame_table_rgb32.hip: on RGB32
frames, four bytes per pixel; csrc/frame_rgb32.hip: RGB32 frames through crop boxes, the axis-aligned edge), whose rows
csrc/landmark_sim.hip fits to landmarks and smooths; csrc/causal_filter.hip: the causal filters of a live feed, their state on
the device).  ``ops`` re-exports the
launchers (``ops.frames_from_u8`` ...), which is the documented API; ``PIXEL_FORMATS`` is what ``IRFD.reenact_video`` walks its one loop with."""
from __future__ import annotations

import ctypes as C
import functools

import torch

from . import _lib as L


# ---- what every launcher of the edge checks, written once (``what``: the caller's prefix, so each message names its function) ----
def _channel_swap(channel_order) -> int:
    if channel_order not in ("rgb", "bgr"):
        raise ValueError(f"channel_order must be 'rgb' or 'bgr', got {channel_order!r}")
    return 1 if channel_order == "bgr" else 0


def _out_size(size, what):
    Hout, Wout = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if Hout < 1 or Wout < 1:
        raise ValueError(f"{what}: size must be >= 1, got {size}")
    return Hout, Wout


def _triple(v, name):
    v = [float(v)] * 3 if isinstance(v, (int, float)) else [float(a) for a in v]
    if len(v) != 3:
        raise ValueError(f"{name} must be a number or three numbers")
    return v


def _affine(mean, std, what):                                             # (x / 255 - mean) / std per channel as scale * x + shift
    mean, std = _triple(mean, "mean"), _triple(std, "std")
    if any(s == 0 for s in std):
        raise ValueError(f"{what}: std must be non-zero")
    return [1.0 / (255.0 * s) for s in std], [-m / s for m, s in zip(mean, std)]


def check_feather(feather, what) -> float:
    feather = float(feather)
    if not (0.0 <= feather < float("inf")):
        raise ValueError(f"{what}: feather must be a finite number >= 0, got {feather}")
    return feather


def _check_chw(x, what):
    if x.dim() != 4 or x.size(1) != 3 or x.size(0) < 1:
        raise ValueError(f"{what}: x must be [N,3,H,W], got {tuple(x.shape)}")


def _origins(origins, device, what):
    """``parse_boxes``' origins as a launcher passes them: -> ``(y0, x0, None)``, or ``(0, 0, int32 [N,2] on device)``, uploaded if need be"""
    if isinstance(origins, tuple):
        return (*origins, None)
    if origins.device != device:
        if origins.is_cuda:
            raise L.SpkError(f"{what}: box origins on {origins.device}, frames on {device}")
        origins = origins.to(device)
    return 0, 0, origins


def _ptr(t):
    return None if t is None else t.data_ptr()


def _table_args(tables):                                                  # the eight table arguments of an entry point
    fy, cy, wy, fx, cx, wx = tables
    return [fy.data_ptr(), cy.data_ptr(), wy.data_ptr(), wy.size(1), fx.data_ptr(), cx.data_ptr(), wx.data_ptr(), wx.size(1)]


# ---- the host-built tables -----------------------------------------------------------------------------------------------------
def _resize_table(n_in, n_out, dtype):
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_tables: sizes must be >= 1, got {n_in} -> {n_out}")
    lib = L.lib()
    taps = lib.spk_resize_table_taps(n_in, n_out)
    if taps < 1:
        raise L.SpkError(f"spk_resize_table_taps failed ({taps}): {lib.spk_last_error().decode()}")
    first, count = torch.empty(n_out, dtype=torch.int32), torch.empty(n_out, dtype=torch.int32)
    w = torch.empty((n_out, taps), dtype=dtype)
    w64, w32 = (w.data_ptr(), None) if dtype == torch.float64 else (None, w.data_ptr())
    L.check(lib.spk_resize_table(n_in, n_out, taps, first.data_ptr(), count.data_ptr(), w64, w32), "spk_resize_table")
    return first, count, w


def resize_tables(n_in, n_out):
    """One axis of the separable triangle filter of ``F.interpolate(mode="bilinear", align_corners=False, antialias=True)``
    for ``n_in -> n_out`` samples, built in fp64 on the host (``spk_resize_table``): output ``o`` is
    ``sum_j w[o, j] * x[first[o] + j]`` over ``j < count[o]``.  -> CPU tensors ``first`` int32 [n_out], ``count`` int32 [n_out],
    ``w`` float64 [n_out, taps], zero padded to the widest window."""
    return _resize_table(n_in, n_out, torch.float64)


def resize_tables_f32(n_in, n_out):
    """The same table as the kernel reads it: fp32 weights, every row summing to exactly 1."""
    return _resize_table(n_in, n_out, torch.float32)


def feather_tables(n, feather):
    """The 1-D edge ramp of a pasted box (``spk_feather_table``, built in fp64 on the host, rounded to fp32):
    ``a[i] = min(1, (min(i, n - 1 - i) + 1) / (feather + 1))``; ``feather >= 0`` is a real number, 0 gives all ones.  A pasted
    pixel ``(y, x)`` is blended with weight ``a_y[y] * a_x[x]``.  -> CPU float32 tensor [n]."""
    n, feather = int(n), float(feather)
    if n < 1:
        raise ValueError(f"feather_tables: n must be >= 1, got {n}")
    feather = check_feather(feather, "feather_tables")
    a = torch.empty(n, dtype=torch.float32)
    L.check(L.lib().spk_feather_table(n, feather, a.data_ptr()), "spk_feather_table")
    return a


@functools.lru_cache(maxsize=32)
def _device_tables(device, Hin, Win, Hout, Wout, feather=None):
    """Device copies, built once per key, of the six resize tables ``Hin x Win -> Hout x Wout`` or (``feather``) the two ramps of a box."""
    if feather is not None:
        return feather_tables(Hout, feather).to(device), feather_tables(Wout, feather).to(device)
    return tuple(a.to(device) for a in resize_tables_f32(Hin, Hout) + resize_tables_f32(Win, Wout))


def _paste_tables(Hs, Ws, h, w, feather, device):                         # -> (the eight table arguments, a_y, a_x: None without a feather)
    ay, ax = _device_tables(device, 0, 0, h, w, feather) if feather > 0 else (None, None)
    return _table_args(_device_tables(device, Hs, Ws, h, w)), _ptr(ay), _ptr(ax)


def parse_boxes(box, N, H, W, what="box", inside=True):
    """The three forms a launcher takes a box in, for ``N`` frames of ``H`` x ``W`` pixels, checked on the host:
    ``(y0, x0, h, w)``, one box for all frames; a host sequence or CPU integer tensor ``[N,4]`` of such rows, one per frame,
    whose ``h, w`` are all equal (a call has one filter table); ``(boxes_yx, h, w)`` with a DEVICE int32 tensor ``[N,2]`` of
    origins, which is not read here (the kernels clamp / skip).  Host boxes that leave the frame raise ``ValueError``.
    ``inside``: the device form's ``h x w`` must fit the frame too (the input kernel clamps origins; the paste kernel skips).
    -> ``(origins, h, w)``: ``origins`` is ``(y0, x0)``, a CPU int32 tensor [N,2] still to be uploaded, or the device tensor."""
    def in_frame(y0, x0, h, w):
        if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
            raise ValueError(f"{what}: box {(y0, x0, h, w)} leaves the {H} x {W} frame")

    if isinstance(box, (tuple, list)) and len(box) == 3 and isinstance(box[0], torch.Tensor):
        yx, h, w = box[0], int(box[1]), int(box[2])
        if yx.dtype != torch.int32 or tuple(yx.shape) != (N, 2):
            raise ValueError(f"{what}: box origins must be an int32 tensor [{N},2], got {yx.dtype} {tuple(yx.shape)}")
        if h < 1 or w < 1 or (inside and (h > H or w > W)):
            raise ValueError(f"{what}: a {h} x {w} box does not fit the {H} x {W} frame")
        if yx.is_cuda and not yx.is_contiguous():
            yx = yx.contiguous()
        return yx, h, w
    if isinstance(box, torch.Tensor):
        if box.is_cuda or box.is_floating_point() or box.dim() != 2:
            raise ValueError(f"{what}: a tensor of boxes must be a CPU integer tensor [N,4] (device origins go as (boxes_yx, h, w))")
        box = box.tolist()
    box = list(box)
    if len(box) == 4 and not isinstance(box[0], (tuple, list)):
        y0, x0, h, w = (int(v) for v in box)
        in_frame(y0, x0, h, w)
        return (y0, x0), h, w
    rows = [tuple(int(v) for v in r) for r in box]
    if len(rows) != N or any(len(r) != 4 for r in rows):
        raise ValueError(f"{what}: per-frame boxes must be [{N},4] rows of (y0, x0, h, w), got {len(rows)} rows")
    h, w = rows[0][2], rows[0][3]
    if any((r[2], r[3]) != (h, w) for r in rows):
        raise ValueError(f"{what}: the boxes of one call must have one size (a call has one filter table per axis), "
                         f"got {sorted(set((r[2], r[3]) for r in rows))}")
    for r in rows:
        in_frame(*r)
    return torch.tensor([r[:2] for r in rows], dtype=torch.int32), h, w


# ---- packed RGB: uint8 HWC frames in and out (csrc/frame_io.hip) ----------------------------------------------------------------
def packed_pixels(frames_u8):
    """uint8 [N,H,W,3] with packed pixels and rows / frames that do not overlap: what the kernels address by byte strides.  A
    ``FrameTable`` has packed pixels by construction: its frames must not share bytes (``SpkError`` names the two that do)."""
    if isinstance(frames_u8, FrameTable):
        frames_u8.check_written()
        return True
    N, H, W, _ = frames_u8.shape
    return frames_u8.stride(3) == 1 and frames_u8.stride(2) == 3 and frames_u8.stride(1) >= 3 * W and \
        (N == 1 or frames_u8.stride(0) >= (H - 1) * frames_u8.stride(1) + 3 * W)


class _Packed:
    """The frames of a call as packed uint8 ``[N,H,W,3]`` (csrc/frame_io.hip, csrc/frame_sim.hip, csrc/frame_blend.hip): how they
    are checked and opened, the argument runs their entry points take for frames that are read and for frames that are written,
    their colour arguments and their entry points.  ``_Surfaces`` says the same of NV12; the launchers are written over either."""
    way_in, paste, sums, match = "spk_frames_u8_to_f32_sim", "spk_frames_paste_u8_sim", "spk_paste_colour_sums_sim", "spk_paste_colour_match_sim"

    def shaped(self, frames, N, what):                                    # N=None: any number, one frame may come as [H,W,3]; -> (frames, N, H, W)
        if N is None and frames.dim() == 3:
            frames = frames.unsqueeze(0)
        if frames.dim() != 4 or frames.size(3) != 3 or (frames.size(0) < 1 if N is None else frames.size(0) != N):
            raise ValueError(f"{what}: frames must be [{'N' if N is None else N},H,W,3], got {tuple(frames.shape)}")
        return (frames, *frames.shape[:3])

    def on_device(self, frames, device=None):                             # device: where x is (a strided launch is not asked)
        if not frames.is_cuda or frames.dtype != torch.uint8:
            raise L.SpkError(f"frames: expected a uint8 HIP tensor, got {frames.dtype} on {frames.device} (no CPU path)")

    def read(self, frames, what, disjoint=False):
        """Frames that are read, in place through their strides or made contiguous (``disjoint``: also where frames overlap):
        -> ``(the tensor to hold until the launch is queued, its pointer and two strides)``"""
        self.on_device(frames)
        N, _, W, _ = frames.shape
        if not (packed_pixels(frames) if disjoint else frames.stride(3) == 1 and frames.stride(2) == 3 and frames.stride(1) >= 3 * W and
                (N == 1 or frames.stride(0) >= 0)):
            frames = frames.contiguous()
        return frames, (frames.data_ptr(), frames.stride(0) if N > 1 else 0, frames.stride(1))

    def target(self, frames, out, N, H, W, device, what):
        """Frames that are written: ``out`` checked, or a packed clone of ``frames``.  -> ``(the result, its pointer and two strides,
        fill)``; ``fill()`` gives an ``out`` that is not ``frames`` its copy of them, once nothing can be refused any more."""
        copy = out is not None and out is not frames and out.data_ptr() != frames.data_ptr()
        if out is None:
            out = frames.clone(memory_format=torch.contiguous_format)
        elif not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != tuple(frames.shape):
            raise L.SpkError(f"out: expected a uint8 HIP tensor {tuple(frames.shape)}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        if not packed_pixels(out):
            raise L.SpkError(f"out: pixels must be packed and rows / frames must not overlap, got strides {out.stride()}")
        return out, (out.data_ptr(), out.stride(0) if N > 1 else 0, out.stride(1)), (lambda: out.copy_(frames)) if copy else (lambda: None)

    def standard(self):                                                   # what the way in takes behind the channel swap
        return ()

    def quantised(self, value_range, channel_order="rgb"):                # -> (the colour arguments of the way out, lo, k), in its check order
        return ((_channel_swap(channel_order),), *quant_range(value_range))

    def blend(self, matte_args, colour):                                  # -> (the paste's entry point, its arguments behind k)
        if matte_args[0] is None and colour is None:
            return self.paste, ()
        return self.paste + "_blend", (*matte_args, _ptr(colour))

    def size(self, H, W):                                                # the size arguments of an entry point: one size per launch
        return (H, W)


_PACKED = _Packed()


# ---- a frame table: every frame its own buffer and size (csrc/frame_table.hip; the definitions are in include/spk.h) ------------
class _DeviceTable:
    """What the tables of this file share once their host copy ``_host`` is filled in: the host check, the one lazy upload, the
    count, and the check that the table's frames may be written"""

    def _checked(self, check, device):
        """``check``: the entry point that judges a host table ``(table, N, written)``; ``device``: where the tensors are, None when
        every entry is absent"""
        self._check = check
        L.check(getattr(L.lib(), check)(C.addressof(self._host), self.N, 0), check)
        self._written, self._dev = False, None
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())

    @property
    def dev(self):
        """The device table, uploaded when a launcher first asks for it: every host check of a call comes before the copy"""
        if self._dev is None:
            self._dev = torch.empty(C.sizeof(self._host), dtype=torch.uint8, device=self.device)
            self._dev.copy_(torch.frombuffer(self._host, dtype=torch.uint8))
        return self._dev

    def __len__(self):
        return self.N

    def check_written(self):
        """The table's frames are about to be written: no two of them (of a surface: no two planes) may share bytes -- the host check
        with ``written`` -- else ``SpkError``"""
        if not self._written:
            L.check(getattr(L.lib(), self._check)(C.addressof(self._host), self.N, 1), self._check)
            self._written = True


class FrameTable(_DeviceTable):
    """``N`` packed uint8 frames that share neither an allocation nor a size, as the aligned launchers address them: a device table
    of ``spk_frame_ref`` entries ``(data, row_stride, H, W)``.  ``frames``: a sequence of device uint8 tensors ``[H_n,W_n,3]`` on one
    device, pixels packed (``stride(2) == 1``, ``stride(1) == 3``) and ``stride(0) >= 3 W_n`` -- a region-of-interest view of a wider
    surface is fine -- with ``None`` for a frame that is ABSENT (an all-zero entry: the launchers treat it like an invalid
    transform); or one ``[N,H,W,3]`` tensor, which gives views of its frames.  Wrong types, shapes or strides raise ``ValueError``
    before a device is touched; CPU tensors raise ``SpkError`` (no CPU path).  The host table is checked
    (``spk_frame_table_check``) here and uploaded ONCE, one host -> device copy of ``24 N`` bytes on the current stream, when a launcher
    first uses the table (so a call that is refused on the host has copied nothing); whether the frames
    may be written is decided where the table is used (``check_written``: the paste).  The table HOLDS REFERENCES to the tensors, so
    the addresses in it stay the tensors' for as long as it lives.

    ``dev``: the device table (uint8 ``[24 N]``); ``sizes``: ``(H, W)`` per frame (``(0, 0)``: absent); ``frames``: the tensors."""

    def __init__(self, frames):
        what = "FrameTable"
        if isinstance(frames, torch.Tensor):
            if frames.dim() != 4 or frames.size(0) < 1:
                raise ValueError(f"{what}: a tensor of frames must be [N,H,W,3], got {tuple(frames.shape)}")
            frames = list(frames.unbind(0))
        else:
            try:
                frames = list(frames)
            except TypeError:
                raise ValueError(f"{what}: frames must be a sequence of uint8 tensors [H,W,3] or a tensor [N,H,W,3], got "
                                 f"{type(frames).__name__}") from None
        if not frames:
            raise ValueError(f"{what}: a table needs at least one frame")
        for n, f in enumerate(frames):
            if f is None:
                continue
            if not isinstance(f, torch.Tensor):
                raise ValueError(f"{what}: frames[{n}] must be a uint8 tensor [H,W,3] or None, got {type(f).__name__}")
            if f.dtype != torch.uint8 or f.dim() != 3 or f.size(2) != 3 or f.size(0) < 1 or f.size(1) < 1:
                raise ValueError(f"{what}: frames[{n}] must be a uint8 tensor [H,W,3] with H, W >= 1, got {f.dtype} {tuple(f.shape)}")
            if f.stride(2) != 1 or f.stride(1) != 3 or f.stride(0) < 3 * f.size(1):
                raise ValueError(f"{what}: frames[{n}]: pixels must be packed and rows must not overlap (strides (>= {3 * f.size(1)}, 3, 1)), "
                                 f"got {f.stride()}")
        there = [f for f in frames if f is not None]
        if any(not f.is_cuda for f in there):
            raise L.SpkError(f"{what}: expected uint8 HIP tensors, got a frame on the CPU (no CPU path)")
        if any(f.device != there[0].device for f in there):
            raise L.SpkError(f"{what}: the frames must be on one device, got {sorted({str(f.device) for f in there})}")
        self.frames, self.N = frames, len(frames)
        self.sizes = [(0, 0) if f is None else (f.size(0), f.size(1)) for f in frames]
        self._host = (L.FrameRef * self.N)()
        for e, f in zip(self._host, frames):
            if f is not None:
                e.data, e.row_stride, e.H, e.W = f.data_ptr(), f.stride(0), f.size(0), f.size(1)
        self._checked("spk_frame_table_check", there[0].device if there else None)


class _Tabled:
    """``_Packed`` for a ``FrameTable``: the frames of a call as entries of a device table (csrc/frame_table.hip).  The size of a
    frame is its entry's, so an entry point takes none; the frames are addressed where they are, never copied."""
    noun = "frame table"
    way_in, paste = "spk_frames_u8_to_f32_sim_table", "spk_frames_paste_u8_sim_table"
    sums, match = "spk_paste_colour_sums_sim_table", "spk_paste_colour_match_sim_table"

    def shaped(self, table, N, what):                                     # -> (table, N, None, None): a table has no one size
        if N is not None and table.N != N:
            raise ValueError(f"{what}: {N} generated frames, a table of {table.N} frames")
        return table, table.N, None, None

    def on_device(self, table, device=None):                              # a table is on a device by construction: on x's?
        if device is not None and table.device != device:
            raise L.SpkError(f"frames: the {self.noun} on {table.device}, x on {device}")

    def read(self, table, what, disjoint=False):
        return table.dev, (table.dev.data_ptr(),)

    def target(self, table, out, N, H, W, device, what):
        if out is not None and out is not table:
            raise L.SpkError(f"{what}: a {self.noun} is pasted in place: out must be None or the table itself")
        table.check_written()                                             # (its device is x's: ``on_device`` saw to it)
        return table, (table.dev.data_ptr(),), lambda: None

    def size(self, H, W):
        return ()

    def standard(self):
        return ()

    def quantised(self, value_range, channel_order="rgb"):
        return _PACKED.quantised(value_range, channel_order)

    def blend(self, matte_args, colour):                                  # one entry point, with or without matte and colour rows
        return self.paste, (*matte_args, _ptr(colour))


_TABLED = _Tabled()


def clone_frames(frames_u8):
    """A packed copy of the frames to paste into: one clone of a tensor; of a ``FrameTable`` a new table over one clone per frame
    (a table of its own: its host check and, at its first launch, its upload come on top of the clones)"""
    if isinstance(frames_u8, FrameTable):
        return FrameTable([None if f is None else f.clone(memory_format=torch.contiguous_format) for f in frames_u8.frames])
    return frames_u8.clone(memory_format=torch.contiguous_format)


def _u8_format(frames_u8):                                                # a tensor takes exactly the path it always took
    return _TABLED if isinstance(frames_u8, FrameTable) else _PACKED


def frames_from_u8(frames_u8, size, *, crop=None, channel_order="rgb", mean=0.5, std=0.5):
    """uint8 HWC video frames -> the network's input, one launch (``spk_frames_u8_to_f32``): crop, antialiased bilinear resize
    to ``size`` x ``size`` (a number, or ``(H, W)``), ``(x / 255 - mean) / std`` per channel and HWC -> CHW -- ``transforms.Resize``
    + ``ToTensor`` + ``Normalize`` of inference.py:29-33 with the ``cv2.cvtColor`` of :53 (``channel_order="bgr"``: the frames are
    BGR, the result is RGB).  ``frames_u8``: uint8 [N,H,W,3] (or [H,W,3]) on the device, pixels packed (any row / frame stride:
    slices of a larger frame are read in place); ``crop=(y0, x0, h, w)``: one box for all frames; a host sequence or CPU integer
    tensor ``[N,4]``: a box per frame, all of one size (``ValueError`` otherwise: a call has one filter table;
    ``frames_from_u8_aligned`` takes a crop of any size and angle per frame), checked on the host and uploaded once; ``(boxes_yx, h, w)`` with a device int32 ``[N,2]`` tensor: origins a tracker left on the device,
    not read on the host -- the kernel clamps each so that the box stays inside the frame (``spk_frames_u8_to_f32_boxes``).
    -> float32 [N,3,size,size]."""
    frames_u8, N, H, W = _PACKED.shaped(frames_u8, None, "frames_from_u8")
    Hout, Wout = _out_size(size, "frames_from_u8")
    swap = _channel_swap(channel_order)
    scale, shift = _affine(mean, std, "frames_from_u8")
    origins = None
    if crop is not None:
        origins, h, w = parse_boxes(crop, N, H, W, "frames_from_u8: crop")
        if isinstance(origins, tuple):                                # one host box: a slice, read in place through its strides
            (y0, x0), origins = origins, None
            frames_u8 = frames_u8[:, y0:y0 + h, x0:x0 + w]
    frames_u8, where = _PACKED.read(frames_u8, "frames_from_u8")
    _, Hin, Win, _ = frames_u8.shape
    out = torch.empty((N, 3, Hout, Wout), device=frames_u8.device, dtype=torch.float32)
    entry, src = "spk_frames_u8_to_f32", (*where, N, Hin, Win)
    if origins is not None:                                               # the box is h x w of the frame, else the (sliced) frame itself
        entry, src = entry + "_boxes", (*src, _origins(origins, frames_u8.device, "frames_from_u8")[2].data_ptr(), h, w)
        Hin, Win = h, w
    L.check(getattr(L.lib(), entry)(*src, swap, *_table_args(_device_tables(frames_u8.device, Hin, Win, Hout, Wout)), out.data_ptr(), Hout, Wout,
                                    *scale, *shift, L.stream_ptr()), entry)
    return out


def quant_range(value_range):
    """``(lo, k)`` of ``q = rint(clamp((x - lo) * k, 0, 255))`` for frames in ``value_range = (lo, hi)``."""
    lo, hi = float(value_range[0]), float(value_range[1])
    if not hi > lo:
        raise ValueError(f"value_range must be increasing, got {tuple(value_range)}")
    return lo, 255.0 / (hi - lo)


def frames_to_u8(x, *, value_range=(-1, 1), channel_order="rgb", out=None):
    """Network frames -> uint8 HWC for a video writer, one launch (``spk_frames_f32_to_u8``): float32 [N,3,H,W] in
    ``value_range`` (the decoder's (-1, 1), or (0, 1)) -> uint8 [N,H,W,3], ``channel_order="bgr"`` for ``cv2.VideoWriter``;
    bit for bit ``((x - lo) * (255 / (hi - lo))).clamp(0, 255).round().to(torch.uint8)``, ties to even; NaN -> 0.  The
    reference's ``save_video`` (inference.py:78-86) multiplies by 255 and casts without offset or clamp, which wraps around on a
    frame in (-1, 1); that is deliberately not reproduced.  ``out``: a uint8 tensor [N,H,W,3] to write (contiguous, any byte
    offset)."""
    _check_chw(x, "frames_to_u8")
    swap = _channel_swap(channel_order)
    lo, k = quant_range(value_range)
    N, _, H, W = x.shape
    xp = L.dptr(x, "x")
    if out is None:
        out = torch.empty((N, H, W, 3), device=x.device, dtype=torch.uint8)
    elif not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != (N, H, W, 3) or not out.is_contiguous():
        raise L.SpkError(f"out: expected a contiguous uint8 HIP tensor {(N, H, W, 3)}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    L.check(L.lib().spk_frames_f32_to_u8(xp, out.data_ptr(), N, H, W, swap, lo, k, L.stream_ptr()), "spk_frames_f32_to_u8")
    return out


def frames_paste_u8(x, frames_u8, box, *, feather=0, value_range=(-1, 1), channel_order="rgb", out=None):
    """Generated frames back into the video they were cropped from, one launch (``spk_frames_paste_u8``): float32 [N,3,Hs,Ws]
    in ``value_range`` is resized to the box size ``h x w`` (antialiased bilinear: shrinking and enlarging), quantised as
    ``frames_to_u8`` does and blended over the pixels of ``frames_u8`` (uint8 [N,H,W,3] on the device, pixels packed, any row /
    frame stride) inside the box: ``rint(b + m (q - b))`` with ``m = a_y[y] a_x[x]`` of ``feather_tables`` (``feather=0``: the box
    replaces the background).  ``box``: ``(y0, x0, h, w)``; a host sequence / CPU integer tensor ``[N,4]`` of one size, checked
    on the host and uploaded once; or ``(boxes_yx, h, w)`` with a device int32 ``[N,2]`` tensor, not read on the host -- box
    pixels that fall outside the frame are skipped.  ``channel_order="bgr"``: the frames are BGR, ``x`` is RGB.  ``out=None``:
    the result is a clone of ``frames_u8``; ``out=frames_u8``: pasted in place through its strides; another ``out`` first
    receives a copy of ``frames_u8``.  -> uint8 [N,H,W,3]."""
    what = "frames_paste_u8"
    _check_chw(x, what)
    N, _, Hs, Ws = x.shape
    frames_u8, _, H, W = _PACKED.shaped(frames_u8, N, what)
    (swap,), lo, k = _PACKED.quantised(value_range, channel_order)
    feather = check_feather(feather, what)
    origins, h, w = parse_boxes(box, N, H, W, f"{what}: box", inside=False)
    xp = L.dptr(x, "x")
    _PACKED.on_device(frames_u8)
    out, where, fill = _PACKED.target(frames_u8, out, N, H, W, x.device, what)
    y0, x0, boxes = _origins(origins, x.device, what)
    fill()
    tables, ay, ax = _paste_tables(Hs, Ws, h, w, feather, x.device)
    L.check(L.lib().spk_frames_paste_u8(xp, N, Hs, Ws, *where, H, W, h, w, y0, x0, _ptr(boxes), swap, *tables, ay, ax, lo, k, L.stream_ptr()),
            "spk_frames_paste_u8")
    return out


# ---- aligned crops: a similarity transform per frame (csrc/frame_sim.hip; the definitions are in include/spk.h) ------------------
SIM_SCALE = (1.0 / 16.0, 16.0)                                            # the valid range of s = sqrt(a^2 + c^2), ends included


def similarity_rows(centre_yx, side, angle=0.0, size=256):
    """Rows ``(a, c, tx, ty)`` of the similarity transform that maps the ``size`` x ``size`` network image onto the square of
    ``side`` frame pixels centred at ``centre_yx = (y, x)`` and rotated by ``angle`` radians (``x = a u - c v + tx``,
    ``y = c u + a v + ty``; a positive angle turns the network's u axis towards the frame's y axis).  ``centre_yx``: one pair or
    ``[N,2]``; ``side`` and ``angle``: a number or ``N`` numbers; ``size``: a number, or ``(H, W)`` -- then ``side`` spans the
    width ``W`` and the centre of the ``H x W`` image lands on ``centre_yx``.  Host only, computed in fp64.
    -> CPU float32 tensor ``[N,4]``; ``angle=0`` and ``centre`` at the middle of a box ``(y0, x0, h, h)`` gives that box."""
    Hout, Wout = _out_size(size, "similarity_rows")
    centre = torch.as_tensor(centre_yx, dtype=torch.float64).reshape(-1, 2)
    side = torch.as_tensor(side, dtype=torch.float64).reshape(-1)
    angle = torch.as_tensor(angle, dtype=torch.float64).reshape(-1)
    N = max(centre.size(0), side.numel(), angle.numel())
    if any(n not in (1, N) for n in (centre.size(0), side.numel(), angle.numel())):
        raise ValueError(f"similarity_rows: centre_yx, side and angle must have one length, got {centre.size(0)}, {side.numel()}, {angle.numel()}")
    s = side / Wout
    a, c = s * torch.cos(angle), s * torch.sin(angle)
    u0, v0 = Wout / 2.0, Hout / 2.0
    rows = torch.stack([a.expand(N), c.expand(N), (centre[:, 1] - (a * u0 - c * v0)).expand(N), (centre[:, 0] - (c * u0 + a * v0)).expand(N)], 1)
    return rows.float()


def parse_sim(sim, N, what="sim"):
    """The two forms a launcher takes transforms in, for ``N`` frames: a DEVICE float32 tensor ``[N,4]``, which is not read here
    (the kernels follow the invalid-row rule of include/spk.h); or a host sequence / CPU tensor ``[N,4]``, rounded to fp32 and
    checked: every number finite and ``1/16 <= s <= 16``, else ``ValueError``.  -> float32 ``[N,4]``, contiguous, still where it was."""
    if isinstance(sim, torch.Tensor) and sim.is_cuda:
        if sim.dtype != torch.float32 or tuple(sim.shape) != (N, 4):
            raise ValueError(f"{what}: device transforms must be a float32 tensor [{N},4], got {sim.dtype} {tuple(sim.shape)}")
        return sim.contiguous()
    try:
        rows = torch.as_tensor(sim).to(torch.float64).to(torch.float32)
    except (ValueError, TypeError) as e:
        raise ValueError(f"{what}: transforms must be [{N},4] rows of (a, c, tx, ty): {e}") from None
    if tuple(rows.shape) != (N, 4):
        raise ValueError(f"{what}: transforms must be [{N},4] rows of (a, c, tx, ty), got {tuple(rows.shape)}")
    r64 = rows.double()
    s = (r64[:, 0] ** 2 + r64[:, 1] ** 2).sqrt()
    bad = ~(torch.isfinite(r64).all(1) & (s >= SIM_SCALE[0]) & (s <= SIM_SCALE[1]))
    if bool(bad.any()):
        n = int(bad.nonzero()[0])
        raise ValueError(f"{what}: row {n} = {rows[n].tolist()} is not a valid transform (finite numbers, 1/16 <= sqrt(a^2 + c^2) <= 16)")
    return rows.contiguous()


def _sim_on(rows, device, what):                                          # host rows: uploaded once; device rows: where the frames are
    if rows.device != device:
        if rows.is_cuda:
            raise L.SpkError(f"{what}: transforms on {rows.device}, frames on {device}")
        rows = rows.to(device)
    return rows


def _from_aligned(fmt, what, frames, size, sim, channel_order, mean, std, **standard):
    """``frames_from_u8_aligned`` / ``frames_from_nv12_aligned``: the host checks in one order, then the device and the one launch"""
    frames, N, H, W = fmt.shaped(frames, None, what)
    Hout, Wout = _out_size(size, what)
    colour = (_channel_swap(channel_order), *fmt.standard(**standard))
    scale, shift = _affine(mean, std, what)
    rows = parse_sim(sim, N, f"{what}: sim")
    held, where = fmt.read(frames, what)
    rows = _sim_on(rows, held.device, what)
    out = torch.empty((N, 3, Hout, Wout), device=held.device, dtype=torch.float32)
    L.check(getattr(L.lib(), fmt.way_in)(*where, N, *fmt.size(H, W), rows.data_ptr(), *colour, out.data_ptr(), Hout, Wout, *scale, *shift, L.stream_ptr()),
            fmt.way_in)
    return out


def frames_from_u8_aligned(frames_u8, size, sim, *, channel_order="rgb", mean=0.5, std=0.5):
    """uint8 HWC video frames -> the network's input through a similarity transform PER FRAME, one launch
    (``spk_frames_u8_to_f32_sim``): the crop of frame ``n`` is the square (rectangle) ``sim[n]`` maps the ``size`` network image
    onto -- any scale and angle per frame, which ``frames_from_u8`` (one box size per call) cannot follow -- filtered with the
    triangle filter of ``interpolate(antialias=True)`` laid along the crop's own axes, weights computed in the kernel in fp64;
    then ``(x / 255 - mean) / std`` and HWC -> CHW as ``frames_from_u8``.  Pixels outside the frame take no part: an output whose
    footprint misses the frame is ``-mean / std``.  ``sim``: rows ``(a, c, tx, ty)`` (``similarity_rows``; include/spk.h): a host
    sequence / CPU tensor ``[N,4]``, checked on the host (``ValueError`` for a row that is not finite or has a scale outside
    [1/16, 16]) and uploaded once; or a device float32 ``[N,4]`` tensor a tracker left there, not read on the host -- an invalid
    row gives a frame of ``-mean / std``.  ``frames_u8`` may be a ``FrameTable``: frames of their own sizes in their own buffers, still
    one launch (``spk_frames_u8_to_f32_sim_table``), frame ``n`` bit for bit this call on frame ``n`` alone; an absent frame gives
    ``-mean / std``.  -> float32 [N,3,size,size]."""
    return _from_aligned(_u8_format(frames_u8), "frames_from_u8_aligned", frames_u8, size, sim, channel_order, mean, std)


def _check_matte(matte, N, Hs, Ws, what):
    """A matte as the blend takes it, its shape and dtype checked before a device is touched: -> ``(matte, matte_frames)``"""
    if matte is None:
        return None, 0
    if not isinstance(matte, torch.Tensor) or matte.dtype != torch.float32 or matte.dim() not in (2, 3) or \
            tuple(matte.shape[-2:]) != (Hs, Ws) or (matte.dim() == 3 and matte.size(0) != N):
        got = f"{matte.dtype} {tuple(matte.shape)}" if isinstance(matte, torch.Tensor) else type(matte).__name__
        raise ValueError(f"{what}: matte must be a float32 tensor [{Hs},{Ws}] or [{N},{Hs},{Ws}] (the generated image's size), got {got}")
    return matte, (1 if matte.dim() == 2 else N)


def _check_colour(colour, N, what):
    if colour is not None and (not isinstance(colour, torch.Tensor) or colour.dtype != torch.float32 or tuple(colour.shape) != (N, 3, 2)):
        got = f"{colour.dtype} {tuple(colour.shape)}" if isinstance(colour, torch.Tensor) else type(colour).__name__
        raise ValueError(f"{what}: colour must be a float32 tensor [{N},3,2] of rows (gain, offset), got {got}")
    return colour


def _there(t, device, name, what):                                        # a checked matte / colour tensor: where the frames are, contiguous
    if t is None:
        return None
    if not t.is_cuda or t.device != device:
        raise L.SpkError(f"{what}: {name} on {t.device}, frames on {device} (no CPU path)")
    if not t.is_contiguous():
        raise L.SpkError(f"{what}: {name}: expected a contiguous tensor, got strides {t.stride()}")
    return t


def _aligned_args(fmt, what, x, frames, sim, feather, value_range, matte=None, colour=None, **order):
    """What the aligned paste and its statistics check alike for every pixel format ``fmt``, in one order:
    -> ``(head, frames, (H, W), rows, tail, matte_args, colour)``: the arguments of an entry point before the frames, the frames as
    ``fmt`` opened them, their size, the device rows (the caller holds them until its launch is queued), the arguments after the
    rows' pointer, the two matte arguments and the colour rows."""
    _check_chw(x, what)
    N, _, Hs, Ws = x.shape
    frames, _, H, W = fmt.shaped(frames, N, what)
    colour_args, lo, k = fmt.quantised(value_range, **order)
    feather = check_feather(feather, what)
    rows = parse_sim(sim, N, f"{what}: sim")
    matte, matte_frames = _check_matte(matte, N, Hs, Ws, what)
    colour = _check_colour(colour, N, what)
    xp = L.dptr(x, "x")
    fmt.on_device(frames, x.device)
    matte, colour = _there(matte, x.device, "matte", what), _there(colour, x.device, "colour", what)
    rows = _sim_on(rows, x.device, what)
    return (xp, N, Hs, Ws), frames, (H, W), rows, (*colour_args, feather, lo, k), (_ptr(matte), matte_frames), colour


def _paste_aligned(fmt, what, x, frames, sim, feather, value_range, out, matte, colour, **order):
    head, frames, (H, W), rows, tail, matte_args, colour = _aligned_args(fmt, what, x, frames, sim, feather, value_range, matte, colour, **order)
    out, where, fill = fmt.target(frames, out, head[1], H, W, x.device, what)
    fill()
    entry, blend = fmt.blend(matte_args, colour)
    L.check(getattr(L.lib(), entry)(*head, *where, *fmt.size(H, W), rows.data_ptr(), *tail, *blend, L.stream_ptr()), entry)
    return out


def frames_paste_u8_aligned(x, frames_u8, sim, *, feather=0, value_range=(-1, 1), channel_order="rgb", out=None, matte=None, colour=None):
    """Generated frames back into the video they were cropped from through ``sim``, one launch (``spk_frames_paste_u8_sim``): the
    inverse of ``frames_from_u8_aligned``.  Every frame pixel whose centre ``sim[n]`` maps from inside the ``Hs x Ws`` image of
    float32 ``x`` [N,3,Hs,Ws] takes the antialiased bilinear value of ``x`` there, quantised as ``frames_to_u8`` does, and is
    blended over the background byte with weight ``a_u a_v``, a ramp over ``feather`` frame pixels at the crop's own edges
    (``feather=0``: the crop replaces the background); every other byte of the frames is left as it is.  ``sim``: the two forms
    of ``frames_from_u8_aligned``; a device row that is invalid leaves its frame untouched.  ``channel_order``, ``out``: as
    ``frames_paste_u8``.

    ``matte`` / ``colour`` (either one: ``spk_frames_paste_u8_sim_blend``, still one launch): ``matte`` is a device float32
    ``[Hs,Ws]`` (one for all frames: ``ellipse_matte``) or ``[N,Hs,Ws]`` tensor in the generated image's coordinates, sampled with
    the weights of ``x``, clamped to [0, 1] (NaN: 0) and multiplied into the blend weight, so only the face is pasted; ``colour``
    is a device float32 ``[N,3,2]`` tensor of rows ``(gain, offset)`` per frame and channel of ``x``, applied to the quantised
    value in front of the blend (``paste_colour_match`` makes them; a row that is not finite counts as ``(1, 0)``).  Without
    both, the call is the one it always was.  -> uint8 [N,H,W,3].

    ``frames_u8`` may be a ``FrameTable`` (``spk_frames_paste_u8_sim_table``, one launch with or without ``matte`` / ``colour``): the
    paste is then IN PLACE, into the table's own frames (``out``: None or the table), which must not share bytes; an absent frame is
    left alone; frame ``n`` gets the bytes of this call on frame ``n`` alone.  -> the table."""
    return _paste_aligned(_u8_format(frames_u8), "frames_paste_u8_aligned", x, frames_u8, sim, feather, value_range, out, matte, colour, channel_order=channel_order)


COLOUR_SUMS = 13                                                          # S0, then (Sq, Sqq, Sb, Sbb) per network channel


@functools.lru_cache(maxsize=8)
def _colour_workspace(device, N):                                         # the partial sums of N frames, kept per (device, N)
    need = L.lib().spk_paste_colour_match_workspace_bytes(N)
    if need < 0:
        raise L.SpkError(f"spk_paste_colour_match_workspace_bytes({N}) failed")
    return torch.empty(need // 8, device=device, dtype=torch.float64)


def _check_match_params(what, max_gain, min_sigma, min_weight):           # the three parameters of the row formula, as floats
    max_gain, min_sigma, min_weight = float(max_gain), float(min_sigma), float(min_weight)
    if not (1.0 <= max_gain < float("inf")):
        raise ValueError(f"{what}: max_gain must be a finite number >= 1, got {max_gain}")
    if not (0.0 <= min_sigma < float("inf")) or not (0.0 <= min_weight < float("inf")):
        raise ValueError(f"{what}: min_sigma and min_weight must be finite numbers >= 0, got {min_sigma}, {min_weight}")
    return max_gain, min_sigma, min_weight


def _stat_out(out, shape, dtype, device):                                 # what a statistics launcher writes: ``out=`` checked, or a new tensor
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != shape or out.device != device or not out.is_contiguous():
        name = str(dtype).replace("torch.", "")
        raise L.SpkError(f"out: expected a contiguous {name} HIP tensor {shape} on {device}")
    return out


def _colour_statistics(fmt, params, what, x, frames, sim, matte, feather, value_range, out, **order):
    """What the four statistics launchers share -- the checks, the background, ``out=``, the workspace and the call of the entry point
    of ``fmt``: the rows of the match with its three ``params`` (in front of the output pointer), the sums without (``None``)"""
    entry, shape, dtype = (fmt.sums, (COLOUR_SUMS,), torch.float64) if params is None else (fmt.match, (3, 2), torch.float32)
    head, frames, (H, W), rows, tail, matte_args, _ = _aligned_args(fmt, what, x, frames, sim, feather, value_range, matte, **order)
    held, where = fmt.read(frames, what, disjoint=True)
    out = _stat_out(out, (head[1], *shape), dtype, x.device)
    ws = _colour_workspace(x.device, head[1])
    L.check(getattr(L.lib(), entry)(*head, *where, *fmt.size(H, W), rows.data_ptr(), *tail, *matte_args, *(params or ()), out.data_ptr(), ws.data_ptr(),
                                    ws.numel() * 8, L.stream_ptr()), entry)
    return out


def paste_colour_match(x, frames_u8, sim, *, matte=None, feather=0, value_range=(-1, 1), channel_order="rgb", max_gain=2.0, min_sigma=1.0,
                       min_weight=16.0, out=None):
    """The colour rows ``frames_paste_u8_aligned(colour=)`` takes, two launches (``spk_paste_colour_match_sim``): per frame and
    channel the ``(gain, offset)`` that carries the mean and standard deviation of the generated face ``x`` onto those of the
    pixels of ``frames_u8`` it is about to replace, both weighted with the very blend weight ``a_u a_v Mt`` the paste will use
    (``x``, ``frames_u8``, ``sim``, ``matte``, ``feather``, ``value_range``, ``channel_order``: as ``frames_paste_u8_aligned``;
    include/spk.h has the sums).  ``frames_u8`` is only read -- call this BEFORE pasting in place.  The gain is kept within
    ``[1 / max_gain, max_gain]`` and is 1 where the generated face has a standard deviation of at most ``min_sigma`` levels; a
    frame whose weights sum to at most ``min_weight``, or whose row is invalid, gets ``(1, 0)``.  The sums are reduced in a fixed
    order without atomics: the same inputs give the same bits.  The rows come back as a tensor; to steady them over time,
    pool the SUMS (``paste_colour_sums`` + ``colour_rows_from_sums``), not the rows.  ``out``: a contiguous device float32 ``[N,3,2]``
    tensor to write.  ``frames_u8`` may be a ``FrameTable`` (``spk_paste_colour_match_sim_table``; an absent frame gets ``(1, 0)``).
    -> device float32 ``[N,3,2]``."""
    what = "paste_colour_match"
    params = _check_match_params(what, max_gain, min_sigma, min_weight)
    return _colour_statistics(_u8_format(frames_u8), params, what, x, frames_u8, sim, matte, feather, value_range, out, channel_order=channel_order)


def paste_colour_sums(x, frames_u8, sim, *, matte=None, feather=0, value_range=(-1, 1), channel_order="rgb", out=None):
    """The statistics of ``paste_colour_match`` as a result, two launches (``spk_paste_colour_sums_sim``): per frame the 13 fp64 sums
    ``S0, (Sq, Sqq, Sb, Sbb)`` x 3 network channels that its rows are made from (include/spk.h), bit for bit the sums it forms
    internally; 13 zeros for a frame whose row is invalid.  The arguments are that launcher's without the three parameters of the
    row formula, which ``colour_rows_from_sums`` takes -- with ``radius=0`` it turns these sums into exactly ``paste_colour_match``'s
    rows, with a radius it pools them over neighbouring frames first.  ``out``: a contiguous device float64 ``[N,13]`` tensor to
    write, for instance the slice ``[t0:t1]`` of a clip-long ``[T,13]`` tensor.  ``frames_u8`` may be a ``FrameTable``
    (``spk_paste_colour_sums_sim_table``; 13 zeros for an absent frame).  -> device float64 ``[N,13]``."""
    return _colour_statistics(_u8_format(frames_u8), None, "paste_colour_sums", x, frames_u8, sim, matte, feather, value_range, out, channel_order=channel_order)


def colour_rows_from_sums(sums, radius=0, sigma=None, *, start=0, stop=None, max_gain=2.0, min_sigma=1.0, min_weight=16.0, out=None):
    """Colour rows from the sums of a clip, pooled over time, one launch (``spk_colour_rows_window``): the rows of frames
    ``start ... stop - 1`` (``stop=None``: the clip's end) of ``sums``, a device float64 ``[T,13]`` tensor as ``paste_colour_sums`` /
    ``paste_colour_sums_nv12`` write it.  Frame ``t``'s 13 sums are replaced by the sums over frames ``t - radius ... t + radius``
    with weights ``exp(-d^2 / (2 sigma^2))`` (``sigma=None``: ``max(radius, 1) / 2``), in fp64, and ``paste_colour_match``'s row
    formula (``max_gain``, ``min_sigma``, ``min_weight``: its parameters) is applied to the result.  A frame takes part in a window
    when its ``S0`` exceeds ``min_weight`` and -- as a neighbour -- its sums are finite: a drop-out of up to ``radius`` frames is
    bridged from its neighbours, a window in which no frame takes part gives ``(1, 0)``.  The sums are linear, so this is the colour
    match of the face over a stretch of video, every frame weighing in with its weighted area; filtering the rows ``(g, o)``
    themselves is not (a ``(1, 0)`` got by rule drags its neighbours to the identity).  ``radius=0``: ``paste_colour_match``'s rows
    bit for bit.  A row depends on its own window only: a sub-range gives the bits of the whole clip.  ``out``: a contiguous device
    float32 ``[stop - start,3,2]`` tensor to write.  -> device float32 ``[stop - start,3,2]``."""
    what = "colour_rows_from_sums"
    radius, sigma = _check_smooth(radius, sigma, what)
    params = _check_match_params(what, max_gain, min_sigma, min_weight)
    if not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64 or sums.dim() != 2 or sums.size(1) != COLOUR_SUMS or sums.size(0) < 1:
        got = f"{sums.dtype} {tuple(sums.shape)}" if isinstance(sums, torch.Tensor) else type(sums).__name__
        raise ValueError(f"{what}: sums must be a float64 tensor [T,{COLOUR_SUMS}], got {got}")
    T = sums.size(0)
    stop = T if stop is None else stop
    if any(isinstance(v, bool) or not isinstance(v, int) for v in (start, stop)) or not 0 <= start < stop <= T:
        raise ValueError(f"{what}: start / stop must be integers with 0 <= start < stop <= {T}, got {start!r}, {stop!r}")
    if not sums.is_cuda:
        raise L.SpkError(f"{what}: sums on {sums.device} (no CPU path)")
    if not sums.is_contiguous():
        raise L.SpkError(f"{what}: sums: expected a contiguous tensor, got strides {sums.stride()}")
    out = _stat_out(out, (stop - start, 3, 2), torch.float32, sums.device)
    L.check(L.lib().spk_colour_rows_window(sums.data_ptr(), T, start, stop - start, radius, sigma, *params, out.data_ptr(), L.stream_ptr()),
            "spk_colour_rows_window")
    return out


def ellipse_matte(size_hw, centre=(0.5, 0.5), radii=(0.36, 0.46), softness=0.1, device=None):
    """A static face matte for ``frames_paste_u8_aligned(matte=)``: an ellipse in the generated image, 1 inside, falling to 0 over
    its rim.  For pixel ``(j, i)`` of an ``Hs x Ws`` image, ``rho = sqrt(((i + 0.5) / Ws - cx)^2 / rx^2 + ((j + 0.5) / Hs - cy)^2 /
    ry^2)`` and ``M = clip((1 - rho) / softness, 0, 1)``; ``centre = (cx, cy)`` and ``radii = (rx, ry)`` are fractions of the width
    and the height, ``softness > 0`` the fraction of the radius the rim takes.  Built in fp64 on the host, rounded to fp32.
    -> float32 ``[Hs,Ws]`` on ``device`` (None: the CPU)."""
    Hs, Ws = _out_size(size_hw, "ellipse_matte")
    (cx, cy), (rx, ry), softness = (float(v) for v in centre), (float(v) for v in radii), float(softness)
    if not (0.0 < softness < float("inf")):
        raise ValueError(f"ellipse_matte: softness must be a finite number > 0, got {softness}")
    if not (0.0 < rx < float("inf") and 0.0 < ry < float("inf")):
        raise ValueError(f"ellipse_matte: radii must be finite numbers > 0, got {(rx, ry)}")
    du = ((torch.arange(Ws, dtype=torch.float64) + 0.5) / Ws - cx) ** 2 / rx ** 2
    dv = ((torch.arange(Hs, dtype=torch.float64) + 0.5) / Hs - cy) ** 2 / ry ** 2
    matte = ((1.0 - (dv.view(Hs, 1) + du.view(1, Ws)).sqrt()) / softness).clamp(0.0, 1.0).float()
    return matte if device is None else matte.to(device)


# ---- landmarks to rows on the device: similarity fit and smoothing (csrc/landmark_sim.hip; the definitions are in include/spk.h) --
LANDMARKS_MAX, SMOOTH_RADIUS_MAX = 4096, 64                               # K and radius as the entry points bound them


def _check_fit(landmarks, template, weights, offset, what):
    """What the fit checks on the host, before a device is touched: -> ``(template, weights, offset)``, host forms rounded to
    float32 CPU tensors still to be uploaded, device forms as they came (not read)."""
    if not isinstance(landmarks, torch.Tensor) or landmarks.dim() != 3 or landmarks.size(2) != 2 or landmarks.size(0) < 1 or \
            not 2 <= landmarks.size(1) <= LANDMARKS_MAX:
        got = tuple(landmarks.shape) if isinstance(landmarks, torch.Tensor) else type(landmarks).__name__
        raise ValueError(f"{what}: landmarks must be a tensor [N,K,2] with 2 <= K <= {LANDMARKS_MAX}, got {got}")
    N, K, _ = landmarks.shape
    if isinstance(template, torch.Tensor) and template.is_cuda:
        if template.dtype != torch.float32 or tuple(template.shape) != (K, 2):
            raise ValueError(f"{what}: a device template must be a float32 tensor [{K},2], got {template.dtype} {tuple(template.shape)}")
    else:
        try:
            template = torch.as_tensor(template).to(torch.float64).to(torch.float32)
        except (ValueError, TypeError, RuntimeError) as e:
            raise ValueError(f"{what}: template must be [{K},2] points (u, v): {e}") from None
        if tuple(template.shape) != (K, 2):
            raise ValueError(f"{what}: template must be [{K},2] points (u, v), one per landmark, got {tuple(template.shape)}")
        if not bool(torch.isfinite(template).all()):
            raise ValueError(f"{what}: template must be finite")
        if bool((template == template[0]).all()):
            raise ValueError(f"{what}: template needs at least two distinct points (a similarity has no scale otherwise)")
    if isinstance(weights, torch.Tensor) and weights.is_cuda:
        if weights.dtype != torch.float32 or tuple(weights.shape) not in ((K,), (N, K)):
            raise ValueError(f"{what}: device weights must be a float32 tensor [{K}] or [{N},{K}], got {weights.dtype} {tuple(weights.shape)}")
    elif weights is not None:
        try:
            weights = torch.as_tensor(weights).to(torch.float64).to(torch.float32)
        except (ValueError, TypeError, RuntimeError) as e:
            raise ValueError(f"{what}: weights must be [{K}] numbers: {e}") from None
        if tuple(weights.shape) != (K,):
            raise ValueError(f"{what}: host weights must be [{K}] numbers, one per landmark, got {tuple(weights.shape)}")
    offset = float(offset)
    if not (-float("inf") < offset < float("inf")):
        raise ValueError(f"{what}: offset must be finite, got {offset}")
    return template, weights, offset


def _fit(landmarks, template, weights, offset, what):                    # checked arguments -> device float32 [N,4], one launch
    if not landmarks.is_cuda or landmarks.dtype != torch.float32:
        raise L.SpkError(f"{what}: landmarks: expected a float32 HIP tensor, got {landmarks.dtype} on {landmarks.device} (no CPU path)")
    N, K, _ = landmarks.shape
    landmarks = landmarks.contiguous()

    def there(t, name):                                                   # host forms: uploaded once; device forms: where the landmarks are
        if t.is_cuda and t.device != landmarks.device:
            raise L.SpkError(f"{what}: {name} on {t.device}, landmarks on {landmarks.device}")
        return t.to(landmarks.device).contiguous()

    template, weights = there(template, "template"), None if weights is None else there(weights, "weights")
    rows = torch.empty((N, 4), device=landmarks.device, dtype=torch.float32)
    L.check(L.lib().spk_sim_fit_landmarks(landmarks.data_ptr(), _ptr(weights), K if weights is not None and weights.dim() == 2 else 0,
                                          template.data_ptr(), N, K, offset, rows.data_ptr(), L.stream_ptr()), "spk_sim_fit_landmarks")
    return rows


def similarity_from_landmarks(landmarks, template, *, weights=None, offset=0.0):
    """Landmarks -> rows ``(a, c, tx, ty)`` where the landmarks are, one launch (``spk_sim_fit_landmarks``): per frame the weighted
    least-squares similarity without reflection that carries ``template`` onto the frame's landmarks (centred sums in fp64;
    include/spk.h has them) -- what ``frames_from_u8_aligned`` / ``frames_paste_u8_aligned`` / ``reenact_video(align=)`` take, with
    no copy to the host.  ``landmarks``: a device float32 ``[N,K,2]`` tensor of ``(x, y)`` in frame coordinates (the centre of pixel
    ``(ix, iy)`` is ``(ix + 0.5, iy + 0.5)``; ``offset`` is added to both: 0.5 for a tracker that reports pixel indices), made
    contiguous if it is not.  ``template``: the same ``K`` landmarks as ``(u, v)`` in the network image -- a host sequence / CPU
    tensor ``[K,2]``, checked (finite, at least two distinct points, else ``ValueError``) and uploaded, or a device float32 tensor,
    not read.  ``weights``: None (all 1); a host sequence / CPU tensor ``[K]``, uploaded; or a device float32 ``[K]`` (one set for
    all frames) or ``[N,K]``, e.g. a tracker's confidences.  A landmark takes part when its weight is finite and > 0 and its
    coordinates are finite; a frame with fewer than two participants, or whose participants share one template point, gives four
    NaNs -- an invalid row, which the way in answers with ``-mean / std`` and the paste by leaving the frame alone.
    -> device float32 ``[N,4]``."""
    what = "similarity_from_landmarks"
    return _fit(landmarks, *_check_fit(landmarks, template, weights, offset, what), what)


def _check_smooth(radius, sigma, what):
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= SMOOTH_RADIUS_MAX:
        raise ValueError(f"{what}: radius must be an integer in [0, {SMOOTH_RADIUS_MAX}], got {radius!r}")
    sigma = max(radius, 1) / 2.0 if sigma is None else float(sigma)
    if not (0.0 < sigma < float("inf")):
        raise ValueError(f"{what}: sigma must be a finite number > 0, got {sigma}")
    return radius, sigma


def smooth_similarity_rows(rows, radius, sigma=None):
    """Rows smoothed over time, one launch (``spk_sim_smooth``): row ``n`` becomes the mean of rows ``n - radius ... n + radius``
    with weights ``exp(-d^2 / (2 sigma^2))`` (``sigma=None``: ``max(radius, 1) / 2``), in fp64 -- the raw per-frame fits jitter by a
    fraction of a pixel, which shows as a pasted face swimming in its frame.  Averaging rows averages the maps, so the result is
    again a similarity.  Rows that are not finite (a tracker drop-out) and rows beyond the clip's ends take no part, so a gap of up
    to ``radius`` frames is BRIDGED from its neighbours; a window without a finite row gives four NaNs.  A caller who wants
    drop-outs to stay drop-outs smooths with ``radius=0`` (a copy of the finite rows) or masks afterwards.  ``rows``: a device
    float32 ``[N,4]`` tensor, or a host sequence / CPU tensor, uploaded unchecked (NaN rows are legal here).  -> a new device
    float32 ``[N,4]``."""
    what = "smooth_similarity_rows"
    radius, sigma = _check_smooth(radius, sigma, what)
    if not (isinstance(rows, torch.Tensor) and rows.is_cuda):
        try:
            rows = torch.as_tensor(rows).to(torch.float64).to(torch.float32)
        except (ValueError, TypeError, RuntimeError) as e:
            raise ValueError(f"{what}: rows must be [N,4] rows of (a, c, tx, ty): {e}") from None
    if rows.dtype != torch.float32 or rows.dim() != 2 or rows.size(1) != 4 or rows.size(0) < 1:
        raise ValueError(f"{what}: rows must be a float32 [N,4] tensor, got {rows.dtype} {tuple(rows.shape)}")
    if not rows.is_cuda:
        if not torch.cuda.is_available():
            raise L.SpkError(f"{what}: no HIP device to upload the rows to (no CPU path)")
        rows = rows.to("cuda")
    rows = rows.contiguous()
    out = torch.empty_like(rows)
    L.check(L.lib().spk_sim_smooth(rows.data_ptr(), rows.size(0), radius, sigma, out.data_ptr(), L.stream_ptr()), "spk_sim_smooth")
    return out


class LandmarkAlign:
    """``IRFD.reenact_video(align=...)`` / ``(identity_align=...)`` from landmarks: what ``similarity_from_landmarks`` takes, kept
    until the call knows its frames.  ``rows(T)`` is one fit launch, plus one ``smooth_similarity_rows(rows, smooth, sigma)`` launch
    when ``smooth > 0`` -- once per clip, so the smoothing sees every frame and the result does not depend on ``chunk``.  The host
    arguments are checked here (``ValueError``), the device ones when the rows are made.  ``template`` is in the coordinates of the
    ``size`` network image the call is made with: no rescaling to another ``size`` is offered."""

    def __init__(self, landmarks, template, *, weights=None, offset=0.0, smooth=0, sigma=None):
        what = "LandmarkAlign"
        self.landmarks = landmarks
        self.template, self.weights, self.offset = _check_fit(landmarks, template, weights, offset, what)
        self.smooth, self.sigma = _check_smooth(smooth, sigma, f"{what}: smooth")

    def rows(self, T, what="LandmarkAlign"):
        """The rows of ``T`` frames -> device float32 ``[T,4]``"""
        if self.landmarks.size(0) != T:
            raise ValueError(f"{what}: landmarks of {self.landmarks.size(0)} frames for {T} frames")
        rows = _fit(self.landmarks, self.template, self.weights, self.offset, what)
        return smooth_similarity_rows(rows, self.smooth, self.sigma) if self.smooth > 0 else rows


# ---- a matte per frame from the landmarks' contour (csrc/landmark_matte.hip; the definitions are in include/spk.h) -----------------
CONTOUR_POINTS, MATTE_SIZE_MAX = (3, 128), 4096                           # Kc and Hs, Ws as the entry point bounds them


def _check_contour(contour, K, what):                                     # -> a list of ints; K=None: the indices' range is checked later
    try:
        idx = torch.as_tensor(contour)
    except (ValueError, TypeError, RuntimeError) as e:
        raise ValueError(f"{what}: contour must be landmark indices in outline order: {e}") from None
    if idx.is_cuda or idx.dim() != 1 or idx.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8) or \
            not CONTOUR_POINTS[0] <= idx.numel() <= CONTOUR_POINTS[1]:
        raise ValueError(f"{what}: contour must be {CONTOUR_POINTS[0]} to {CONTOUR_POINTS[1]} integer landmark indices on the host, "
                         f"got {idx.dtype} {tuple(idx.shape)} on {idx.device}")
    idx = idx.tolist()
    return idx if K is None else _contour_in(idx, K, what)


def _contour_in(idx, K, what):
    if min(idx) < 0 or max(idx) >= K:
        raise ValueError(f"{what}: contour holds an index outside [0, {K}): the landmarks have {K} points per frame")
    return idx


def _check_matte_landmarks(landmarks, what):
    if not isinstance(landmarks, torch.Tensor) or landmarks.dim() != 3 or landmarks.size(2) != 2 or landmarks.size(0) < 1 or \
            not 1 <= landmarks.size(1) <= LANDMARKS_MAX:
        got = tuple(landmarks.shape) if isinstance(landmarks, torch.Tensor) else type(landmarks).__name__
        raise ValueError(f"{what}: landmarks must be a tensor [N,K,2] with 1 <= K <= {LANDMARKS_MAX}, got {got}")
    return landmarks


def _finite(v, name, what, positive=False):
    try:
        v = float(v)
    except (ValueError, TypeError):
        raise ValueError(f"{what}: {name} must be a number, got {v!r}") from None
    if not (-float("inf") < v < float("inf")) or (positive and v <= 0.0):
        raise ValueError(f"{what}: {name} must be a finite number{' > 0' if positive else ''}, got {v}")
    return v


def _check_fallback(fallback, Kc, what):                                  # host points: rounded to fp32 and checked; device points: not read
    if fallback is None:
        return None
    if isinstance(fallback, torch.Tensor) and fallback.is_cuda:
        if fallback.dtype != torch.float32 or tuple(fallback.shape) != (Kc, 2):
            raise ValueError(f"{what}: a device fallback must be a float32 tensor [{Kc},2], got {fallback.dtype} {tuple(fallback.shape)}")
        return fallback
    try:
        fallback = torch.as_tensor(fallback).to(torch.float64).to(torch.float32)
    except (ValueError, TypeError, RuntimeError) as e:
        raise ValueError(f"{what}: fallback must be [{Kc},2] points (u, v): {e}") from None
    if tuple(fallback.shape) != (Kc, 2) or not bool(torch.isfinite(fallback).all()):
        raise ValueError(f"{what}: fallback must be [{Kc},2] finite points (u, v), one per contour index, got {tuple(fallback.shape)}")
    return fallback


def _matte_size(size_hw, what):
    Hs, Ws = _out_size(size_hw, what)
    if Hs > MATTE_SIZE_MAX or Ws > MATTE_SIZE_MAX:
        raise ValueError(f"{what}: size must be <= {MATTE_SIZE_MAX}, got {size_hw}")
    return Hs, Ws


def _matte(landmarks, rows, Hs, Ws, idx, softness, grow, offset, fallback, radius, sigma, what):   # checked arguments -> [N,Hs,Ws], one launch
    if not landmarks.is_cuda or landmarks.dtype != torch.float32:
        raise L.SpkError(f"{what}: landmarks: expected a float32 HIP tensor, got {landmarks.dtype} on {landmarks.device} (no CPU path)")
    N, K, _ = landmarks.shape
    landmarks = landmarks.contiguous()
    rows = _sim_on(rows, landmarks.device, what)
    if fallback is not None:                                              # a host outline: uploaded once
        if fallback.is_cuda and fallback.device != landmarks.device:
            raise L.SpkError(f"{what}: fallback on {fallback.device}, landmarks on {landmarks.device}")
        fallback = fallback.to(landmarks.device).contiguous()
    out = torch.empty((N, Hs, Ws), device=landmarks.device, dtype=torch.float32)
    L.check(L.lib().spk_matte_from_landmarks(landmarks.data_ptr(), N, K, offset, rows.data_ptr(), (C.c_int32 * len(idx))(*idx), len(idx),
                                             _ptr(fallback), radius, sigma, softness, grow, out.data_ptr(), Hs, Ws, L.stream_ptr()),
            "spk_matte_from_landmarks")
    return out


def matte_from_landmarks(landmarks, sim, size_hw, contour, *, softness=4.0, grow=0.0, offset=0.0, fallback=None, smooth=0, sigma=None):
    """A face matte per frame for ``frames_paste_u8_aligned(matte=)`` / ``frames_paste_nv12_aligned(matte=)`` from the landmarks
    themselves, one launch (``spk_matte_from_landmarks``; include/spk.h has the definitions): the closed outline through the
    landmarks ``contour`` names (the jaw line and the brows, say, in outline order), carried through each frame's row into the
    ``size_hw`` generated image, and ``M = clip((d + grow) / softness, 0, 1)`` of the signed distance ``d`` of every pixel centre to
    it (positive inside; even-odd parity, so a concave or self-crossing outline is defined) -- a matte that follows the jaw when the
    mouth opens, where ``ellipse_matte`` is one oval for the clip.  ``landmarks``: a device float32 ``[N,K,2]`` tensor of ``(x, y)``
    in frame coordinates, ``offset`` added to both (``similarity_from_landmarks``).  ``sim``: the rows that map the GENERATED image
    into the frames, in the two forms of ``frames_paste_u8_aligned`` (host rows are checked, device rows are not read; a point
    of an invalid row or with a coordinate that is not finite takes no part).  ``contour``: 3 to 128 integer indices in ``[0, K)``, a
    host sequence.  ``softness > 0``: the ramp's width in generated pixels; ``grow``: moves the outline outwards by that many pixels
    (0: nothing outside the tracked face is pasted).  ``smooth`` / ``sigma``: every outline point is averaged over frames
    ``n - smooth ... n + smooth`` with the weights of ``smooth_similarity_rows``, points that take no part left out, so a drop-out
    is bridged; a point without any participant comes from ``fallback`` -- ``[Kc,2]`` points in generated-image coordinates, a
    host sequence (checked, uploaded once) or a device float32 tensor -- and without a fallback that frame's matte is zeros.
    -> device float32 ``[N,Hs,Ws]``."""
    what = "matte_from_landmarks"
    landmarks = _check_matte_landmarks(landmarks, what)
    Hs, Ws = _matte_size(size_hw, what)
    idx = _check_contour(contour, landmarks.size(1), what)
    softness, grow, offset = _finite(softness, "softness", what, positive=True), _finite(grow, "grow", what), _finite(offset, "offset", what)
    radius, sigma = _check_smooth(smooth, sigma, f"{what}: smooth")
    rows = parse_sim(sim, landmarks.size(0), f"{what}: sim")
    fallback = _check_fallback(fallback, len(idx), what)
    return _matte(landmarks, rows, Hs, Ws, idx, softness, grow, offset, fallback, radius, sigma, what)


class LandmarkMatte:
    """``IRFD.reenact_video(matte=...)`` from landmarks: what ``matte_from_landmarks`` takes, kept until the call knows its rows and
    the generated size ``R``.  ``landmarks=None``: the landmarks of the call's ``align=LandmarkAlign(...)`` (without one:
    ``ValueError``); ``offset`` / ``smooth`` (with its ``sigma``) ``=None``: that ``LandmarkAlign``'s when the call has one, else 0.
    ``fallback``: ``"template"`` -- the contour's points of the ``LandmarkAlign``'s template (it needs one) -- or ``[Kc,2]`` points, a
    host sequence, like the template in the coordinates of the ``size`` network image and scaled to ``R`` with it; or None.  The
    matte is made once per clip, with the rows the paste uses, so the window sees every frame and the result does not depend on
    ``chunk``.  The host arguments are checked here and in ``bind`` (``ValueError``), the device ones when the matte is made."""

    def __init__(self, contour, *, landmarks=None, softness=4.0, grow=0.0, offset=None, fallback="template", smooth=None, sigma=None):
        what = "LandmarkMatte"
        self.landmarks = None if landmarks is None else _check_matte_landmarks(landmarks, what)
        self.contour = _check_contour(contour, None if landmarks is None else landmarks.size(1), what)
        self.softness, self.grow = _finite(softness, "softness", what, positive=True), _finite(grow, "grow", what)
        self.offset = None if offset is None else _finite(offset, "offset", what)
        if smooth is None and sigma is not None:
            raise ValueError(f"{what}: sigma comes with smooth")
        self.smooth = None if smooth is None else _check_smooth(smooth, sigma, f"{what}: smooth")
        if isinstance(fallback, str):
            if fallback != "template":
                raise ValueError(f"{what}: fallback must be 'template', [{len(self.contour)},2] points or None, got {fallback!r}")
        elif isinstance(fallback, torch.Tensor) and fallback.is_cuda:
            raise ValueError(f"{what}: fallback points are a host sequence (they are scaled to the generated size before the upload)")
        else:
            fallback = _check_fallback(fallback, len(self.contour), what)
        self.fallback = fallback

    def bind(self, align, T, what="reenact_video: matte"):
        """The carrier against the call's ``align=`` and its ``T`` frames, on the host: -> ``make(aligned, size)``, which takes what
        ``Aligned.chunk(0, T, y)`` gave (the clip's rows scaled to the generated size) and the ``(H, W)`` of the network image
        -> device float32 ``[T,Hs,Ws]``, one launch."""
        la = align if isinstance(align, LandmarkAlign) else None
        landmarks = self.landmarks
        if landmarks is None:
            if la is None:
                raise ValueError(f"{what}: LandmarkMatte(landmarks=None) takes its landmarks from align=LandmarkAlign(...), and align is not one")
            landmarks = la.landmarks
        if landmarks.size(0) != T:
            raise ValueError(f"{what}: landmarks of {landmarks.size(0)} frames for {T} frames")
        idx = _contour_in(self.contour, landmarks.size(1), what)
        offset = self.offset if self.offset is not None else la.offset if la is not None else 0.0
        radius, sigma = self.smooth if self.smooth is not None else (la.smooth, la.sigma) if la is not None else _check_smooth(0, None, what)
        fallback = self.fallback
        if isinstance(fallback, str):
            if la is None or la.template.is_cuda:
                raise ValueError(f"{what}: fallback='template' needs align=LandmarkAlign(...) with a host template")
            if max(idx) >= la.template.size(0):
                raise ValueError(f"{what}: contour holds an index outside the template's {la.template.size(0)} points")
            fallback = la.template[idx]

        def make(aligned, size):
            Hs, Ws = _matte_size(aligned.size, what)
            k = torch.tensor(Ws / size[1], dtype=torch.float32)               # the template lives in the network image: scaled in fp32
            return _matte(landmarks, aligned.rows, Hs, Ws, idx, self.softness, self.grow, offset, None if fallback is None else fallback * k,
                          radius, sigma, what)
        return make


# ---- causal filters with their state on the device (csrc/causal_filter.hip; the definitions are in include/spk.h) -------------------
FILTER_DEFAULTS = dict(min_cutoff=1.0, beta=0.05, d_cutoff=1.0, hold=5)   # a face in a 30 fps feed, landmarks in frame pixels


def check_filter_params(what, group, rate, min_cutoff, beta, d_cutoff, hold):
    """The parameters of ``causal_filter`` as the entry point takes them, checked on the host: -> the six, as ints and floats"""
    if isinstance(group, bool) or not isinstance(group, int) or not 1 <= group <= 4:
        raise ValueError(f"{what}: group must be 1, 2, 3 or 4, got {group!r}")
    rate, min_cutoff, d_cutoff = (_finite(v, n, what, positive=True) for v, n in ((rate, "rate"), (min_cutoff, "min_cutoff"), (d_cutoff, "d_cutoff")))
    beta = _finite(beta, "beta", what)
    if beta < 0.0:
        raise ValueError(f"{what}: beta must be a finite number >= 0, got {beta}")
    if isinstance(hold, bool) or not isinstance(hold, int) or not 0 <= hold < 2 ** 31:
        raise ValueError(f"{what}: hold must be an integer >= 0 (frames a drop-out is bridged over), got {hold!r}")
    return group, rate, min_cutoff, beta, d_cutoff, hold


def causal_filter_state(D, group, device):
    """The empty state of ``causal_filter`` for a signal of ``D`` components in groups of ``group``: zeros, float64
    ``[D / group, 2 + 2 group]`` on ``device`` (per group ``(k, w_last, xh[group], dh[group])``; include/spk.h).  Zeroing it again
    (``state.zero_()``) forgets the past."""
    what = "causal_filter_state"
    if isinstance(group, bool) or not isinstance(group, int) or not 1 <= group <= 4:
        raise ValueError(f"{what}: group must be 1, 2, 3 or 4, got {group!r}")
    if isinstance(D, bool) or not isinstance(D, int) or D < 1 or D % group:
        raise ValueError(f"{what}: D must be a positive multiple of group = {group}, got {D!r}")
    device = torch.device(device)
    if device.type != "cuda":
        raise L.SpkError(f"{what}: the state lives on a HIP device, got {device} (no CPU path)")
    return torch.zeros((D // group, 2 + 2 * group), device=device, dtype=torch.float64)


def causal_filter(x, state, *, weights=None, group=2, rate=30.0, min_cutoff=1.0, beta=0.05, d_cutoff=1.0, hold=5, out=None):
    """A one-euro filter over the next ``N`` frames of a signal, one launch (``spk_causal_filter``; include/spk.h has the recursion):
    a low-pass whose cut-off is ``min_cutoff + beta |filtered speed|`` Hz, so what stands still is held steady and what moves is
    followed without lag -- the causal counterpart of ``smooth_similarity_rows`` for a feed whose next frame does not exist yet,
    applied to the landmarks themselves.  ``x``: a device float32 tensor ``[N, ...]``, frame after frame at ``rate`` frames per
    second, its trailing dimensions flattened to ``D`` components in ``G = D / group`` groups of ``group`` consecutive ones that
    share one speed (landmarks ``[N,K,2]``: ``group=2``; a feature vector: ``group=1``).  ``state``: the float64 ``[G, 2 + 2 group]``
    tensor of ``causal_filter_state``, read at the start and written at the end of the call -- ``N`` frames in one call and the same
    frames in any split of calls give the same bits.  ``weights``: None (all 1); a device float32 ``[G]`` (one set for all frames)
    or ``[N,G]`` tensor, a tracker's confidences; or a host sequence ``[G]``, uploaded.  A group takes part in a frame when its
    weight is finite and > 0 and its components are finite (the rule of ``similarity_from_landmarks``); a drop-out of up to ``hold``
    frames is bridged with the held estimate, a longer one gives NaN from then on and restarts from the first sample that takes
    part.  ``out``: a contiguous device float32 tensor in the shape of ``x`` to write, ``x`` itself included.
    -> ``(y, wy)``: the filtered signal in the shape of ``x``, and float32 ``[N,G]`` weights -- the frame's own where the group took
    part, the last one where it was held, 0 where ``y`` is NaN -- which is what ``similarity_from_landmarks(y, ..., weights=wy)``
    takes."""
    what = "causal_filter"
    group, rate, min_cutoff, beta, d_cutoff, hold = check_filter_params(what, group, rate, min_cutoff, beta, d_cutoff, hold)
    if not isinstance(x, torch.Tensor) or x.dim() < 2 or x.size(0) < 1 or x.numel() < 1 or x.numel() >= 2 ** 31:
        got = tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"{what}: x must be a tensor [N, ...] of N >= 1 frames (fewer than 2^31 numbers), got {got}")
    N, D = x.size(0), x.numel() // x.size(0)
    if D % group:
        raise ValueError(f"{what}: group = {group} does not divide the {D} components of a frame")
    G = D // group
    if not isinstance(state, torch.Tensor) or state.dtype != torch.float64 or tuple(state.shape) != (G, 2 + 2 * group):
        got = f"{state.dtype} {tuple(state.shape)}" if isinstance(state, torch.Tensor) else type(state).__name__
        raise ValueError(f"{what}: state must be a float64 tensor [{G},{2 + 2 * group}] (causal_filter_state), got {got}")
    if isinstance(weights, torch.Tensor) and weights.is_cuda:
        if weights.dtype != torch.float32 or tuple(weights.shape) not in ((G,), (N, G)):
            raise ValueError(f"{what}: device weights must be a float32 tensor [{G}] or [{N},{G}], got {weights.dtype} {tuple(weights.shape)}")
    elif weights is not None:
        try:
            weights = torch.as_tensor(weights).to(torch.float64).to(torch.float32)
        except (ValueError, TypeError, RuntimeError) as e:
            raise ValueError(f"{what}: weights must be [{G}] numbers: {e}") from None
        if tuple(weights.shape) != (G,):
            raise ValueError(f"{what}: host weights must be [{G}] numbers, one per group, got {tuple(weights.shape)}")
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(x.shape)):
        got = tuple(out.shape) if isinstance(out, torch.Tensor) else type(out).__name__
        raise ValueError(f"{what}: out must be a tensor in the shape of x {tuple(x.shape)}, got {got}")
    if not x.is_cuda or x.dtype != torch.float32:
        raise L.SpkError(f"{what}: x: expected a float32 HIP tensor, got {x.dtype} on {x.device} (no CPU path)")
    if state.device != x.device or not state.is_contiguous():
        raise L.SpkError(f"{what}: state: expected a contiguous tensor on {x.device}, got strides {state.stride()} on {state.device}")
    if out is not None and (out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous()):
        raise L.SpkError(f"{what}: out: expected a contiguous float32 tensor on {x.device}, got {out.dtype} on {out.device}")
    if weights is not None:
        if weights.is_cuda and weights.device != x.device:
            raise L.SpkError(f"{what}: weights on {weights.device}, x on {x.device}")
        weights = weights.to(x.device).contiguous()
    x = x.contiguous()
    y = torch.empty_like(x) if out is None else out
    wy = torch.empty((N, G), device=x.device, dtype=torch.float32)
    L.check(L.lib().spk_causal_filter(x.data_ptr(), _ptr(weights), G if weights is not None and weights.dim() == 2 else 0, N, D, group, rate,
                                      min_cutoff, beta, d_cutoff, hold, state.data_ptr(), y.data_ptr(), wy.data_ptr(), L.stream_ptr()),
            "spk_causal_filter")
    return y, wy


def colour_rows_causal(sums, state, decay, *, max_gain=2.0, min_sigma=1.0, min_weight=16.0, out=None):
    """Colour rows from the sums of the next ``N`` frames with exponential forgetting, one launch (``spk_colour_rows_causal``): the
    causal counterpart of ``colour_rows_from_sums``.  ``sums``: a device float64 ``[N,13]`` tensor as ``paste_colour_sums`` /
    ``paste_colour_sums_nv12`` write it.  ``state``: a device float64 ``[13]`` tensor, the pooled sums ``P`` (zeros: nothing yet), read
    at the start and written at the end of the call.  Per frame, ``P <- decay P + S`` when the frame has statistics (``S0 >
    min_weight``, all 13 sums finite), then ``paste_colour_match``'s row formula on ``P`` (``max_gain``, ``min_sigma``, ``min_weight``:
    its parameters; ``(1, 0)`` while ``P0 <= min_weight``).  The sums are linear, so this is the match over a fading stretch of the
    past: ``decay=0`` gives ``paste_colour_match``'s rows bit for bit on frames that all have statistics, ``decay`` near 1 a long
    memory; a frame without statistics keeps the previous row.  ``N`` frames in one call and the same frames in any split of calls
    give the same bits.  ``out``: a contiguous device float32 ``[N,3,2]`` tensor to write.  -> device float32 ``[N,3,2]``."""
    what = "colour_rows_causal"
    try:
        decay = float(decay)
    except (ValueError, TypeError):
        raise ValueError(f"{what}: decay must be a number in [0, 1], got {decay!r}") from None
    if not 0.0 <= decay <= 1.0:
        raise ValueError(f"{what}: decay must be in [0, 1], got {decay}")
    params = _check_match_params(what, max_gain, min_sigma, min_weight)
    if not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64 or sums.dim() != 2 or sums.size(1) != COLOUR_SUMS or sums.size(0) < 1:
        got = f"{sums.dtype} {tuple(sums.shape)}" if isinstance(sums, torch.Tensor) else type(sums).__name__
        raise ValueError(f"{what}: sums must be a float64 tensor [N,{COLOUR_SUMS}], got {got}")
    if not isinstance(state, torch.Tensor) or state.dtype != torch.float64 or tuple(state.shape) != (COLOUR_SUMS,):
        got = f"{state.dtype} {tuple(state.shape)}" if isinstance(state, torch.Tensor) else type(state).__name__
        raise ValueError(f"{what}: state must be a float64 tensor [{COLOUR_SUMS}], got {got}")
    if not sums.is_cuda:
        raise L.SpkError(f"{what}: sums on {sums.device} (no CPU path)")
    if not sums.is_contiguous():
        raise L.SpkError(f"{what}: sums: expected a contiguous tensor, got strides {sums.stride()}")
    if state.device != sums.device or not state.is_contiguous():
        raise L.SpkError(f"{what}: state: expected a contiguous tensor on {sums.device}, got strides {state.stride()} on {state.device}")
    out = _stat_out(out, (sums.size(0), 3, 2), torch.float32, sums.device)
    L.check(L.lib().spk_colour_rows_causal(sums.data_ptr(), sums.size(0), decay, *params, state.data_ptr(), out.data_ptr(), L.stream_ptr()),
            "spk_colour_rows_causal")
    return out


def colour_rows_causal_feeds(sums, state, decay, *, max_gain=2.0, min_sigma=1.0, min_weight=16.0, out=None):
    """``colour_rows_causal`` for ``S`` feeds side by side, one launch (``spk_colour_rows_causal_feeds``).  ``sums``: a device float64
    ``[N,S,13]`` tensor, frame ``n`` of feed ``s``; ``state``: a device float64 ``[S,13]`` tensor, one ``P`` per feed.  Feed ``s`` is
    ``colour_rows_causal(sums[:, s], state[s], decay, ...)`` bit for bit, rows and state, and never touches another feed's.  ``out``:
    a contiguous device float32 ``[N,S,3,2]`` tensor to write.  -> device float32 ``[N,S,3,2]``."""
    what = "colour_rows_causal_feeds"
    try:
        decay = float(decay)
    except (ValueError, TypeError):
        raise ValueError(f"{what}: decay must be a number in [0, 1], got {decay!r}") from None
    if not 0.0 <= decay <= 1.0:
        raise ValueError(f"{what}: decay must be in [0, 1], got {decay}")
    params = _check_match_params(what, max_gain, min_sigma, min_weight)
    if not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64 or sums.dim() != 3 or sums.size(2) != COLOUR_SUMS or sums.size(0) < 1 \
            or sums.size(1) < 1 or sums.numel() >= 2 ** 31:
        got = f"{sums.dtype} {tuple(sums.shape)}" if isinstance(sums, torch.Tensor) else type(sums).__name__
        raise ValueError(f"{what}: sums must be a float64 tensor [N,S,{COLOUR_SUMS}] of N >= 1 frames of S >= 1 feeds (fewer than 2^31 sums), got {got}")
    N, S = sums.size(0), sums.size(1)
    if not isinstance(state, torch.Tensor) or state.dtype != torch.float64 or tuple(state.shape) != (S, COLOUR_SUMS):
        got = f"{state.dtype} {tuple(state.shape)}" if isinstance(state, torch.Tensor) else type(state).__name__
        raise ValueError(f"{what}: state must be a float64 tensor [{S},{COLOUR_SUMS}], one row per feed of the sums, got {got}")
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (N, S, 3, 2) or out.dtype != torch.float32):
        got = f"{out.dtype} {tuple(out.shape)}" if isinstance(out, torch.Tensor) else type(out).__name__
        raise ValueError(f"{what}: out must be a float32 tensor [{N},{S},3,2], got {got}")
    if not sums.is_cuda:
        raise L.SpkError(f"{what}: sums on {sums.device} (no CPU path)")
    if not sums.is_contiguous():
        raise L.SpkError(f"{what}: sums: expected a contiguous tensor, got strides {sums.stride()}")
    if state.device != sums.device or not state.is_contiguous():
        raise L.SpkError(f"{what}: state: expected a contiguous tensor on {sums.device}, got strides {state.stride()} on {state.device}")
    out = _stat_out(out, (N, S, 3, 2), torch.float32, sums.device)
    L.check(L.lib().spk_colour_rows_causal_feeds(sums.data_ptr(), N, S, decay, *params, state.data_ptr(), out.data_ptr(), L.stream_ptr()),
            "spk_colour_rows_causal_feeds")
    return out


# ---- NV12 (csrc/frame_nv12.hip; the definitions are in include/spk.h) ---------------------------------------------------------------
def yuv_standard(standard, full_range):
    if standard not in ("bt601", "bt709"):
        raise ValueError(f"standard must be 'bt601' or 'bt709', got {standard!r}")
    if not isinstance(full_range, (bool, int)) or full_range not in (0, 1):
        raise ValueError(f"full_range must be a bool, got {full_range!r}")
    return (601 if standard == "bt601" else 709), int(full_range)


def yuv_coeffs(standard="bt601", full_range=False):
    """The two 3 x 4 affine maps in byte units between R'G'B' 0..255 and the Y, U, V bytes (``spk_yuv_coeffs``, built in fp64 on the
    host from the primaries): ``to_rgb`` rows R, G, B over ``(y, u, v, 1)``; ``from_rgb`` rows Y, U, V over ``(r, g, b, 1)``.
    ``standard``: "bt601" | "bt709"; limited range (Y 16..235, C 16..240) unless ``full_range``.  -> two CPU float64 tensors [3,4]."""
    std, full = yuv_standard(standard, full_range)
    to_rgb, from_rgb = (C.c_double * 12)(), (C.c_double * 12)()
    L.check(L.lib().spk_yuv_coeffs(std, full, to_rgb, from_rgb), "spk_yuv_coeffs")
    return torch.tensor(list(to_rgb), dtype=torch.float64).view(3, 4), torch.tensor(list(from_rgb), dtype=torch.float64).view(3, 4)


def nv12_planes(nv12):
    """The two planes of NV12 frames as views.  ``nv12``: one uint8 tensor ``[N, 3H/2, W]`` (or ``[3H/2, W]``), a decoder surface
    with unit pixel stride and any row pitch whose rows ``H..`` are the UV plane; or a pair ``(y [N,H,W], uv [N,H/2,W/2,2])``
    (planes that live apart).  ``H`` and ``W`` are even.  -> ``(y [N,H,W], uv [N,H/2,W/2,2])``, no copy."""
    if isinstance(nv12, (tuple, list)):
        if len(nv12) != 2 or not all(isinstance(t, torch.Tensor) for t in nv12):
            raise ValueError("nv12: a pair must be (y [N,H,W], uv [N,H/2,W/2,2])")
        y, uv = nv12
        if y.dim() == 2 and uv.dim() == 3:
            y, uv = y.unsqueeze(0), uv.unsqueeze(0)
        if y.dim() != 3 or uv.dim() != 4 or y.size(0) < 1 or y.size(1) % 2 or y.size(2) % 2 or y.size(1) < 2 or y.size(2) < 2 or \
                tuple(uv.shape) != (y.size(0), y.size(1) // 2, y.size(2) // 2, 2):
            raise ValueError(f"nv12: planes must be y [N,H,W] and uv [N,H/2,W/2,2] with even H, W, got {tuple(y.shape)} and {tuple(uv.shape)}")
        if y.dtype != torch.uint8 or uv.dtype != torch.uint8 or y.device != uv.device:
            raise ValueError(f"nv12: planes must be uint8 tensors on one device, got {y.dtype} on {y.device} and {uv.dtype} on {uv.device}")
        return y, uv
    if not isinstance(nv12, torch.Tensor):
        raise ValueError("nv12: expected a uint8 tensor [N,3H/2,W] or a pair of planes")
    buf = nv12.unsqueeze(0) if nv12.dim() == 2 else nv12
    if buf.dim() != 3 or buf.size(0) < 1 or buf.size(1) % 3 or buf.size(1) < 3 or buf.size(2) % 2 or buf.size(2) < 2:
        raise ValueError(f"nv12: a surface must be [N,3H/2,W] with even H, W, got {tuple(nv12.shape)}")
    if buf.dtype != torch.uint8:
        raise ValueError(f"nv12: a surface must be uint8, got {buf.dtype}")
    N, W = buf.size(0), buf.size(2)
    H = buf.size(1) // 3 * 2
    if buf.stride(2) != 1:
        raise ValueError(f"nv12: a surface must have unit pixel stride, got strides {buf.stride()}")
    return buf[:, :H], buf[:, H:].unflatten(2, (W // 2, 2))


def nv12_strides(y, uv, what, written):
    """Byte strides of the two planes as the kernels take them, checked on the host."""
    N, H, W = y.shape
    if not y.is_cuda or y.dtype != torch.uint8 or not uv.is_cuda:
        raise L.SpkError(f"{what}: expected uint8 HIP tensors, got {y.dtype} on {y.device} (no CPU path)")
    if y.stride(2) != 1 or uv.stride(3) != 1 or uv.stride(2) != 2:
        raise L.SpkError(f"{what}: the Y pixel stride must be 1 and a UV pair packed, got strides {y.stride()} and {uv.stride()}")
    ys, us = (y.stride(0) if N > 1 else 0, y.stride(1)), (uv.stride(0) if N > 1 else 0, uv.stride(1))
    if ys[1] < W or us[1] < W or uv.data_ptr() % 2 or us[0] % 2 or us[1] % 2:
        raise L.SpkError(f"{what}: rows must hold W = {W} bytes and the UV plane be 2-byte aligned with even strides, "
                         f"got strides {y.stride()} and {uv.stride()}")
    if N > 1 and (ys[0] < 0 or us[0] < 0 or (written and (ys[0] < (H - 1) * ys[1] + W or us[0] < (H // 2 - 1) * us[1] + W))):
        raise L.SpkError(f"{what}: frames must not overlap, got strides {y.stride()} and {uv.stride()}")
    return ys, us


def frames_from_nv12(nv12, size, *, crop=None, channel_order="rgb", mean=0.5, std=0.5, standard="bt601", full_range=False):
    """NV12 video frames -> the network's input, one launch (``spk_frames_nv12_to_f32``): crop, antialiased bilinear resize of the
    Y, U and V fields to ``size`` x ``size`` (a number, or ``(H, W)``), YUV -> RGB (``yuv_coeffs``), clamp to 0..255 and
    ``(x / 255 - mean) / std`` per channel, CHW.  ``nv12``: what ``nv12_planes`` takes, on the device, read in place through its
    strides.  ``crop``: the three forms of ``parse_boxes``; an origin may be odd (chroma is sited by replication: pixel ``(Y, X)``
    has sample ``(Y >> 1, X >> 1)``); device origins are clamped by the kernel so that the box stays inside the frame.
    ``channel_order`` only says which plane order the network input has ("bgr": planes B, G, R).  -> float32 [N,3,size,size]."""
    return _from_boxes(_SURFACES, "frames_from_nv12", nv12, size, crop, channel_order, mean, std, standard, full_range)


class _Surfaces:
    """``_Packed`` for NV12: the frames of a call as what ``nv12_planes`` takes (csrc/frame_nv12.hip, csrc/frame_sim_nv12.hip)."""
    layout = "NV12"
    way_in, paste = "spk_frames_nv12_to_f32_sim", "spk_frames_paste_nv12_sim"
    sums, match = "spk_paste_colour_sums_nv12_sim", "spk_paste_colour_match_nv12_sim"
    box_in, box_paste, whole = "spk_frames_nv12_to_f32", "spk_frames_paste_nv12", "spk_frames_f32_to_nv12"      # the axis-aligned edge

    def shaped(self, nv12, N, what):                                      # -> ((y, uv), N, H, W)
        y, uv = nv12_planes(nv12)
        if N is not None and y.size(0) != N:
            raise ValueError(f"{what}: {N} generated frames, {y.size(0)} NV12 frames")
        return ((y, uv), *y.shape)

    def on_device(self, planes, device=None):
        if not planes[0].is_cuda:
            raise L.SpkError(f"frames: expected uint8 HIP tensors, got {planes[0].dtype} on {planes[0].device} (no CPU path)")

    def read(self, planes, what, disjoint=False):                         # always in place; -> (the Y plane, the two pointers with their strides)
        y, uv = planes
        ys, us = nv12_strides(y, uv, what, written=False)
        return y, (y.data_ptr(), *ys, uv.data_ptr(), *us)

    def target(self, planes, out, N, H, W, device, what):
        """The surface a launcher writes: ``out`` (what ``nv12_planes`` takes) or a fresh packed ``[N, 3H/2, W]`` buffer; ``fill()``
        copies each plane of ``planes`` that is not the result's own"""
        if out is None:
            out = torch.empty((N, 3 * H // 2, W), device=device, dtype=torch.uint8)
        y, uv = nv12_planes(out)
        if tuple(y.shape) != (N, H, W):
            raise L.SpkError(f"{what}: out must hold {N} NV12 frames of {H} x {W}, got planes {tuple(y.shape)}")
        ys, us = nv12_strides(y, uv, f"{what}: out", written=True)

        def fill():
            for dst, src in ((y, planes[0]), (uv, planes[1])):
                if dst.data_ptr() != src.data_ptr() or dst.stride() != src.stride():
                    dst.copy_(src)
        return out, (y.data_ptr(), *ys, uv.data_ptr(), *us), fill

    def size(self, H, W):
        return (H, W)

    def standard(self, standard="bt601", full_range=False):
        return yuv_standard(standard, full_range)

    def quantised(self, value_range, standard="bt601", full_range=False):
        lo, k = quant_range(value_range)
        return yuv_standard(standard, full_range), lo, k

    def blend(self, matte_args, colour):                                  # one entry point, with or without matte and colour rows
        return self.paste, (*matte_args, _ptr(colour))


_SURFACES = _Surfaces()


# The three axis-aligned launchers of a Y, U, V format (``fmt``: ``_SURFACES`` or ``_PLANAR``): one body per launcher, the format
# says how its surfaces are parsed and addressed and which entry point takes them.
def _from_boxes(fmt, what, frames, size, crop, channel_order, mean, std, standard, full_range):
    planes, N, H, W = fmt.shaped(frames, None, what)
    Hout, Wout = _out_size(size, what)
    swap = _channel_swap(channel_order)
    code, full = yuv_standard(standard, full_range)
    scale, shift = _affine(mean, std, what)
    origins, h, w = parse_boxes((0, 0, H, W) if crop is None else crop, N, H, W, f"{what}: crop")
    y, where = fmt.read(planes, what)
    y0, x0, boxes = _origins(origins, y.device, what)
    out = torch.empty((N, 3, Hout, Wout), device=y.device, dtype=torch.float32)
    L.check(getattr(L.lib(), fmt.box_in)(*where, N, H, W, _ptr(boxes), y0, x0, h, w, swap, code, full,
                                         *_table_args(_device_tables(y.device, h, w, Hout, Wout)), out.data_ptr(), Hout, Wout, *scale, *shift,
                                         L.stream_ptr()), fmt.box_in)
    return out


def _to_surfaces(fmt, what, x, value_range, standard, full_range, out):
    _check_chw(x, what)
    N, _, H, W = x.shape
    if H % 2 or W % 2 or H < 2 or W < 2:
        raise ValueError(f"{what}: {fmt.layout} frames have an even height and width, got {H} x {W}")
    lo, k = quant_range(value_range)
    code, full = yuv_standard(standard, full_range)
    xp = L.dptr(x, "x")
    out, where, _ = fmt.target(None, out, N, H, W, x.device, what)
    L.check(getattr(L.lib(), fmt.whole)(xp, N, H, W, *where, code, full, lo, k, L.stream_ptr()), fmt.whole)
    return out


def _paste_boxes(fmt, what, x, frames, box, feather, value_range, standard, full_range, out):
    _check_chw(x, what)
    N, _, Hs, Ws = x.shape
    planes, _, H, W = fmt.shaped(frames, N, what)
    (code, full), lo, k = fmt.quantised(value_range, standard, full_range)
    feather = check_feather(feather, what)
    origins, h, w = parse_boxes(box, N, H, W, f"{what}: box", inside=False)
    xp = L.dptr(x, "x")
    fmt.on_device(planes)
    out, where, fill = fmt.target(planes, out, N, H, W, x.device, what)
    y0, x0, boxes = _origins(origins, x.device, what)
    fill()
    tables, ay, ax = _paste_tables(Hs, Ws, h, w, feather, x.device)
    L.check(getattr(L.lib(), fmt.box_paste)(xp, N, Hs, Ws, *where, H, W, h, w, y0, x0, _ptr(boxes), code, full, *tables, ay, ax, lo, k,
                                            L.stream_ptr()), fmt.box_paste)
    return out


# ---- a surface table: every NV12 surface its own planes, pitches and size (csrc/frame_table_nv12.hip; include/spk.h) ---------------
def plane_pair(nv12) -> bool:
    """A pair ``(y, uv)`` of planes -- the UV plane has one dimension more -- and not a sequence of two surfaces"""
    return isinstance(nv12, (tuple, list)) and len(nv12) == 2 and all(isinstance(t, torch.Tensor) for t in nv12) and \
        nv12[1].dim() == nv12[0].dim() + 1


class SurfaceTable(_DeviceTable):
    """``N`` NV12 surfaces that share neither an allocation nor a size, as the aligned NV12 launchers address them: a device table of
    ``spk_surface_ref`` entries ``(y, uv, y_row_stride, uv_row_stride, H, W)``.  ``surfaces``: a sequence whose elements are what
    ``nv12_planes`` takes for ONE frame -- a uint8 tensor ``[3H/2, W]`` with unit pixel stride and any (even) pitch, or a pair
    ``(y [H,W], uv [H/2,W/2,2])`` of planes that live apart; a region of interest at even offsets of a wider surface is such a pair
    of views -- on one device, with ``None`` for a surface that is ABSENT (an all-zero entry: the launchers treat it like an invalid
    transform); or one ``[N,3H/2,W]`` tensor or one pair of planes ``(y [N,H,W], uv [N,H/2,W/2,2])``, which give views of their
    frames.  Wrong types, shapes or strides raise ``ValueError`` before a device is touched; CPU tensors raise ``SpkError`` (no CPU
    path).  The host table is checked (``spk_surface_table_check``) here and uploaded ONCE, one host -> device copy of ``40 N`` bytes
    on the current stream, when a launcher first uses the table (so a call that is refused on the host has copied nothing); whether
    the surfaces may be written is decided where the table is used (``check_written``: the paste).  The table HOLDS REFERENCES to the
    tensors, so the addresses in it stay the tensors' for as long as it lives.

    ``dev``: the device table (uint8 ``[40 N]``); ``sizes``: ``(H, W)`` per surface (``(0, 0)``: absent); ``surfaces``: the elements as
    they were given; ``planes``: ``(y [H,W], uv [H/2,W/2,2])`` views per surface, or None."""

    def __init__(self, surfaces):
        what = "SurfaceTable"
        if isinstance(surfaces, torch.Tensor) or plane_pair(surfaces):
            if isinstance(surfaces, torch.Tensor) and surfaces.dim() != 3:
                raise ValueError(f"{what}: a tensor of surfaces must be [N,3H/2,W], got {tuple(surfaces.shape)}")
            y, uv = nv12_planes(surfaces)
            surfaces = list(zip(y.unbind(0), uv.unbind(0)))
        else:
            try:
                surfaces = list(surfaces)
            except TypeError:
                raise ValueError(f"{what}: surfaces must be a sequence of NV12 surfaces ([3H/2,W] tensors or pairs of planes), a tensor "
                                 f"[N,3H/2,W] or a pair of planes, got {type(surfaces).__name__}") from None
        if not surfaces:
            raise ValueError(f"{what}: a table needs at least one surface")
        planes = []
        for n, s in enumerate(surfaces):
            if s is None:
                planes.append(None)
                continue
            if isinstance(s, torch.Tensor) and s.dim() != 2:
                raise ValueError(f"{what}: surfaces[{n}] must be ONE surface, a uint8 tensor [3H/2,W] or a pair (y [H,W], uv [H/2,W/2,2]), "
                                 f"got {tuple(s.shape)}")
            try:
                y, uv = nv12_planes(s)
            except ValueError as e:
                raise ValueError(f"{what}: surfaces[{n}]: {e}") from None
            if y.size(0) != 1:
                raise ValueError(f"{what}: surfaces[{n}] must be ONE surface, got planes of {y.size(0)} frames")
            y, uv = y[0], uv[0]
            W = y.size(1)
            if y.stride(1) != 1 or uv.stride(2) != 1 or uv.stride(1) != 2 or y.stride(0) < W or uv.stride(0) < W or uv.stride(0) % 2:
                raise ValueError(f"{what}: surfaces[{n}]: the Y pixel stride must be 1, a UV pair packed, rows must hold W = {W} bytes and the "
                                 f"UV pitch be even, got strides {y.stride()} and {uv.stride()}")
            planes.append((y, uv))
        there = [p for p in planes if p is not None]
        if any(not p[0].is_cuda for p in there):
            raise L.SpkError(f"{what}: expected uint8 HIP tensors, got a surface on the CPU (no CPU path)")
        if any(p[0].device != there[0][0].device for p in there):
            raise L.SpkError(f"{what}: the surfaces must be on one device, got {sorted({str(p[0].device) for p in there})}")
        self.surfaces, self.planes, self.N = surfaces, planes, len(surfaces)
        self.sizes = [(0, 0) if p is None else tuple(p[0].shape) for p in planes]
        self._host = (L.SurfaceRef * self.N)()
        for e, p in zip(self._host, planes):
            if p is not None:
                e.y, e.uv, e.y_row_stride, e.uv_row_stride, e.H, e.W = p[0].data_ptr(), p[1].data_ptr(), p[0].stride(0), p[1].stride(0), *p[0].shape
        self._checked("spk_surface_table_check", there[0][0].device if there else None)


class _TabledSurfaces(_Tabled):
    """``_Surfaces`` for a ``SurfaceTable``, as ``_Tabled`` is ``_Packed`` for a ``FrameTable`` (csrc/frame_table_nv12.hip): the size
    of a surface is its entry's, the surfaces are addressed where they are, and the colour arguments are NV12's."""
    noun = "surface table"
    way_in, paste = "spk_frames_nv12_to_f32_sim_table", "spk_frames_paste_nv12_sim_table"
    sums, match = "spk_paste_colour_sums_nv12_sim_table", "spk_paste_colour_match_nv12_sim_table"

    def standard(self, standard="bt601", full_range=False):
        return yuv_standard(standard, full_range)

    def quantised(self, value_range, standard="bt601", full_range=False):
        return _SURFACES.quantised(value_range, standard, full_range)


_TABLED_SURFACES = _TabledSurfaces()


def _nv12_format(nv12):                                                   # a tensor or a pair takes exactly the path it always took
    return _TABLED_SURFACES if isinstance(nv12, SurfaceTable) else _SURFACES


def clone_surfaces(nv12):
    """A packed copy of the surfaces to paste into: of a ``SurfaceTable`` a new table over one packed ``[3H/2, W]`` clone per surface (a
    table of its own: its host check and, at its first launch, its upload come on top of the clones); else the one clone of
    ``Nv12.clone``, a packed ``[N, 3H/2, W]`` tensor"""
    if isinstance(nv12, SurfaceTable):
        clones = []
        for p in nv12.planes:
            if p is None:
                clones.append(None)
                continue
            out, _, fill = _SURFACES.target((p[0].unsqueeze(0), p[1].unsqueeze(0)), None, 1, *p[0].shape, p[0].device, "clone_surfaces")
            fill()
            clones.append(out[0])
        return SurfaceTable(clones)
    planes = nv12_planes(nv12)
    out, _, fill = _SURFACES.target(planes, None, *planes[0].shape, planes[0].device, "clone_surfaces")
    fill()
    return out


def frames_to_nv12(x, *, value_range=(-1, 1), standard="bt601", full_range=False, out=None):
    """Network frames -> NV12 for a hardware encoder, one launch (``spk_frames_f32_to_nv12``): float32 [N,3,H,W] (R, G, B planes,
    ``H`` and ``W`` even) in ``value_range`` is quantised as ``frames_to_u8`` does without its rounding, converted with
    ``from_rgb`` of ``yuv_coeffs`` in fp64, and stored as ``Y = rint(clamp(e_y))`` per pixel and ``C = rint(clamp(mean of the four
    e_c))`` per 2 x 2 block.  ``out``: what ``nv12_planes`` takes (any row pitch).  -> uint8 [N, 3H/2, W], or ``out``."""
    return _to_surfaces(_SURFACES, "frames_to_nv12", x, value_range, standard, full_range, out)


def frames_paste_nv12(x, nv12, box, *, feather=0, value_range=(-1, 1), standard="bt601", full_range=False, out=None):
    """Generated frames back into the NV12 video they were cropped from, one launch (``spk_frames_paste_nv12``): float32
    [N,3,Hs,Ws] in ``value_range`` is resized to the box size ``h x w``, quantised, converted to YUV and blended over the box with
    weight ``m = a_y[y] a_x[x]`` of ``feather_tables``: luma per pixel, chroma per 2 x 2 block as the quarter-weighted sum of the
    block's box pixels over the sample underneath (include/spk.h has the arithmetic).  ``box``: the three forms of
    ``parse_boxes``; origins may be odd; box pixels outside the frame are skipped.  ``out=None``: the result is a packed clone of
    ``nv12``; ``out=nv12`` (the same tensor, or the same pair of planes): pasted in place through its strides; another ``out``
    first receives a copy.  -> uint8 [N, 3H/2, W], or ``out``."""
    return _paste_boxes(_SURFACES, "frames_paste_nv12", x, nv12, box, feather, value_range, standard, full_range, out)


# ---- aligned crops on NV12 surfaces (csrc/frame_sim_nv12.hip; the definitions are in include/spk.h) --------------------------------
def frames_from_nv12_aligned(nv12, size, sim, *, channel_order="rgb", mean=0.5, std=0.5, standard="bt601", full_range=False):
    """NV12 video frames -> the network's input through a similarity transform PER FRAME, one launch
    (``spk_frames_nv12_to_f32_sim``): ``frames_from_u8_aligned`` on surfaces.  The footprint and the fp64 weights are that
    launcher's; they run over the Y, U and V fields (chroma by replication), then YUV -> RGB (``yuv_coeffs``), clamp to 0..255 and
    ``(x / 255 - mean) / std`` as ``frames_from_nv12``.  An output whose footprint misses the frame is ``-mean / std`` exactly, and
    so is every output of a frame whose device row is invalid.  ``nv12``: what ``nv12_planes`` takes, on the device, read in place
    through its strides; ``sim``: the two forms of ``parse_sim``; ``channel_order``: the plane order of the result, as
    ``frames_from_nv12``.  ``nv12`` may be a ``SurfaceTable``: surfaces of their own sizes in their own buffers, still one launch
    (``spk_frames_nv12_to_f32_sim_table``), frame ``n`` bit for bit this call on surface ``n`` alone; an absent surface gives
    ``-mean / std``.  -> float32 [N,3,size,size]."""
    return _from_aligned(_nv12_format(nv12), "frames_from_nv12_aligned", nv12, size, sim, channel_order, mean, std, standard=standard, full_range=full_range)


def frames_paste_nv12_aligned(x, nv12, sim, *, feather=0, value_range=(-1, 1), standard="bt601", full_range=False, out=None, matte=None,
                              colour=None):
    """Generated frames back into the NV12 video they were cropped from through ``sim``, one launch (``spk_frames_paste_nv12_sim``):
    the inverse of ``frames_from_nv12_aligned``, and ``frames_paste_u8_aligned`` on surfaces.  Region, value, ``feather`` ramp,
    ``matte`` and ``colour`` rows are that launcher's (rows act on the R, G, B value in front of the conversion, so
    ``paste_colour_match_nv12`` and ``paste_colour_match`` rows mean the same thing); the result is converted with ``from_rgb`` of
    ``yuv_coeffs`` and blended as ``frames_paste_nv12`` blends: luma per pixel, chroma per 2 x 2 block as the quarter-weighted sum
    of the block's region pixels over the sample underneath.  Every byte outside the region's pixels and blocks is left as it is; a
    device row that is invalid leaves its frame untouched.  ``nv12``, ``out``: as ``frames_paste_nv12`` (``out=nv12`` pastes in
    place).  -> uint8 [N, 3H/2, W], or ``out``.

    ``nv12`` may be a ``SurfaceTable`` (``spk_frames_paste_nv12_sim_table``, one launch): the paste is then IN PLACE, into the table's
    own surfaces (``out``: None or the table), no two planes of which may share bytes; an absent surface is left alone; surface ``n``
    gets the bytes of this call on surface ``n`` alone.  -> the table."""
    return _paste_aligned(_nv12_format(nv12), "frames_paste_nv12_aligned", x, nv12, sim, feather, value_range, out, matte, colour, standard=standard,
                          full_range=full_range)


def paste_colour_match_nv12(x, nv12, sim, *, matte=None, feather=0, value_range=(-1, 1), standard="bt601", full_range=False, max_gain=2.0,
                            min_sigma=1.0, min_weight=16.0, out=None):
    """The colour rows ``frames_paste_nv12_aligned(colour=)`` takes, two launches (``spk_paste_colour_match_nv12_sim``):
    ``paste_colour_match`` for a surface background.  The same sums, weights, row formula and arguments; the background of a
    region pixel is what ``frames_from_nv12_aligned`` makes of it, ``clamp(to_rgb . (Y, U, V, 1))``, so the rows are per network
    channel R, G, B.  ``nv12`` is only read -- call this BEFORE pasting in place.  Reduced in a fixed order without atomics: the
    same inputs give the same bits.  ``out``: a contiguous device float32 ``[N,3,2]`` tensor to write.  ``nv12`` may be a
    ``SurfaceTable`` (``spk_paste_colour_match_nv12_sim_table``; an absent surface gets ``(1, 0)``).
    -> device float32 ``[N,3,2]``."""
    what = "paste_colour_match_nv12"
    params = _check_match_params(what, max_gain, min_sigma, min_weight)
    return _colour_statistics(_nv12_format(nv12), params, what, x, nv12, sim, matte, feather, value_range, out, standard=standard, full_range=full_range)


def paste_colour_sums_nv12(x, nv12, sim, *, matte=None, feather=0, value_range=(-1, 1), standard="bt601", full_range=False, out=None):
    """``paste_colour_sums`` for a surface background, two launches (``spk_paste_colour_sums_nv12_sim``): the 13 sums
    ``paste_colour_match_nv12`` makes its rows from, bit for bit, per network channel R, G, B -- so ``colour_rows_from_sums`` serves
    both pixel formats.  ``out``: a contiguous device float64 ``[N,13]`` tensor to write (a slice of a clip-long one).  ``nv12`` may
    be a ``SurfaceTable`` (``spk_paste_colour_sums_nv12_sim_table``; 13 zeros for an absent surface).
    -> device float64 ``[N,13]``."""
    return _colour_statistics(_nv12_format(nv12), None, "paste_colour_sums_nv12", x, nv12, sim, matte, feather, value_range, out, standard=standard,
                              full_range=full_range)


# ---- aligned crops on I420 surfaces: three planes (csrc/frame_sim_i420.hip, csrc/frame_table_i420.hip; include/spk.h) --------------
def plane_triple(i420, one=True) -> bool:
    """A triple ``(y, u, v)`` of planes and not a sequence of three surfaces (which are 2-D packed tensors ``[3H/2, W]`` or triples
    themselves): three 3-D tensors, or -- where ONE frame may be meant (``one``) -- three 2-D ones, the last two of half the first's
    rows and columns"""
    if not (isinstance(i420, (tuple, list)) and len(i420) == 3 and all(isinstance(t, torch.Tensor) for t in i420)):
        return False
    y, u, v = i420
    if y.dim() == u.dim() == v.dim() == 3:
        return True
    return one and y.dim() == u.dim() == v.dim() == 2 and tuple(u.shape) == tuple(v.shape) == (y.size(0) // 2, y.size(1) // 2)


def i420_planes(i420):
    """The three planes of I420 frames as views.  ``i420``: a triple ``(y [N,H,W], u [N,H/2,W/2], v [N,H/2,W/2])`` of planes that
    live where a decoder left them, in any order in memory and with any row pitch (2-D / 2-D / 2-D for one frame); or one CONTIGUOUS
    uint8 tensor ``[N, 3H/2, W]`` (or ``[3H/2, W]``) in packed I420 layout -- the ``H`` rows of Y, then the ``HW/4`` bytes of U, then
    those of V (``yuv420p`` in one buffer); a non-contiguous one is refused, since the chroma bytes are not rows of the tensor.
    ``H`` and ``W`` are even.  -> ``(y [N,H,W], u [N,H/2,W/2], v [N,H/2,W/2])``, no copy."""
    if isinstance(i420, (tuple, list)):
        if len(i420) != 3 or not all(isinstance(t, torch.Tensor) for t in i420):
            raise ValueError("i420: a triple must be (y [N,H,W], u [N,H/2,W/2], v [N,H/2,W/2])")
        y, u, v = i420
        if y.dim() == 2 and u.dim() == 2 and v.dim() == 2:
            y, u, v = y.unsqueeze(0), u.unsqueeze(0), v.unsqueeze(0)
        half = (y.size(0), y.size(1) // 2, y.size(2) // 2) if y.dim() == 3 else None
        if y.dim() != 3 or y.size(0) < 1 or y.size(1) % 2 or y.size(2) % 2 or y.size(1) < 2 or y.size(2) < 2 or tuple(u.shape) != half or \
                tuple(v.shape) != half:
            raise ValueError(f"i420: planes must be y [N,H,W], u [N,H/2,W/2] and v [N,H/2,W/2] with even H, W, got {tuple(y.shape)}, "
                             f"{tuple(u.shape)} and {tuple(v.shape)}")
        if any(t.dtype != torch.uint8 for t in (y, u, v)) or u.device != y.device or v.device != y.device:
            raise ValueError(f"i420: planes must be uint8 tensors on one device, got {y.dtype} on {y.device}, {u.dtype} on {u.device} and "
                             f"{v.dtype} on {v.device}")
        return y, u, v
    if not isinstance(i420, torch.Tensor):
        raise ValueError("i420: expected a uint8 tensor [N,3H/2,W] or a triple of planes")
    buf = i420.unsqueeze(0) if i420.dim() == 2 else i420
    if buf.dim() != 3 or buf.size(0) < 1 or buf.size(1) % 3 or buf.size(1) < 3 or buf.size(2) % 2 or buf.size(2) < 2:
        raise ValueError(f"i420: a packed surface must be [N,3H/2,W] with even H, W, got {tuple(i420.shape)}")
    if buf.dtype != torch.uint8:
        raise ValueError(f"i420: a packed surface must be uint8, got {buf.dtype}")
    if not buf.is_contiguous():
        raise ValueError(f"i420: a packed surface must be contiguous (its U and V bytes follow the Y rows), got strides {i420.stride()}; "
                         "give planes with a pitch as a triple (y, u, v)")
    N, W = buf.size(0), buf.size(2)
    H = buf.size(1) // 3 * 2
    flat, q = buf.view(N, -1), H * W // 4
    return buf[:, :H], flat[:, H * W:H * W + q].view(N, H // 2, W // 2), flat[:, H * W + q:].view(N, H // 2, W // 2)


def i420_strides(y, u, v, what, written):
    """Byte strides of the three planes as the kernels take them, checked on the host: -> three ``(image_stride, row_stride)``"""
    N, H, W = y.shape
    if not all(t.is_cuda and t.dtype == torch.uint8 for t in (y, u, v)):
        raise L.SpkError(f"{what}: expected uint8 HIP tensors, got {y.dtype} on {y.device} (no CPU path)")
    if y.stride(2) != 1 or u.stride(2) != 1 or v.stride(2) != 1:
        raise L.SpkError(f"{what}: the pixel stride of every plane must be 1, got strides {y.stride()}, {u.stride()} and {v.stride()}")
    strides = [(t.stride(0) if N > 1 else 0, t.stride(1)) for t in (y, u, v)]
    if strides[0][1] < W or strides[1][1] < W // 2 or strides[2][1] < W // 2:
        raise L.SpkError(f"{what}: rows must hold W = {W} (Y) and W / 2 (U, V) bytes, got strides {y.stride()}, {u.stride()} and {v.stride()}")
    extents = ((H - 1) * strides[0][1] + W, (H // 2 - 1) * strides[1][1] + W // 2, (H // 2 - 1) * strides[2][1] + W // 2)
    if N > 1 and any(s[0] < 0 or (written and s[0] < e) for s, e in zip(strides, extents)):
        raise L.SpkError(f"{what}: frames must not overlap, got strides {y.stride()}, {u.stride()} and {v.stride()}")
    return strides


def _planar_where(planes, strides):                                       # the nine surface arguments of a strided entry point
    return tuple(a for t, s in zip(planes, strides) for a in (t.data_ptr(), *s))


class _Planar(_Surfaces):
    """``_Surfaces`` for I420: the frames of a call as what ``i420_planes`` takes (csrc/frame_sim_i420.hip); the colour arguments
    are NV12's"""
    layout = "I420"
    way_in, paste = "spk_frames_i420_to_f32_sim", "spk_frames_paste_i420_sim"
    sums, match = "spk_paste_colour_sums_i420_sim", "spk_paste_colour_match_i420_sim"
    box_in, box_paste, whole = "spk_frames_i420_to_f32", "spk_frames_paste_i420", "spk_frames_f32_to_i420"      # csrc/frame_i420.hip

    def shaped(self, i420, N, what):                                      # -> ((y, u, v), N, H, W)
        planes = i420_planes(i420)
        if N is not None and planes[0].size(0) != N:
            raise ValueError(f"{what}: {N} generated frames, {planes[0].size(0)} I420 frames")
        return (planes, *planes[0].shape)

    def read(self, planes, what, disjoint=False):                         # always in place; -> (the Y plane, the three pointers with their strides)
        return planes[0], _planar_where(planes, i420_strides(*planes, what, written=False))

    def target(self, planes, out, N, H, W, device, what):
        """The surface a launcher writes: ``out`` (what ``i420_planes`` takes) or a fresh packed ``[N, 3H/2, W]`` buffer; ``fill()``
        copies each plane of ``planes`` that is not the result's own"""
        if out is None:
            out = torch.empty((N, 3 * H // 2, W), device=device, dtype=torch.uint8)
        dst = i420_planes(out)
        if tuple(dst[0].shape) != (N, H, W):
            raise L.SpkError(f"{what}: out must hold {N} I420 frames of {H} x {W}, got planes {tuple(dst[0].shape)}")
        where = _planar_where(dst, i420_strides(*dst, f"{what}: out", written=True))

        def fill():
            for d, s in zip(dst, planes):
                if d.data_ptr() != s.data_ptr() or d.stride() != s.stride():
                    d.copy_(s)
        return out, where, fill


_PLANAR = _Planar()


class PlanarTable(_DeviceTable):
    """``N`` I420 surfaces that share neither an allocation nor a size, as the aligned I420 launchers address them: a device table of
    ``spk_planar_ref`` entries ``(y, u, v, y_row_stride, u_row_stride, v_row_stride, H, W)``.  ``surfaces``: a sequence whose elements
    are what ``i420_planes`` takes for ONE frame -- a contiguous uint8 tensor ``[3H/2, W]`` in packed I420 layout, or a triple
    ``(y [H,W], u [H/2,W/2], v [H/2,W/2])`` of planes that live apart, each with unit pixel stride and any pitch (odd ones and odd
    base addresses included; V may come first in memory); a region of interest at even luma offsets of a wider surface is such a
    triple of views -- on one device, with ``None`` for a surface that is ABSENT (an all-zero entry: the launchers treat it like an
    invalid transform); or one packed ``[N,3H/2,W]`` tensor or one triple of planes ``(y [N,H,W], u [N,H/2,W/2], v [N,H/2,W/2])``,
    which give views of their frames.  Wrong types, shapes or strides raise ``ValueError`` before a device is touched; CPU tensors
    raise ``SpkError`` (no CPU path).  The host table is checked (``spk_planar_table_check``) here and uploaded ONCE, one host ->
    device copy of ``56 N`` bytes on the current stream, when a launcher first uses the table (so a call that is refused on the host
    has copied nothing); whether the surfaces may be written is decided where the table is used (``check_written``: the paste; the
    rule is over byte RANGES, so chroma halves laid side by side on one pitch count as overlapping).  The table HOLDS REFERENCES to
    the tensors, so the addresses in it stay the tensors' for as long as it lives.

    ``dev``: the device table (uint8 ``[56 N]``); ``sizes``: ``(H, W)`` per surface (``(0, 0)``: absent); ``surfaces``: the elements as
    they were given; ``planes``: ``(y [H,W], u [H/2,W/2], v [H/2,W/2])`` views per surface, or None."""

    def __init__(self, surfaces):
        what = "PlanarTable"
        if isinstance(surfaces, torch.Tensor) or plane_triple(surfaces, one=False):
            if isinstance(surfaces, torch.Tensor) and surfaces.dim() != 3:
                raise ValueError(f"{what}: a tensor of surfaces must be [N,3H/2,W], got {tuple(surfaces.shape)}")
            surfaces = list(zip(*(p.unbind(0) for p in i420_planes(surfaces))))
        else:
            try:
                surfaces = list(surfaces)
            except TypeError:
                raise ValueError(f"{what}: surfaces must be a sequence of I420 surfaces ([3H/2,W] tensors or triples of planes), a tensor "
                                 f"[N,3H/2,W] or a triple of planes, got {type(surfaces).__name__}") from None
        if not surfaces:
            raise ValueError(f"{what}: a table needs at least one surface")
        planes = []
        for n, s in enumerate(surfaces):
            if s is None:
                planes.append(None)
                continue
            if isinstance(s, torch.Tensor) and s.dim() != 2:
                raise ValueError(f"{what}: surfaces[{n}] must be ONE surface, a uint8 tensor [3H/2,W] or a triple (y [H,W], u [H/2,W/2], "
                                 f"v [H/2,W/2]), got {tuple(s.shape)}")
            try:
                p = i420_planes(s)
            except ValueError as e:
                raise ValueError(f"{what}: surfaces[{n}]: {e}") from None
            if p[0].size(0) != 1:
                raise ValueError(f"{what}: surfaces[{n}] must be ONE surface, got planes of {p[0].size(0)} frames")
            y, u, v = (t[0] for t in p)
            W = y.size(1)
            if any(t.stride(1) != 1 for t in (y, u, v)) or y.stride(0) < W or u.stride(0) < W // 2 or v.stride(0) < W // 2:
                raise ValueError(f"{what}: surfaces[{n}]: the pixel stride of every plane must be 1 and rows must hold W = {W} (Y) and W / 2 "
                                 f"(U, V) bytes, got strides {y.stride()}, {u.stride()} and {v.stride()}")
            planes.append((y, u, v))
        there = [p for p in planes if p is not None]
        if any(not t.is_cuda for p in there for t in p):
            raise L.SpkError(f"{what}: expected uint8 HIP tensors, got a surface on the CPU (no CPU path)")
        if any(p[0].device != there[0][0].device for p in there):
            raise L.SpkError(f"{what}: the surfaces must be on one device, got {sorted({str(p[0].device) for p in there})}")
        self.surfaces, self.planes, self.N = surfaces, planes, len(surfaces)
        self.sizes = [(0, 0) if p is None else tuple(p[0].shape) for p in planes]
        self._host = (L.PlanarRef * self.N)()
        for e, p in zip(self._host, planes):
            if p is not None:
                e.y, e.u, e.v = (t.data_ptr() for t in p)
                e.y_row_stride, e.u_row_stride, e.v_row_stride = (t.stride(0) for t in p)
                e.H, e.W = p[0].shape
        self._checked("spk_planar_table_check", there[0][0].device if there else None)


class _TabledPlanar(_TabledSurfaces):
    """``_Planar`` for a ``PlanarTable``, as ``_TabledSurfaces`` is ``_Surfaces`` for a ``SurfaceTable`` (csrc/frame_table_i420.hip)"""
    noun = "planar table"
    way_in, paste = "spk_frames_i420_to_f32_sim_table", "spk_frames_paste_i420_sim_table"
    sums, match = "spk_paste_colour_sums_i420_sim_table", "spk_paste_colour_match_i420_sim_table"


_TABLED_PLANAR = _TabledPlanar()


def _i420_format(i420):
    return _TABLED_PLANAR if isinstance(i420, PlanarTable) else _PLANAR


def clone_planar(i420):
    """A packed copy of the surfaces to paste into, ``clone_surfaces`` for I420: of a ``PlanarTable`` a new table over one packed
    ``[3H/2, W]`` clone per surface (a table of its own: its host check and, at its first launch, its upload come on top of the
    clones); else one packed ``[N, 3H/2, W]`` tensor"""
    if isinstance(i420, PlanarTable):
        clones = []
        for p in i420.planes:
            if p is None:
                clones.append(None)
                continue
            out, _, fill = _PLANAR.target(tuple(t.unsqueeze(0) for t in p), None, 1, *p[0].shape, p[0].device, "clone_planar")
            fill()
            clones.append(out[0])
        return PlanarTable(clones)
    planes = i420_planes(i420)
    out, _, fill = _PLANAR.target(planes, None, *planes[0].shape, planes[0].device, "clone_planar")
    fill()
    return out


# ---- the axis-aligned edge on I420 surfaces (csrc/frame_i420.hip; the definitions are in include/spk.h) ---------------------------
def frames_from_i420(i420, size, *, crop=None, channel_order="rgb", mean=0.5, std=0.5, standard="bt601", full_range=False):
    """``frames_from_nv12`` for I420 surfaces, one launch (``spk_frames_i420_to_f32``): the same crop, resize, colour maps and
    arguments over three planes, and the same fp32 BITS as that launcher gives on the NV12 surface with the same Y bytes and
    ``UV[cy][cx] = (U[cy][cx], V[cy][cx])``.  ``i420``: what ``i420_planes`` takes -- a contiguous packed ``[N,3H/2,W]`` tensor or a
    triple of plane views of any pitch -- on the device, read in place through its strides; no alignment, parity or order in memory
    is asked of a chroma plane (chroma is loaded as bytes; YV12 is the triple with the planes swapped).  ``crop``: the three forms
    of ``parse_boxes``; an origin may be odd; device origins are clamped by the kernel.  -> float32 [N,3,size,size]."""
    return _from_boxes(_PLANAR, "frames_from_i420", i420, size, crop, channel_order, mean, std, standard, full_range)


def frames_to_i420(x, *, value_range=(-1, 1), standard="bt601", full_range=False, out=None):
    """``frames_to_nv12`` for I420, one launch (``spk_frames_f32_to_i420``): the Y, U and V bytes are those that launcher leaves in
    its Y plane and in the two halves of its UV pairs.  ``out``: what ``i420_planes`` takes, a packed tensor or a triple of planes
    of any pitch (bytes that belong to no plane are not touched).  -> ``out``, or a fresh packed uint8 ``[N, 3H/2, W]`` tensor: the
    ``H`` rows of Y, then the ``HW/4`` bytes of U, then those of V."""
    return _to_surfaces(_PLANAR, "frames_to_i420", x, value_range, standard, full_range, out)


def frames_paste_i420(x, i420, box, *, feather=0, value_range=(-1, 1), standard="bt601", full_range=False, out=None):
    """``frames_paste_nv12`` for I420 surfaces, one launch (``spk_frames_paste_i420``): the same resize, values, ``feather`` and
    blend, luma per pixel and chroma per 2 x 2 block, with a byte load and a byte store per chroma plane; the Y, U and V bytes are
    those the NV12 launcher leaves on the interleaved surface.  ``box``: the three forms of ``parse_boxes``; origins may be odd; box
    pixels outside the frame are skipped.  ``out=None``: the result is ONE packed clone of ``i420`` with every plane copied, the
    input unchanged; ``out=i420`` (the same tensor, or the same triple of planes): pasted in place through its strides; another
    ``out`` first receives a copy.  -> uint8 [N, 3H/2, W], or ``out``."""
    return _paste_boxes(_PLANAR, "frames_paste_i420", x, i420, box, feather, value_range, standard, full_range, out)


def frames_from_i420_aligned(i420, size, sim, *, channel_order="rgb", mean=0.5, std=0.5, standard="bt601", full_range=False):
    """``frames_from_nv12_aligned`` for I420 surfaces, one launch (``spk_frames_i420_to_f32_sim``): the same footprint, weights,
    colour maps and arguments over three planes, and the same fp32 BITS as that launcher gives on the NV12 surface with the same Y
    bytes and ``UV[cy][cx] = (U[cy][cx], V[cy][cx])``.  ``i420``: what ``i420_planes`` takes, on the device, read in place through
    its strides (no alignment or parity is asked of a chroma plane), or a ``PlanarTable``: surfaces of their own sizes in their own
    buffers, still one launch (``spk_frames_i420_to_f32_sim_table``), frame ``n`` bit for bit this call on surface ``n`` alone; an
    absent surface gives ``-mean / std``.  -> float32 [N,3,size,size]."""
    return _from_aligned(_i420_format(i420), "frames_from_i420_aligned", i420, size, sim, channel_order, mean, std, standard=standard, full_range=full_range)


def frames_paste_i420_aligned(x, i420, sim, *, feather=0, value_range=(-1, 1), standard="bt601", full_range=False, out=None, matte=None,
                              colour=None):
    """``frames_paste_nv12_aligned`` for I420 surfaces, one launch (``spk_frames_paste_i420_sim``): the same region, values, ``feather``,
    ``matte`` and ``colour`` rows and the same blend, luma per pixel and chroma per 2 x 2 block, with a byte load and a byte store
    per chroma plane; the Y, U and V bytes are those the NV12 launcher leaves on the interleaved surface.  ``i420``, ``out``: what
    ``i420_planes`` takes (``out=i420``, the same tensor or the same triple of planes, pastes in place; ``out=None``: a packed
    ``[N, 3H/2, W]`` clone).  -> uint8 [N, 3H/2, W], or ``out``.

    ``i420`` may be a ``PlanarTable`` (``spk_frames_paste_i420_sim_table``, one launch): the paste is then IN PLACE, into the table's
    own surfaces (``out``: None or the table), no two planes of which may share a byte range; an absent surface is left alone.
    -> the table."""
    return _paste_aligned(_i420_format(i420), "frames_paste_i420_aligned", x, i420, sim, feather, value_range, out, matte, colour, standard=standard,
                          full_range=full_range)


def paste_colour_match_i420(x, i420, sim, *, matte=None, feather=0, value_range=(-1, 1), standard="bt601", full_range=False, max_gain=2.0,
                            min_sigma=1.0, min_weight=16.0, out=None):
    """``paste_colour_match_nv12`` for an I420 background, two launches (``spk_paste_colour_match_i420_sim``): the same rows, bit
    for bit, as on the interleaved surface.  ``i420`` is only read, and may be a ``PlanarTable``
    (``spk_paste_colour_match_i420_sim_table``; an absent surface gets ``(1, 0)``).  -> device float32 ``[N,3,2]``."""
    what = "paste_colour_match_i420"
    params = _check_match_params(what, max_gain, min_sigma, min_weight)
    return _colour_statistics(_i420_format(i420), params, what, x, i420, sim, matte, feather, value_range, out, standard=standard, full_range=full_range)


def paste_colour_sums_i420(x, i420, sim, *, matte=None, feather=0, value_range=(-1, 1), standard="bt601", full_range=False, out=None):
    """``paste_colour_sums_nv12`` for an I420 background, two launches (``spk_paste_colour_sums_i420_sim``): the same 13 sums per
    frame, bit for bit, so ``colour_rows_from_sums`` and the causal rows serve all three pixel formats.  ``i420`` may be a
    ``PlanarTable`` (``spk_paste_colour_sums_i420_sim_table``; 13 zeros for an absent surface).  -> device float64 ``[N,13]``."""
    return _colour_statistics(_i420_format(i420), None, "paste_colour_sums_i420", x, i420, sim, matte, feather, value_range, out, standard=standard,
                              full_range=full_range)


# ---- RGB32: uint8 [H,W,4] frames, a pixel one aligned 32-bit word (csrc/frame_sim_rgb32.hip, csrc/frame_table_rgb32.hip) -----------
RGB32_ORDERS = {"rgba": ("rgb", 0), "bgra": ("bgr", 0), "argb": ("rgb", 1), "abgr": ("bgr", 1)}


def rgb32_order(channel_order):
    """One of the four orders of an RGB32 pixel -> ``(the order of its colour bytes, "rgb" or "bgr"; alpha_first)``; an ``X`` byte in
    the alpha's place is the same order.  Anything else raises ``ValueError``."""
    if not isinstance(channel_order, str) or channel_order not in RGB32_ORDERS:
        raise ValueError(f"channel_order must be one of {', '.join(repr(o) for o in RGB32_ORDERS)}, got {channel_order!r}")
    return RGB32_ORDERS[channel_order]


def _aligned32(t, row):                                                   # a tensor's base and the strides in front of ``row`` lead to aligned pixels
    return t.data_ptr() % 4 == 0 and all(t.stride(d) % 4 == 0 for d in range(row + 1) if t.size(d) > 1 or d == row)


def rgb32_pixels(frames):
    """uint8 [N,H,W,4] whose pixels are aligned 32-bit words -- ``stride(3) == 1``, ``stride(2) == 4``, a row stride that is a multiple
    of 4 and ``>= 4 W``, a 4-aligned ``data_ptr()`` (with ``N > 1``: a frame stride that is a multiple of 4) -- and whose rows / frames
    do not overlap: what the kernels address by byte strides.  An ``Rgb32Table`` has such pixels by construction: its frames must
    not share bytes (``SpkError`` names the two that do)."""
    if isinstance(frames, Rgb32Table):
        frames.check_written()
        return True
    N, H, W, _ = frames.shape
    return frames.stride(3) == 1 and frames.stride(2) == 4 and frames.stride(1) >= 4 * W and _aligned32(frames, 1) and \
        (N == 1 or frames.stride(0) >= (H - 1) * frames.stride(1) + 4 * W)


class _Packed32(_Packed):
    """``_Packed`` for RGB32 frames, uint8 ``[N,H,W,4]``: the same launchers over the ``_rgb32_sim`` entry points, which take
    ``alpha_first`` behind the channel swap.  Frames that are only read and do not fit are made contiguous; frames that are written
    and do not fit are refused."""
    way_in, paste = "spk_frames_rgb32_to_f32_sim", "spk_frames_paste_rgb32_sim"
    sums, match = "spk_paste_colour_sums_rgb32_sim", "spk_paste_colour_match_rgb32_sim"

    def shaped(self, frames, N, what):                                    # N=None: any number, one frame may come as [H,W,4]; -> (frames, N, H, W)
        if not isinstance(frames, torch.Tensor):
            raise ValueError(f"{what}: frames must be a uint8 tensor [N,H,W,4] or an Rgb32Table, got {type(frames).__name__}")
        if N is None and frames.dim() == 3:
            frames = frames.unsqueeze(0)
        if frames.dim() != 4 or frames.size(3) != 4 or (frames.size(0) < 1 if N is None else frames.size(0) != N):
            raise ValueError(f"{what}: frames must be [{'N' if N is None else N},H,W,4], got {tuple(frames.shape)}")
        return (frames, *frames.shape[:3])

    def read(self, frames, what, disjoint=False):
        self.on_device(frames)
        N, _, W, _ = frames.shape
        if not (rgb32_pixels(frames) if disjoint else frames.stride(3) == 1 and frames.stride(2) == 4 and frames.stride(1) >= 4 * W and
                _aligned32(frames, 1) and (N == 1 or frames.stride(0) >= 0)):
            frames = frames.contiguous()
            if frames.data_ptr() % 4:                                     # (an allocator's block is aligned; a view into one need not be)
                frames = frames.clone(memory_format=torch.contiguous_format)
        return frames, (frames.data_ptr(), frames.stride(0) if N > 1 else 0, frames.stride(1))

    def target(self, frames, out, N, H, W, device, what):
        copy = out is not None and out is not frames and out.data_ptr() != frames.data_ptr()
        if out is None:
            out = frames.clone(memory_format=torch.contiguous_format)
        elif not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != tuple(frames.shape):
            raise L.SpkError(f"out: expected a uint8 HIP tensor {tuple(frames.shape)}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        if not rgb32_pixels(out):
            raise L.SpkError(f"out: pixels must be aligned 32-bit words (strides (4 k, 4 k >= 4 W, 4, 1), a data pointer that is a multiple of "
                             f"4) and rows / frames must not overlap, got strides {out.stride()} at {out.data_ptr():#x}")
        return out, (out.data_ptr(), out.stride(0) if N > 1 else 0, out.stride(1)), (lambda: out.copy_(frames)) if copy else (lambda: None)

    def standard(self, alpha_first=0):
        return (alpha_first,)

    def quantised(self, value_range, channel_order="rgb", alpha_first=0):
        return ((_channel_swap(channel_order), alpha_first), *quant_range(value_range))


_PACKED32 = _Packed32()


class Rgb32Table(_DeviceTable):
    """``FrameTable`` for RGB32 frames: ``N`` uint8 frames ``[H_n,W_n,4]`` that share neither an allocation nor a size, as the aligned
    RGB32 launchers address them -- a device table of the same 24-byte ``spk_frame_ref`` entries ``(data, row_stride, H, W)``.
    ``frames``: a sequence of device uint8 tensors ``[H_n,W_n,4]`` on one device, each with ``stride(2) == 1``, ``stride(1) == 4``, a
    ``stride(0)`` that is a multiple of 4 and ``>= 4 W_n`` and a 4-aligned ``data_ptr()`` -- a region-of-interest view at any pixel
    offset of a wider surface is fine -- with ``None`` for a frame that is ABSENT (an all-zero entry: the launchers treat it like an
    invalid transform); or one ``[N,H,W,4]`` tensor, which gives views of its frames.  Wrong types, shapes or strides raise
    ``ValueError`` before a device is touched; CPU tensors raise ``SpkError`` (no CPU path).  The host table is checked
    (``spk_frame_table_check_rgb32``) here and uploaded ONCE, one host -> device copy of ``24 N`` bytes on the current stream, when a
    launcher first uses the table; whether the frames may be written is decided where the table is used (``check_written``: the
    paste).  The table HOLDS REFERENCES to the tensors.

    ``dev``: the device table (uint8 ``[24 N]``); ``sizes``: ``(H, W)`` per frame (``(0, 0)``: absent); ``frames``: the tensors."""

    def __init__(self, frames):
        what = "Rgb32Table"
        if isinstance(frames, torch.Tensor):
            if frames.dim() != 4 or frames.size(0) < 1:
                raise ValueError(f"{what}: a tensor of frames must be [N,H,W,4], got {tuple(frames.shape)}")
            frames = list(frames.unbind(0))
        else:
            try:
                frames = list(frames)
            except TypeError:
                raise ValueError(f"{what}: frames must be a sequence of uint8 tensors [H,W,4] or a tensor [N,H,W,4], got "
                                 f"{type(frames).__name__}") from None
        if not frames:
            raise ValueError(f"{what}: a table needs at least one frame")
        for n, f in enumerate(frames):
            if f is None:
                continue
            if not isinstance(f, torch.Tensor):
                raise ValueError(f"{what}: frames[{n}] must be a uint8 tensor [H,W,4] or None, got {type(f).__name__}")
            if f.dtype != torch.uint8 or f.dim() != 3 or f.size(2) != 4 or f.size(0) < 1 or f.size(1) < 1:
                raise ValueError(f"{what}: frames[{n}] must be a uint8 tensor [H,W,4] with H, W >= 1, got {f.dtype} {tuple(f.shape)}")
            if f.stride(2) != 1 or f.stride(1) != 4 or f.stride(0) < 4 * f.size(1) or f.stride(0) % 4:
                raise ValueError(f"{what}: frames[{n}]: pixels must be 4 bytes apart and rows a multiple of 4 bytes apart that do not overlap "
                                 f"(strides (4 k >= {4 * f.size(1)}, 4, 1)), got {f.stride()}")
            if f.data_ptr() % 4:
                raise ValueError(f"{what}: frames[{n}]: the first pixel must be aligned to 4 bytes, got data_ptr() = {f.data_ptr():#x}")
        there = [f for f in frames if f is not None]
        if any(not f.is_cuda for f in there):
            raise L.SpkError(f"{what}: expected uint8 HIP tensors, got a frame on the CPU (no CPU path)")
        if any(f.device != there[0].device for f in there):
            raise L.SpkError(f"{what}: the frames must be on one device, got {sorted({str(f.device) for f in there})}")
        self.frames, self.N = frames, len(frames)
        self.sizes = [(0, 0) if f is None else (f.size(0), f.size(1)) for f in frames]
        self._host = (L.FrameRef * self.N)()
        for e, f in zip(self._host, frames):
            if f is not None:
                e.data, e.row_stride, e.H, e.W = f.data_ptr(), f.stride(0), f.size(0), f.size(1)
        self._checked("spk_frame_table_check_rgb32", there[0].device if there else None)


class _Tabled32(_Tabled):
    """``_Packed32`` for an ``Rgb32Table`` (csrc/frame_table_rgb32.hip)"""
    noun = "RGB32 table"
    way_in, paste = "spk_frames_rgb32_to_f32_sim_table", "spk_frames_paste_rgb32_sim_table"
    sums, match = "spk_paste_colour_sums_rgb32_sim_table", "spk_paste_colour_match_rgb32_sim_table"

    def standard(self, alpha_first=0):
        return (alpha_first,)

    def quantised(self, value_range, channel_order="rgb", alpha_first=0):
        return _PACKED32.quantised(value_range, channel_order, alpha_first)


_TABLED32 = _Tabled32()


def _rgb32_format(frames):
    return _TABLED32 if isinstance(frames, Rgb32Table) else _PACKED32


def clone_rgb32(frames):
    """A contiguous copy of the RGB32 frames to paste into, ``clone_frames`` for ``[.,.,.,4]``: one clone of a tensor; of an
    ``Rgb32Table`` a new table over one clone per frame"""
    if isinstance(frames, Rgb32Table):
        return Rgb32Table([None if f is None else f.clone(memory_format=torch.contiguous_format) for f in frames.frames])
    return frames.clone(memory_format=torch.contiguous_format)


def frames_from_rgb32_aligned(frames, size, sim, *, channel_order="rgba", mean=0.5, std=0.5):
    """``frames_from_u8_aligned`` for RGB32 frames, one launch (``spk_frames_rgb32_to_f32_sim``): the same footprint, weights and
    arguments, a tap one aligned 32-bit load, and the fp32 BITS that launcher gives on a packed copy of the colour bytes.
    ``frames``: uint8 ``[N,H,W,4]`` (one frame: ``[H,W,4]``) on the device, read in place through its strides when its pixels are
    aligned words (``rgb32_pixels`` without the overlap rule; a region-of-interest view at any pixel offset is), else through a
    contiguous copy.  ``channel_order``: ``"rgba"``, ``"bgra"``, ``"argb"`` or ``"abgr"``, the bytes of a pixel in memory order (an
    ``X`` byte counts as the ``a``; it is never interpreted); the network gets R, G, B planes.  ``frames`` may be an ``Rgb32Table``:
    frames of their own sizes in their own buffers, still one launch (``spk_frames_rgb32_to_f32_sim_table``), frame ``n`` bit for bit
    this call on frame ``n`` alone; an absent frame gives ``-mean / std``.  -> float32 [N,3,size,size]."""
    order, alpha_first = rgb32_order(channel_order)
    return _from_aligned(_rgb32_format(frames), "frames_from_rgb32_aligned", frames, size, sim, order, mean, std, alpha_first=alpha_first)


def frames_paste_rgb32_aligned(x, frames, sim, *, feather=0, value_range=(-1, 1), channel_order="rgba", out=None, matte=None, colour=None):
    """``frames_paste_u8_aligned`` for RGB32 frames, one launch (``spk_frames_paste_rgb32_sim``, with ``matte`` / ``colour``
    ``spk_frames_paste_rgb32_sim_blend``): the same region, values, ``feather``, ``matte`` and ``colour`` rows and the same blend; a
    pasted pixel is one 32-bit load and one 32-bit store, its colour bytes those the packed launcher leaves on a packed copy, ITS
    FOURTH BYTE AS IT WAS.  ``out=None``: a contiguous clone of ``frames`` (alpha included) is pasted into; ``out=frames``: in place;
    another ``out`` first receives a copy.  Frames that are written must have aligned pixels and must not overlap
    (``rgb32_pixels``), else ``SpkError``.  -> uint8 [N,H,W,4].

    ``frames`` may be an ``Rgb32Table`` (``spk_frames_paste_rgb32_sim_table``, one launch): the paste is then IN PLACE, into the
    table's own frames (``out``: None or the table), which must not share bytes; an absent frame is left alone.  -> the table."""
    order, alpha_first = rgb32_order(channel_order)
    return _paste_aligned(_rgb32_format(frames), "frames_paste_rgb32_aligned", x, frames, sim, feather, value_range, out, matte, colour,
                          channel_order=order, alpha_first=alpha_first)


def paste_colour_match_rgb32(x, frames, sim, *, matte=None, feather=0, value_range=(-1, 1), channel_order="rgba", max_gain=2.0, min_sigma=1.0,
                             min_weight=16.0, out=None):
    """``paste_colour_match`` for an RGB32 background, two launches (``spk_paste_colour_match_rgb32_sim``): the same rows, bit for
    bit, as on a packed copy of the colour bytes.  ``frames`` is only read, and may be an ``Rgb32Table``
    (``spk_paste_colour_match_rgb32_sim_table``; an absent frame gets ``(1, 0)``).  -> device float32 ``[N,3,2]``."""
    what = "paste_colour_match_rgb32"
    order, alpha_first = rgb32_order(channel_order)
    params = _check_match_params(what, max_gain, min_sigma, min_weight)
    return _colour_statistics(_rgb32_format(frames), params, what, x, frames, sim, matte, feather, value_range, out, channel_order=order,
                              alpha_first=alpha_first)


def paste_colour_sums_rgb32(x, frames, sim, *, matte=None, feather=0, value_range=(-1, 1), channel_order="rgba", out=None):
    """``paste_colour_sums`` for an RGB32 background, two launches (``spk_paste_colour_sums_rgb32_sim``): the same 13 sums per frame,
    bit for bit, so ``colour_rows_from_sums`` and the causal rows serve every pixel format.  ``frames`` may be an ``Rgb32Table``
    (``spk_paste_colour_sums_rgb32_sim_table``; 13 zeros for an absent frame).  -> device float64 ``[N,13]``."""
    order, alpha_first = rgb32_order(channel_order)
    return _colour_statistics(_rgb32_format(frames), None, "paste_colour_sums_rgb32", x, frames, sim, matte, feather, value_range, out,
                              channel_order=order, alpha_first=alpha_first)


# ---- RGB32, axis-aligned: boxes in, a paste, whole frames out (csrc/frame_rgb32.hip) -------------------------------------------------
def frames_from_rgb32(frames, size, *, crop=None, channel_order="rgba", mean=0.5, std=0.5):
    """``frames_from_u8`` for RGB32 frames, one launch (``spk_frames_rgb32_to_f32``; per-frame or device boxes:
    ``spk_frames_rgb32_to_f32_boxes``): the same crop, tables, normalisation and arguments, a tap one aligned 32-bit load, and the
    fp32 BITS that launcher gives on a packed copy of the colour bytes.  ``frames``: uint8 ``[N,H,W,4]`` (one frame: ``[H,W,4]``) on
    the device, read in place through its strides when its pixels are aligned words (a region-of-interest view at any pixel offset
    is), else through a contiguous copy.  ``channel_order``: ``"rgba"``, ``"bgra"``, ``"argb"`` or ``"abgr"`` (``rgb32_order``); the
    network gets R, G, B planes and the fourth byte is never interpreted.  ``crop``: the three forms of ``frames_from_u8``.
    -> float32 [N,3,size,size]."""
    what = "frames_from_rgb32"
    frames, N, H, W = _PACKED32.shaped(frames, None, what)
    Hout, Wout = _out_size(size, what)
    order, alpha_first = rgb32_order(channel_order)
    swap = _channel_swap(order)
    scale, shift = _affine(mean, std, what)
    origins = None
    if crop is not None:
        origins, h, w = parse_boxes(crop, N, H, W, f"{what}: crop")
        if isinstance(origins, tuple):                                # one host box: a slice, read in place through its strides
            (y0, x0), origins = origins, None
            frames = frames[:, y0:y0 + h, x0:x0 + w]
    frames, where = _PACKED32.read(frames, what)
    _, Hin, Win, _ = frames.shape
    out = torch.empty((N, 3, Hout, Wout), device=frames.device, dtype=torch.float32)
    entry, src = "spk_frames_rgb32_to_f32", (*where, N, Hin, Win)
    if origins is not None:                                               # the box is h x w of the frame, else the (sliced) frame itself
        entry, src = entry + "_boxes", (*src, _origins(origins, frames.device, what)[2].data_ptr(), h, w)
        Hin, Win = h, w
    L.check(getattr(L.lib(), entry)(*src, swap, alpha_first, *_table_args(_device_tables(frames.device, Hin, Win, Hout, Wout)), out.data_ptr(),
                                    Hout, Wout, *scale, *shift, L.stream_ptr()), entry)
    return out


def rgb32_alpha(alpha, what):
    """The fourth byte of the way out: an integer ``0 .. 255``, or None for "keep what is there" -> the entry point's ``alpha``
    (``-1``: keep).  Anything else raises ``ValueError``."""
    if alpha is None:
        return -1
    if isinstance(alpha, bool) or not isinstance(alpha, int) or not 0 <= alpha <= 255:
        raise ValueError(f"{what}: alpha must be an integer 0 .. 255, or None to keep the fourth bytes of out, got {alpha!r}")
    return alpha


def frames_to_rgb32(x, *, value_range=(-1, 1), channel_order="rgba", alpha=255, out=None):
    """``frames_to_u8`` for RGB32 frames, one launch (``spk_frames_f32_to_rgb32``): float32 [N,3,H,W] in ``value_range`` -> uint8
    ``[N,H,W,4]`` in ``channel_order`` (``rgb32_order``), the colour bytes those of ``frames_to_u8`` bit for bit (ties to even; NaN
    -> 0), the fourth byte of every pixel ``alpha`` (0 .. 255).  ``out``: a uint8 tensor ``[N,H,W,4]`` to write through its strides --
    a region-of-interest view of a wider texture is written directly; its pixels must be aligned words and its rows / frames must
    not overlap (``rgb32_pixels``), else ``SpkError``.  ``alpha=None`` (needs ``out=``): KEEP -- the fourth bytes already in ``out``
    stay.  Without ``out=`` the result is a new contiguous tensor."""
    what = "frames_to_rgb32"
    _check_chw(x, what)
    order, alpha_first = rgb32_order(channel_order)
    (swap, alpha_first), lo, k = _PACKED32.quantised(value_range, order, alpha_first)
    a = rgb32_alpha(alpha, what)
    if a < 0 and out is None:
        raise ValueError(f"{what}: alpha=None keeps the fourth bytes of out, and there is no out=")
    N, _, H, W = x.shape
    xp = L.dptr(x, "x")
    if out is None:
        out = torch.empty((N, H, W, 4), device=x.device, dtype=torch.uint8)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != (N, H, W, 4):
        got = f"{out.dtype} {tuple(out.shape)} on {out.device}" if isinstance(out, torch.Tensor) else type(out).__name__
        raise L.SpkError(f"out: expected a uint8 HIP tensor {(N, H, W, 4)}, got {got}")
    elif not rgb32_pixels(out):
        raise L.SpkError(f"out: pixels must be aligned 32-bit words (strides (4 k, 4 k >= 4 W, 4, 1), a data pointer that is a multiple of "
                         f"4) and rows / frames must not overlap, got strides {out.stride()} at {out.data_ptr():#x}")
    L.check(L.lib().spk_frames_f32_to_rgb32(xp, out.data_ptr(), out.stride(0) if N > 1 else 0, out.stride(1), N, H, W, swap, alpha_first, a, lo, k,
                                            L.stream_ptr()), "spk_frames_f32_to_rgb32")
    return out


def frames_paste_rgb32(x, frames, box, *, feather=0, value_range=(-1, 1), channel_order="rgba", out=None):
    """``frames_paste_u8`` for RGB32 frames, one launch (``spk_frames_paste_rgb32``): the same resize, quantisation, ``feather`` and
    blend inside the same box (its three forms; box pixels outside the frame are skipped); a pasted pixel is one 32-bit load and one
    32-bit store, its colour bytes those the packed launcher leaves on a packed copy, ITS FOURTH BYTE AS IT WAS.  ``out=None``: a
    contiguous clone of ``frames`` (alpha included) is pasted into; ``out=frames``: in place through its strides; another ``out``
    first receives a copy.  Frames that are written must have aligned pixels and must not overlap (``rgb32_pixels``), else
    ``SpkError``.  -> uint8 [N,H,W,4]."""
    what = "frames_paste_rgb32"
    _check_chw(x, what)
    N, _, Hs, Ws = x.shape
    frames, _, H, W = _PACKED32.shaped(frames, N, what)
    order, alpha_first = rgb32_order(channel_order)
    (swap, alpha_first), lo, k = _PACKED32.quantised(value_range, order, alpha_first)
    feather = check_feather(feather, what)
    origins, h, w = parse_boxes(box, N, H, W, f"{what}: box", inside=False)
    xp = L.dptr(x, "x")
    _PACKED32.on_device(frames)
    out, where, fill = _PACKED32.target(frames, out, N, H, W, x.device, what)
    y0, x0, boxes = _origins(origins, x.device, what)
    fill()
    tables, ay, ax = _paste_tables(Hs, Ws, h, w, feather, x.device)
    L.check(L.lib().spk_frames_paste_rgb32(xp, N, Hs, Ws, *where, H, W, h, w, y0, x0, _ptr(boxes), swap, alpha_first, *tables, ay, ax, lo, k,
                                           L.stream_ptr()), "spk_frames_paste_rgb32")
    return out


def generated_row_scale(size, Ws, device):
    """The network image has ``size`` pixels where a generated one is ``Ws`` wide: -> the factor of a row ``(a, c, tx, ty)`` that maps
    the generated image into the frames, a float32 ``[4]`` tensor on ``device`` made in fp32, or None when it is 1"""
    k = size[1] / Ws
    return None if k == 1 else torch.tensor([k, k, 1.0, 1.0], dtype=torch.float32).to(device)


def chunk_matte(matte, t0, t1):                                           # a clip's matte for frames [t0, t1): a per-frame one is sliced
    return matte[t0:t1] if matte is not None and matte.dim() == 3 else matte


class Aligned:
    """``IRFD.reenact_video(align=...)``: the transforms of a clip, standing where a crop box would.  ``rows``: float32 ``[T,4]``
    where the frames are; ``size``: ``(H, W)`` of the network image the rows map into the frames."""

    def __init__(self, rows, size):
        self.rows, self.size, self._generated = rows, size, {}

    @classmethod
    def parse(cls, sim, T, size, device, what="reenact_video: align"):    # host rows: checked here, uploaded once for both edges
        rows = sim.rows(T, what) if isinstance(sim, LandmarkAlign) else parse_sim(sim, T, what)      # landmarks: fitted once per clip
        if not rows.is_cuda and device.type == "cuda":
            rows = rows.to(device)
        return cls(rows, _out_size(size, "reenact_video"))

    def chunk(self, t0, t1, y):
        """The transforms of frames ``[t0, t1)`` for pasting their generated images ``y`` [n,3,Hs,Ws]: the network image has
        ``size`` pixels where ``y`` has ``Hs x Ws``, so ``(a, c)`` are scaled by ``size / Ws`` (once per clip, in fp32)."""
        Hs, Ws = y.shape[2:]
        if Hs * self.size[1] != Ws * self.size[0]:
            raise ValueError(f"reenact_video: align needs generated frames in the shape of the network input, got {Hs} x {Ws} for {self.size}")
        if Ws not in self._generated:
            scale = generated_row_scale(self.size, Ws, self.rows.device)
            self._generated[Ws] = self.rows if scale is None else self.rows * scale
        return Aligned(self._generated[Ws][t0:t1], (Hs, Ws))


# ---- what IRFD.reenact_video asks of a pixel format -------------------------------------------------------------------------------
class Rgb24:
    """Packed uint8 frames ``[T,H,W,3]`` in ``channel_order``."""
    output, needs_box = "uint8", False        # reenact(output=...) without a paste; crop=None goes to the launcher as it is

    def __init__(self, channel_order, standard, full_range):
        self.args = dict(channel_order=channel_order)                     # what the launchers and reenact(output=...) take

    def open(self, frames, inplace):
        """-> (what the methods below take, its device, T, H, W); ``inplace``: the frames can be pasted into"""
        if frames.dim() != 4 or frames.size(3) != 3 or frames.size(0) < 1:
            raise ValueError(f"reenact_video: pose_u8 must be [T,H,W,3], got {tuple(frames.shape)}")
        if inplace and not packed_pixels(frames):
            raise L.SpkError(f"reenact_video: inplace needs packed pixels and rows / frames that do not overlap, got strides {frames.stride()}")
        return (frames, frames.device, *frames.shape[:3])

    def network_input(self, frames, size, crop):                          # ``crop``: a box in a launcher's forms, or ``Aligned``
        if isinstance(crop, Aligned):
            return frames_from_u8_aligned(frames, size, crop.rows, **self.args)
        return frames_from_u8(frames, size, crop=crop, **self.args)

    def clone(self, frames):                                              # -> (the result, what ``paste`` takes)
        return (frames.clone(memory_format=torch.contiguous_format),) * 2

    def paste(self, y, frames, t0, t1, box, feather, matte=None, colour_match=False):    # ``box``: a box, or what ``Aligned.chunk`` gave
        if isinstance(box, Aligned):
            blend = {}
            if matte is not None or colour_match:                         # the statistics read the background before the paste writes it
                matte = chunk_matte(matte, t0, t1)
                rows = paste_colour_match(y, frames[t0:t1], box.rows, matte=matte, feather=feather, **self.args) if colour_match else None
                blend = dict(matte=matte, colour=rows)
            frames_paste_u8_aligned(y, frames[t0:t1], box.rows, feather=feather, out=frames[t0:t1], **self.args, **blend)
        else:
            frames_paste_u8(y, frames[t0:t1], box, feather=feather, out=frames[t0:t1], **self.args)

    # colour_smooth > 0: the statistics of a chunk now, its paste once the sums of its whole window exist (``box``: an ``Aligned``)
    def colour_sums(self, y, frames, t0, t1, box, feather, matte, sums):
        paste_colour_sums(y, frames[t0:t1], box.rows, matte=chunk_matte(matte, t0, t1), feather=feather, out=sums[t0:t1], **self.args)

    def paste_matched(self, y, frames, t0, t1, box, feather, matte, colour):
        frames_paste_u8_aligned(y, frames[t0:t1], box.rows, feather=feather, out=frames[t0:t1], matte=chunk_matte(matte, t0, t1), colour=colour,
                                **self.args)


class Rgb32(Rgb24):
    """RGB32 frames ``[T,H,W,4]`` in one of the four orders of ``rgb32_order``: ``Rgb24`` over the RGB32 launchers.  The fourth byte
    of a frame that is pasted into stays; a generated frame gets 255."""
    output = "rgb32"

    def __init__(self, channel_order, standard, full_range):
        rgb32_order(channel_order)                                        # one of the four, or ValueError: before anything else
        self.args = dict(channel_order=channel_order)

    def open(self, frames, inplace):
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.size(3) != 4 or frames.size(0) < 1:
            got = tuple(frames.shape) if isinstance(frames, torch.Tensor) else type(frames).__name__
            raise ValueError(f"reenact_video: pose_u8 must be [T,H,W,4] with pixel_format='rgb32', got {got}")
        if inplace and not rgb32_pixels(frames):
            raise L.SpkError(f"reenact_video: inplace needs pixels that are aligned 32-bit words (strides (4 k, 4 k >= 4 W, 4, 1), a data pointer "
                             f"that is a multiple of 4) and rows / frames that do not overlap, got strides {frames.stride()} at "
                             f"{frames.data_ptr():#x}")
        return (frames, frames.device, *frames.shape[:3])

    def network_input(self, frames, size, crop):
        if isinstance(crop, Aligned):
            return frames_from_rgb32_aligned(frames, size, crop.rows, **self.args)
        return frames_from_rgb32(frames, size, crop=crop, **self.args)

    def clone(self, frames):
        return (clone_rgb32(frames),) * 2

    def paste(self, y, frames, t0, t1, box, feather, matte=None, colour_match=False):
        if isinstance(box, Aligned):
            blend = {}
            if matte is not None or colour_match:                         # the statistics read the background before the paste writes it
                matte = chunk_matte(matte, t0, t1)
                rows = paste_colour_match_rgb32(y, frames[t0:t1], box.rows, matte=matte, feather=feather, **self.args) if colour_match else None
                blend = dict(matte=matte, colour=rows)
            frames_paste_rgb32_aligned(y, frames[t0:t1], box.rows, feather=feather, out=frames[t0:t1], **self.args, **blend)
        else:
            frames_paste_rgb32(y, frames[t0:t1], box, feather=feather, out=frames[t0:t1], **self.args)

    def colour_sums(self, y, frames, t0, t1, box, feather, matte, sums):
        paste_colour_sums_rgb32(y, frames[t0:t1], box.rows, matte=chunk_matte(matte, t0, t1), feather=feather, out=sums[t0:t1], **self.args)

    def paste_matched(self, y, frames, t0, t1, box, feather, matte, colour):
        frames_paste_rgb32_aligned(y, frames[t0:t1], box.rows, feather=feather, out=frames[t0:t1], matte=chunk_matte(matte, t0, t1), colour=colour,
                                   **self.args)


class Nv12:
    """NV12 surfaces: what ``nv12_planes`` takes, in the colour of ``standard`` / ``full_range``."""
    output, needs_box = "nv12", True

    def __init__(self, channel_order, standard, full_range):
        self.args = dict(standard=standard, full_range=full_range)

    def open(self, frames, inplace):
        planes = nv12_planes(frames)
        if inplace:
            nv12_strides(*planes, "reenact_video: inplace", written=True)
        return (planes, planes[0].device, *planes[0].shape)

    def network_input(self, frames, size, crop):
        return frames_from_nv12(frames, size, crop=crop, **self.args)

    def clone(self, planes):                                              # one clone: a packed surface per frame
        out, _, fill = _SURFACES.target(planes, None, *planes[0].shape, planes[0].device, "reenact_video")
        fill()
        return out, nv12_planes(out)

    def paste(self, y, planes, t0, t1, box, feather):
        part = (planes[0][t0:t1], planes[1][t0:t1])
        frames_paste_nv12(y, part, box, feather=feather, out=part, **self.args)


class I420(Nv12):
    """I420 surfaces: what ``i420_planes`` takes, in the colour of ``standard`` / ``full_range``."""
    output = "i420"

    def open(self, frames, inplace):
        planes = i420_planes(frames)
        if inplace:
            i420_strides(*planes, "reenact_video: inplace", written=True)
        return (planes, planes[0].device, *planes[0].shape)

    def network_input(self, frames, size, crop):
        return frames_from_i420(frames, size, crop=crop, **self.args)

    def clone(self, planes):                                              # one clone: a packed surface per frame
        out = clone_planar(planes)
        return out, i420_planes(out)

    def paste(self, y, planes, t0, t1, box, feather):
        part = tuple(p[t0:t1] for p in planes)
        frames_paste_i420(y, part, box, feather=feather, out=part, **self.args)


PIXEL_FORMATS = {"rgb24": Rgb24, "nv12": Nv12, "i420": I420, "rgb32": Rgb32}
