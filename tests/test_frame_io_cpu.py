"""CPU-side checks of the video-frame edge: the host-built resize tables (``ops.resize_tables``, ``spk_resize_table``) against
torch's own fp64 ``interpolate(mode="bilinear", antialias=True)``, the fp32 rows the kernel reads, the new launch-list kind on both
sides of the C boundary, and the argument errors of the launchers and entry points (raised without a device)."""
import importlib
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n_in, n_out): down by a non-integer factor with windows cut at both ends; up (at most two taps); identity; the smallest sizes
SIZES = [(37, 16), (53, 16), (135, 32), (240, 32), (20, 32), (28, 32), (32, 32), (7, 7), (2, 1), (1, 4)]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")


def dense(first, count, w, n_in):
    """The [n_out, n_in] matrix a table stands for."""
    m = torch.zeros(first.numel(), n_in, dtype=torch.float64)
    for o in range(first.numel()):
        m[o, int(first[o]):int(first[o]) + int(count[o])] = w[o, :int(count[o])].double()
    return m


@pytest.mark.parametrize("n_in,n_out", SIZES)
def test_resize_tables_equal_torch_fp64_interpolate(pkg, n_in, n_out):
    first, count, w = pkg.ops.resize_tables(n_in, n_out)
    assert first.dtype == torch.int32 and count.dtype == torch.int32 and w.dtype == torch.float64
    assert first.shape == (n_out,) and count.shape == (n_out,) and w.shape == (n_out, int(count.max()))
    assert int(count.min()) >= 1 and int(first.min()) >= 0 and int((first + count).max()) <= n_in
    for o in range(n_out):
        assert torch.all(w[o, int(count[o]):] == 0)                       # zero padded
    g = torch.Generator().manual_seed(n_in * 1000 + n_out)
    x = torch.rand(2, 3, n_in, 5, generator=g, dtype=torch.float64) * 255
    got = torch.einsum("oi,bciw->bcow", dense(first, count, w, n_in), x)
    ref = F.interpolate(x, size=(n_out, 5), mode="bilinear", align_corners=False, antialias=True)
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"resize_tables {n_in} -> {n_out}: taps {w.shape[1]}, max error relative to the largest value {err:.3e}")
    assert err <= 1e-12
    # the other axis of the same call (torch's filter is separable)
    xt = x.transpose(2, 3).contiguous()
    got_t = torch.einsum("oi,bchi->bcho", dense(first, count, w, n_in), xt)
    ref_t = F.interpolate(xt, size=(5, n_out), mode="bilinear", align_corners=False, antialias=True)
    assert float((got_t - ref_t).abs().max() / ref_t.abs().max()) <= 1e-12
    if n_in == n_out:
        assert torch.all(count == 1) and torch.equal(first, torch.arange(n_in, dtype=torch.int32)) and torch.all(w == 1)
    if n_out > n_in:
        assert int(count.max()) <= 2


@pytest.mark.parametrize("n_in,n_out", SIZES + [(1080, 256), (1920, 256)])
def test_fp32_rows_sum_to_one(pkg, n_in, n_out):
    first, count, w = pkg.ops.resize_tables(n_in, n_out)
    assert float((w.float().double().sum(1) - 1).abs().max()) <= 1e-6          # plain rounding of the fp64 table
    f32, c32, w32 = pkg.ops.resize_tables_f32(n_in, n_out)
    assert w32.dtype == torch.float32 and torch.equal(f32, first) and torch.equal(c32, count) and w32.shape == w.shape
    dev = float((w32.double().sum(1) - 1).abs().max())
    moved = float(((w32.double() - w) .abs() / w.clamp_min(1e-300)).max())
    print(f"fp32 table {n_in} -> {n_out}: |row sum - 1| <= {dev:.3e}, largest relative move of a weight {moved:.3e}")
    assert dev <= 1e-6 and int((first + count).max()) <= n_in
    assert dev == 0.0                                                     # the kernel's rows are an exact partition of unity
    # and still the fp64 weights to fp32 accuracy: a rounding errs by at most 2^-25 (weights < 1), so the residual the
    # rows absorb is at most taps * 2^-25 and no weight ends further from its fp64 value than that plus its own rounding
    assert float((w32.double() - w).abs().max()) <= (w.shape[1] + 1) * 2.0 ** -25
    assert torch.all(w32 >= 0)


def test_table_argument_errors(pkg):
    lib = pkg._lib.lib()
    assert lib.spk_resize_table_taps(0, 4) < 0 and lib.spk_resize_table_taps(4, 0) < 0
    assert lib.spk_resize_table_taps(32, 32) == 1 and lib.spk_resize_table_taps(20, 32) == 2
    first, count = torch.empty(4, dtype=torch.int32), torch.empty(4, dtype=torch.int32)
    w = torch.empty(4, 8, dtype=torch.float64)
    assert lib.spk_resize_table(16, 4, 8, None, count.data_ptr(), w.data_ptr(), None) < 0 and b"null" in lib.spk_last_error()
    assert lib.spk_resize_table(16, 4, 8, first.data_ptr(), count.data_ptr(), None, None) < 0
    assert lib.spk_resize_table(16, 4, 2, first.data_ptr(), count.data_ptr(), w.data_ptr(), None) < 0 and b"taps" in lib.spk_last_error()
    assert lib.spk_resize_table(16, 4, 8, first.data_ptr(), count.data_ptr(), w.data_ptr(), None) == 0
    with pytest.raises(ValueError):
        pkg.ops.resize_tables(0, 3)


def test_kernel_argument_errors_need_no_device(pkg):
    """Every refusal of the two entry points happens before a launch: a negative code and a message, on a machine without a GPU."""
    lib = pkg._lib.lib()
    p = 4096                     # any non-null address: the arguments are refused before anything is read or launched

    def to_f32(src=p, dst=p, tab=p, N=1, Hin=4, Win=4, row=12, taps=2, Hout=2, Wout=2):
        return lib.spk_frames_u8_to_f32(src, Hin * row, row, N, Hin, Win, 0, tab, tab, tab, taps, tab, tab, tab, taps, dst, Hout, Wout,
                                        1.0, 1.0, 1.0, 0.0, 0.0, 0.0, None)

    for bad in (dict(src=None), dict(dst=None), dict(tab=None), dict(N=0), dict(Hin=0), dict(Win=0), dict(Hout=0), dict(Wout=0),
                dict(taps=0), dict(row=11)):
        assert to_f32(**bad) == -1, bad
        assert lib.spk_last_error()
    assert b"row stride" in lib.spk_last_error()
    for bad in ((None, p, 1, 4, 4), (p, None, 1, 4, 4), (p, p, 0, 4, 4), (p, p, 1, 0, 4), (p, p, 1, 4, 0)):
        assert lib.spk_frames_f32_to_u8(bad[0], bad[1], bad[2], bad[3], bad[4], 0, -1.0, 127.5, None) == -1, bad
    assert lib.spk_frames_f32_to_u8(p, p, 1, 4, 4, 0, -1.0, 0.0, None) == -1


def test_launchers_refuse_cpu_tensors_and_bad_arguments(pkg):
    ops, SpkError = pkg.ops, pkg._lib.SpkError
    u8 = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_from_u8(u8, 4)
    with pytest.raises(SpkError, match="uint8"):
        ops.frames_from_u8(u8.float(), 4)
    with pytest.raises(ValueError):
        ops.frames_from_u8(torch.zeros(2, 3, 8, 8, dtype=torch.uint8), 4)          # CHW is not a frame layout
    with pytest.raises(ValueError):
        ops.frames_from_u8(u8, 4, channel_order="gbr")
    with pytest.raises(ValueError):
        ops.frames_from_u8(u8, 4, crop=(4, 4, 8, 2))                               # the box leaves the frame
    with pytest.raises(ValueError):
        ops.frames_from_u8(u8, 4, std=(0.5, 0.0, 0.5))
    with pytest.raises(ValueError):
        ops.frames_from_u8(u8, 0)
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(SpkError, match="HIP|device|CPU"):
        ops.frames_to_u8(x)
    with pytest.raises(ValueError):
        ops.frames_to_u8(torch.zeros(2, 8, 8, 3))
    with pytest.raises(ValueError):
        ops.frames_to_u8(x, value_range=(1, 1))
    with pytest.raises(ValueError):
        ops.frames_to_u8(x, channel_order="bgra")
    assert ops.quant_range((-1, 1)) == (-1.0, 127.5) and ops.quant_range((0, 1)) == (0.0, 255.0)


def test_header_and_ctypes_agree_on_the_frame_op(pkg):
    L = pkg._lib
    src = open(os.path.join(ROOT, "include", "spk.h")).read()
    kinds = dict((n, int(v)) for n, v in re.findall(r"(SPK_OP_[A-Z0-9_]+)\s*=\s*(\d+)", src))
    assert kinds["SPK_OP_FRAMES_TO_U8"] == L.OP_FRAMES_TO_U8 == 11 and sorted(kinds.values()) == list(range(1, 12))
    body = re.search(r"typedef struct spk_frames_to_u8_args \{(.*?)\} spk_frames_to_u8_args;", src, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*(?:,|;)", body)
    assert names == [f[0] for f in L.FramesToU8Args._fields_] == ["x", "y", "N", "H", "W", "swap_rb", "lo", "k"]
    assert L.FramesToU8Args.N.offset == 16 and L.FramesToU8Args.k.offset == 36
    launch = open(os.path.join(ROOT, "speak-hack_amd", "csrc", "launch_list.hip")).read()
    assert "case SPK_OP_FRAMES_TO_U8" in launch


def test_reenact_video_and_output_argument_errors(pkg):
    import model
    m = model.IRFD()
    assert callable(m.reenact_video) and model.IRFD.reenact_video is importlib.import_module("speak-hack_amd.irfd").IRFD.reenact_video
    img, frames = torch.zeros(1, 3, 64, 64), torch.zeros(3, 3, 64, 64)
    with pytest.raises(ValueError):
        m.reenact(img, frames, output="u8")
    with pytest.raises(ValueError):
        m.reenact(img, frames, output="uint8", channel_order="brg")
    with pytest.raises(ValueError):
        m.reenact(img, frames, channel_order="bgr")                                # a channel order without uint8 output
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        m.reenact(img, frames, output="uint8")
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        m.reenact_video(torch.zeros(48, 64, 3, dtype=torch.uint8), torch.zeros(3, 48, 64, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        importlib.import_module("speak-hack_amd.plan").DecoderPlan(m.Gd.synthesis, 1, torch.device("cpu"), output="u8")
