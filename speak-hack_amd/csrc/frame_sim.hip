// The video-frame edge through a per-frame similarity transform: aligned face crops in and out (include/spk.h has the definitions).
//
// A tracker that fits eye and mouth landmarks leaves one row sim = (a, c, tx, ty) per frame on the device:
//   x = a u - c v + tx,  y = c u + a v + ty,  s = sqrt(a^2 + c^2)      network coordinates (u, v) -> frame coordinates (x, y)
// The table-driven resize of csrc/frame_io.hip has one host-built table per axis per call; a crop whose scale and angle change per
// frame has its filter weights computed here, in the kernel, in fp64:
//   frames_u8_to_f32_sim: warp + triangle filter along the crop's own axes + normalise + HWC -> CHW, one pass;
//   frames_paste_u8_sim:  inverse warp + quantise + feather-blend into the full frames + CHW -> HWC, one pass.
// A row that is not finite or whose s is outside [1/16, 16] is INVALID: the way in writes shift_c, the way out leaves the frame
// alone.  The bound keeps every footprint, and with it every thread's loop, finite whatever a tracker wrote.  Coordinates are
// clamped in fp64 BEFORE they become integers, so a wild but finite tx cannot overflow an index.
// This file holds where the bytes of packed frames are read on the way in; the kernel around them is csrc/frame_sim_common.hpp's,
// and the way out is that header's paste kernel with matte and colour rows absent at compile time.
#include "frame_sim_common.hpp"

namespace {

using namespace spk::frame;

// The way in reads packed pixels (RgbTaps) of frames addressed by byte strides, all of the launch's size.
struct RgbSource : RgbTaps {
    const uint8_t* src;
    long long image_stride, row_stride;
    __device__ __forceinline__ LaunchFrame frame(long long, int H, int W) const { return {H, W}; }
    __device__ __forceinline__ const uint8_t* row(const LaunchFrame&, long long n, int iy) const {
        return src + n * image_stride + (long long)iy * row_stride;
    }
};

}  // namespace

extern "C" {

int spk_frames_u8_to_f32_sim(const uint8_t* src, int64_t image_stride, int64_t row_stride, int N, int H, int W, const float* sim_dev,
                             int swap_rb, float* dst, int Hout, int Wout, float scale0, float scale1, float scale2, float shift0,
                             float shift1, float shift2, void* stream) {
    const char* who = "frames_u8_to_f32_sim";
    SPK_REQUIRE(src && dst, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(N >= 1 && H >= 1 && W >= 1 && Hout >= 1 && Wout >= 1, "%s: N / H / W must be >= 1 (N %d, %d x %d -> %d x %d)", who, N, H, W,
                Hout, Wout);
    SPK_REQUIRE(row_stride >= 3ll * W, "%s: row stride %lld is smaller than 3 * W = %lld", who, (long long)row_stride, 3ll * W);
    SPK_REQUIRE(image_stride >= 0, "%s: negative image stride", who);
    return launch_frames_to_f32_sim("frames_u8_to_f32_sim_kernel", RgbSource{{}, src, (long long)image_stride, (long long)row_stride}, N, H, W, sim_dev,
                                    swap_rb, dst, Hout, Wout, Affine3{{scale0, scale1, scale2}, {shift0, shift1, shift2}}, stream);
}

int spk_frames_paste_u8_sim(const float* src, int N, int Hs, int Ws, uint8_t* dst, int64_t image_stride, int64_t row_stride, int H, int W,
                            const float* sim_dev, int swap_rb, double feather, float lo, float k, void* stream) {
    const char* who = "frames_paste_u8_sim";
    if (int rc = check_paste_u8(who, src, dst, sim_dev, N, Hs, Ws, image_stride, row_stride, H, W, feather, lo, k, nullptr, 0)) return rc;
    return launch_paste_u8_sim<false>("frames_paste_u8_sim_kernel", src, N, Hs, Ws, dst, image_stride, row_stride, H, W, sim_dev, swap_rb, feather, lo,
                                      k, nullptr, 0, nullptr, stream);
}

}  // extern "C"
