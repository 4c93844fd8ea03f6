// Seamless paste-back for aligned crops (include/spk.h has the definitions): the paste of csrc/frame_sim.hip with a face-shaped
// alpha matte in generated-image coordinates and a per-channel gain / offset, and the statistics that gain and offset come from.
//   frames_paste_u8_sim_blend: inverse warp + quantise + (g, o) per channel + feather x matte blend into the full frames, one pass;
//   paste_colour_match_sim:    weighted mean / variance of the generated face and of the pixels it is about to replace, per frame
//                              and channel -> rows (g, o).  It reads the background and writes no frame.
//   paste_colour_sums_sim:     the same statistics handed back as their 13 sums per frame, for csrc/colour_window.hip to pool.
// Both kernels take every per-pixel quantity -- region test, taps, val, q, the feather ramp, the matte sample, m -- from ONE device
// function, region_pixel, so the weights of the statistics are the weights of the paste and the two cannot drift.  The paste is
// one kernel for this file and csrc/frame_sim.hip: that file's instance has matte and colour rows absent at compile time, this
// file's tests both pointers at run time, and without a matte and without colour rows the two give the same bytes.  Kernel and
// region_pixel live in csrc/frame_sim_common.hpp, the statistics in csrc/frame_blend_common.hpp; the NV12 form
// (csrc/frame_sim_nv12.hip) shares both.
//
// The statistics are 13 fp64 sums per frame.  A fixed number of workgroups per frame (PASTE_WGS, the paste's own decomposition)
// each reduce theirs in a fixed order -- per thread over its pixels, a butterfly over the wave, the waves in index order through
// LDS -- and store one partial; a second kernel adds a frame's partials in index order.  No atomics: an fp64 atomic add on global
// memory would make the order of the additions, and with it the last bits of a row, depend on the order workgroups happen to run
// in, and a row that changes from run to run shows as flicker.  Two calls on the same inputs give the same bits.
#include "frame_blend_common.hpp"

namespace {

using namespace spk::frame;

// How the statistics read the background of a region pixel of packed frames: the three bytes of the pixel, by network channel.
struct RgbBackground {
    const uint8_t* dst;
    long long image_stride, row_stride;
    int swap_rb;
    __device__ __forceinline__ LaunchFrame frame(long long, int H, int W) const { return {H, W}; }
    __device__ __forceinline__ void load(const LaunchFrame&, long long n, int X, int Y, double (&b)[3]) const {
        rgb_background(dst + n * image_stride + (long long)Y * row_stride + (long long)X * 3, swap_rb, b);
    }
};

}  // namespace

extern "C" {

int spk_frames_paste_u8_sim_blend(const float* src, int N, int Hs, int Ws, uint8_t* dst, int64_t image_stride, int64_t row_stride, int H, int W,
                                  const float* sim_dev, int swap_rb, double feather, float lo, float k, const float* matte_dev, int matte_frames,
                                  const float* colour_dev, void* stream) {
    const char* who = "frames_paste_u8_sim_blend";
    if (int rc = check_paste_u8(who, src, dst, sim_dev, N, Hs, Ws, image_stride, row_stride, H, W, feather, lo, k, matte_dev, matte_frames)) return rc;
    return launch_paste_u8_sim<true>("frames_paste_u8_sim_blend_kernel", src, N, Hs, Ws, dst, image_stride, row_stride, H, W, sim_dev, swap_rb, feather,
                                     lo, k, matte_dev, matte_frames, colour_dev, stream);
}

int64_t spk_paste_colour_match_workspace_bytes(int N) { return colour_match_workspace_bytes(N); }

int spk_paste_colour_match_sim(const float* src, int N, int Hs, int Ws, const uint8_t* dst, int64_t image_stride, int64_t row_stride, int H,
                               int W, const float* sim_dev, int swap_rb, double feather, float lo, float k, const float* matte_dev,
                               int matte_frames, double max_gain, double min_sigma, double min_weight, float* colour_out_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_match_sim";
    if (int rc = check_paste_u8(who, src, dst, sim_dev, N, Hs, Ws, image_stride, row_stride, H, W, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_match(who, N, max_gain, min_sigma, min_weight, colour_out_dev, workspace_dev, workspace_bytes)) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel", RgbBackground{dst, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, swap_rb},
                                    src, N, Hs, Ws, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames, workspace_dev,
                                    ColourFinish{colour_out_dev, max_gain, min_sigma, min_weight, nullptr}, stream);
}

int spk_paste_colour_sums_sim(const float* src, int N, int Hs, int Ws, const uint8_t* dst, int64_t image_stride, int64_t row_stride, int H,
                              int W, const float* sim_dev, int swap_rb, double feather, float lo, float k, const float* matte_dev,
                              int matte_frames, double* sums_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_sums_sim";
    if (int rc = check_paste_u8(who, src, dst, sim_dev, N, Hs, Ws, image_stride, row_stride, H, W, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_sums(who, N, sums_out_dev, workspace_dev, workspace_bytes)) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel", RgbBackground{dst, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, swap_rb},
                                    src, N, Hs, Ws, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames, workspace_dev,
                                    ColourFinish{nullptr, 0.0, 0.0, 0.0, sums_out_dev}, stream);
}

}  // extern "C"
