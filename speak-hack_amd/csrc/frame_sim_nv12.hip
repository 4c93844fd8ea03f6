// Aligned crops on NV12 surfaces (include/spk.h has the definitions): the similarity warp of csrc/frame_sim.hip and the matte and
// colour match of csrc/frame_blend.hip for what a hardware decoder / encoder holds -- a Y plane and an interleaved UV plane, chroma
// sited by replication -- without a packed-RGB detour on either side.
//   frames_nv12_to_f32_sim:       warp + triangle filter along the crop's own axes over the three component fields + YUV -> RGB +
//                                 clamp + normalise -> CHW, one pass;
//   frames_paste_nv12_sim:        inverse warp + quantise + (g, o) per channel + RGB -> YUV + feather x matte blend into the
//                                 surfaces, one pass, one thread per chroma block (2 x 2 luma pixels);
//   paste_colour_match_nv12_sim:  the statistics of csrc/frame_blend_common.hpp over a background read through to_rgb;
//   paste_colour_sums_nv12_sim:   the same statistics handed back as their 13 sums per frame (csrc/colour_window.hip pools them).
// This file holds where the bytes of a surface are read and written and nothing else: rows, validity, footprints and the region
// and the way in's kernel are csrc/frame_sim_common.hpp's, every per-pixel quantity of the way out is its region_pixel's, the sums
// and rows are those of csrc/frame_blend_common.hpp, the taps, the colour arithmetic and the surface checks are
// csrc/frame_nv12_common.hpp's, the way out's kernel -- a template over where its surfaces are, which csrc/frame_table_nv12.hip
// instantiates over a device table -- is csrc/frame_sim_nv12_common.hpp's.  H and W are even, so
// frame pixel (Y, X) inside the frame has its chroma sample (Y >> 1, X >> 1) inside the UV plane, and a chroma block lies wholly
// inside the frame: the clamps of the shared geometry keep every load and store of this file in bounds.
#include "frame_sim_nv12_common.hpp"

namespace {

using namespace spk::frame;

struct Nv12Planes {                     // the two planes of N surfaces, strides in bytes
    const uint8_t* y;
    long long y_image_stride, y_row_stride;
    const uint8_t* uv;
    long long uv_image_stride, uv_row_stride;
};

// the planes as the kernels walk them: one frame has no image stride (the caller's may be anything)
Nv12Planes planes_of(const uint8_t* y, int64_t y_image_stride, int64_t y_row_stride, const uint8_t* uv, int64_t uv_image_stride,
                     int64_t uv_row_stride, int N) {
    return {y, N > 1 ? (long long)y_image_stride : 0ll, (long long)y_row_stride, uv, N > 1 ? (long long)uv_image_stride : 0ll,
            (long long)uv_row_stride};
}

// How surfaces are read: the arithmetic is Nv12Taps' (csrc/frame_nv12_common.hpp); frame n begins n image strides behind the planes.
struct Nv12Read : Nv12Taps<Nv12Read> {
    Nv12Planes p;
    Mat34 to_rgb;
    __device__ __forceinline__ LaunchFrame frame(long long, int H, int W) const { return {H, W}; }
    __device__ __forceinline__ Row row(const LaunchFrame&, long long n, int iy) const {
        return open_row(p.y + n * p.y_image_stride, p.y_row_stride, p.uv + n * p.uv_image_stride, p.uv_row_stride, iy);
    }
    __device__ __forceinline__ void load(const LaunchFrame&, long long n, int X, int Y, double (&b)[3]) const {
        background(p.y + n * p.y_image_stride, p.y_row_stride, p.uv + n * p.uv_image_stride, p.uv_row_stride, X, Y, b);
    }
};

// The paste's target (csrc/frame_sim_nv12_common.hpp has the kernel): the planes of a surface that is written
struct Nv12Target {
    uint8_t* y;
    long long y_image_stride, y_row_stride;
    uint8_t* uv;
    long long uv_image_stride, uv_row_stride;
    __device__ __forceinline__ LaunchFrame frame(long long, int H, int W) const { return {H, W}; }
    __device__ __forceinline__ uint8_t* luma(const LaunchFrame&, long long n, int X, int Y) const {
        return y + n * y_image_stride + (long long)Y * y_row_stride + X;
    }
    __device__ __forceinline__ uint8_t* chroma(long long n, int CX, int CY) const {
        return uv + n * uv_image_stride + (long long)CY * uv_row_stride + (long long)CX * 2;
    }
    __device__ __forceinline__ void load_chroma(const LaunchFrame&, long long n, int CX, int CY, unsigned& u, unsigned& v) const {
        Nv12Pair::load(chroma(n, CX, CY), u, v);
    }
    __device__ __forceinline__ void store_chroma(const LaunchFrame&, long long n, int CX, int CY, unsigned u, unsigned v) const {
        Nv12Pair::store(chroma(n, CX, CY), u, v);
    }
};

// what the paste and its statistics check alike
int check_paste(const char* who, const void* src, const void* y, int64_t y_image_stride, int64_t y_row_stride, const void* uv,
                int64_t uv_image_stride, int64_t uv_row_stride, const float* sim_dev, int N, int Hs, int Ws, int H, int W, bool written,
                double feather, float lo, float k, const float* matte_dev, int matte_frames) {
    SPK_REQUIRE(src, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    if (int rc = check_surface(who, y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N, H, W, written)) return rc;
    SPK_REQUIRE(Hs >= 1 && Ws >= 1, "%s: the source size must be >= 1 (got %d x %d)", who, Hs, Ws);
    return check_blend_params(who, N, feather, lo, k, matte_dev, matte_frames);
}

}  // namespace

extern "C" {

int spk_frames_nv12_to_f32_sim(const uint8_t* y, int64_t y_image_stride, int64_t y_row_stride, const uint8_t* uv, int64_t uv_image_stride,
                               int64_t uv_row_stride, int N, int H, int W, const float* sim_dev, int swap_rb, int standard, int full_range,
                               float* dst, int Hout, int Wout, float scale0, float scale1, float scale2, float shift0, float shift1,
                               float shift2, void* stream) {
    const char* who = "frames_nv12_to_f32_sim";
    if (int rc = check_surface(who, y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N, H, W, false)) return rc;
    SPK_REQUIRE(dst, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(Hout >= 1 && Wout >= 1, "%s: the output size must be >= 1 (got %d x %d)", who, Hout, Wout);
    Nv12Read in = {{}, planes_of(y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N), {}};
    if (int rc = colour_maps(who, standard, full_range, in.to_rgb.m, nullptr)) return rc;
    return launch_frames_to_f32_sim("frames_nv12_to_f32_sim_kernel", in, N, H, W, sim_dev, swap_rb, dst, Hout, Wout,
                                    Affine3{{scale0, scale1, scale2}, {shift0, shift1, shift2}}, stream);
}

int spk_frames_paste_nv12_sim(const float* src, int N, int Hs, int Ws, uint8_t* y, int64_t y_image_stride, int64_t y_row_stride, uint8_t* uv,
                              int64_t uv_image_stride, int64_t uv_row_stride, int H, int W, const float* sim_dev, int standard, int full_range,
                              double feather, float lo, float k, const float* matte_dev, int matte_frames, const float* colour_dev,
                              void* stream) {
    const char* who = "frames_paste_nv12_sim";
    if (int rc = check_paste(who, src, y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, sim_dev, N, Hs, Ws, H, W, true, feather,
                             lo, k, matte_dev, matte_frames))
        return rc;
    Mat34 M;
    if (int rc = colour_maps(who, standard, full_range, nullptr, M.m)) return rc;
    const Nv12Planes p = planes_of(y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N);
    return launch_paste_nv12_sim("frames_paste_nv12_sim_kernel", src, N, Hs, Ws,
                                 Nv12Target{y, p.y_image_stride, p.y_row_stride, uv, p.uv_image_stride, p.uv_row_stride}, H, W, sim_dev, feather, lo, k,
                                 matte_dev, matte_frames, colour_dev, M, stream);
}

int spk_paste_colour_match_nv12_sim(const float* src, int N, int Hs, int Ws, const uint8_t* y, int64_t y_image_stride, int64_t y_row_stride,
                                    const uint8_t* uv, int64_t uv_image_stride, int64_t uv_row_stride, int H, int W, const float* sim_dev,
                                    int standard, int full_range, double feather, float lo, float k, const float* matte_dev, int matte_frames,
                                    double max_gain, double min_sigma, double min_weight, float* colour_out_dev, void* workspace_dev,
                                    size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_match_nv12_sim";
    if (int rc = check_paste(who, src, y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, sim_dev, N, Hs, Ws, H, W, false, feather,
                             lo, k, matte_dev, matte_frames))
        return rc;
    if (int rc = check_colour_match(who, N, max_gain, min_sigma, min_weight, colour_out_dev, workspace_dev, workspace_bytes)) return rc;
    Nv12Read bg = {{}, planes_of(y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N), {}};
    if (int rc = colour_maps(who, standard, full_range, bg.to_rgb.m, nullptr)) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<nv12>", bg, src, N, Hs, Ws, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames,
                                    workspace_dev, ColourFinish{colour_out_dev, max_gain, min_sigma, min_weight, nullptr}, stream);
}

int spk_paste_colour_sums_nv12_sim(const float* src, int N, int Hs, int Ws, const uint8_t* y, int64_t y_image_stride, int64_t y_row_stride,
                                   const uint8_t* uv, int64_t uv_image_stride, int64_t uv_row_stride, int H, int W, const float* sim_dev,
                                   int standard, int full_range, double feather, float lo, float k, const float* matte_dev, int matte_frames,
                                   double* sums_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_sums_nv12_sim";
    if (int rc = check_paste(who, src, y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, sim_dev, N, Hs, Ws, H, W, false, feather,
                             lo, k, matte_dev, matte_frames))
        return rc;
    if (int rc = check_colour_sums(who, N, sums_out_dev, workspace_dev, workspace_bytes)) return rc;
    Nv12Read bg = {{}, planes_of(y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N), {}};
    if (int rc = colour_maps(who, standard, full_range, bg.to_rgb.m, nullptr)) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<nv12>", bg, src, N, Hs, Ws, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames,
                                    workspace_dev, ColourFinish{nullptr, 0.0, 0.0, 0.0, sums_out_dev}, stream);
}

}  // extern "C"
