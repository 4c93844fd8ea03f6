// The aligned video edge on RGB32 frames (include/spk.h has the definitions): uint8 [H][W][4] as everything that holds an RGB
// picture on a GPU holds it -- capture surfaces, interop textures, compositors, ARGB buffers -- read and written where the producer
// left them.
//   frames_rgb32_to_f32_sim:        the way in of csrc/frame_sim.hip;
//   frames_paste_rgb32_sim[_blend]: the paste of csrc/frame_sim.hip / csrc/frame_blend.hip;
//   paste_colour_{sums,match}_rgb32_sim: the statistics of csrc/frame_blend.hip.
// The kernels are the templates of csrc/frame_sim_common.hpp and csrc/frame_blend_common.hpp: this file holds where the bytes of
// strided RGB32 frames are, the pixel itself is csrc/frame_rgb32_common.hpp's -- one aligned 32-bit load per tap and per
// background pixel, one load and one store per pasted pixel, the fourth byte carried through.  swap_rb and alpha_first say where the
// colour is; the byte values and the order they enter the sums in are the packed edge's, so every result is that edge's on the
// colour bytes, bit for bit.
#include "frame_rgb32_common.hpp"

namespace {

using namespace spk::frame;

struct Rgb32Source : Rgb32Taps {        // the way in
    const uint8_t* src;
    long long image_stride, row_stride;
    __device__ __forceinline__ LaunchFrame frame(long long, int H, int W) const { return {H, W}; }
    __device__ __forceinline__ const uint8_t* row(const LaunchFrame&, long long n, int iy) const {
        return src + n * image_stride + (long long)iy * row_stride;
    }
};

struct Rgb32Background {                // the statistics
    const uint8_t* dst;
    long long image_stride, row_stride;
    int swap_rb, shift0;
    __device__ __forceinline__ LaunchFrame frame(long long, int H, int W) const { return {H, W}; }
    __device__ __forceinline__ void load(const LaunchFrame&, long long n, int X, int Y, double (&b)[3]) const {
        rgb32_background(dst + n * image_stride + (long long)Y * row_stride, X, shift0, swap_rb, b);
    }
};

struct Rgb32Target {                    // the paste
    uint8_t* dst;
    long long image_stride, row_stride;
    int shift0;
    __device__ __forceinline__ LaunchFrame frame(long long, int H, int W) const { return {H, W}; }
    __device__ __forceinline__ Rgb32Pixel pixel(const LaunchFrame&, long long n, int X, int Y) const {
        return {reinterpret_cast<uint32_t*>(dst + n * image_stride + (long long)Y * row_stride) + X, shift0};
    }
};

// what the entry points of the RGB32 paste and its statistics check alike: check_paste_u8 for a pixel stride of 4
int check_paste_rgb32(const char* who, const void* src, const void* dst, const float* sim_dev, int N, int Hs, int Ws, int64_t image_stride,
                      int64_t row_stride, int H, int W, int alpha_first, bool written, double feather, float lo, float k, const float* matte_dev,
                      int matte_frames) {
    SPK_REQUIRE(src && dst, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(N >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1, "%s: N / H / W must be >= 1 (N %d, source %d x %d, frame %d x %d)", who, N,
                Hs, Ws, H, W);
    if (int rc = check_rgb32_frames(who, dst, image_stride, row_stride, N, H, W, alpha_first, written)) return rc;
    return check_blend_params(who, N, feather, lo, k, matte_dev, matte_frames);
}

template <bool SEAMLESS>
int launch_paste_rgb32(const char* kernel, const float* src, int N, int Hs, int Ws, uint8_t* dst, int64_t image_stride, int64_t row_stride, int H,
                       int W, const float* sim_dev, int swap_rb, int alpha_first, double feather, float lo, float k, const float* matte_dev,
                       int matte_frames, const float* colour_dev, void* stream) {
    return launch_paste_sim<SEAMLESS>(kernel, src, N, Hs, Ws,
                                      Rgb32Target{dst, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, 8 * alpha_first}, H, W, sim_dev,
                                      swap_rb, feather, lo, k, matte_dev, matte_frames, colour_dev, stream);
}

}  // namespace

extern "C" {

int spk_frames_rgb32_to_f32_sim(const uint8_t* src, int64_t image_stride, int64_t row_stride, int N, int H, int W, const float* sim_dev,
                                int swap_rb, int alpha_first, float* dst, int Hout, int Wout, float scale0, float scale1, float scale2,
                                float shift0, float shift1, float shift2, void* stream) {
    const char* who = "frames_rgb32_to_f32_sim";
    SPK_REQUIRE(src && dst, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(N >= 1 && H >= 1 && W >= 1 && Hout >= 1 && Wout >= 1, "%s: N / H / W must be >= 1 (N %d, %d x %d -> %d x %d)", who, N, H, W,
                Hout, Wout);
    if (int rc = check_rgb32_frames(who, src, image_stride, row_stride, N, H, W, alpha_first, false)) return rc;
    return launch_frames_to_f32_sim("frames_rgb32_to_f32_sim_kernel",
                                    Rgb32Source{{8 * alpha_first}, src, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride}, N, H, W,
                                    sim_dev, swap_rb, dst, Hout, Wout, Affine3{{scale0, scale1, scale2}, {shift0, shift1, shift2}}, stream);
}

int spk_frames_paste_rgb32_sim(const float* src, int N, int Hs, int Ws, uint8_t* dst, int64_t image_stride, int64_t row_stride, int H, int W,
                               const float* sim_dev, int swap_rb, int alpha_first, double feather, float lo, float k, void* stream) {
    const char* who = "frames_paste_rgb32_sim";
    if (int rc = check_paste_rgb32(who, src, dst, sim_dev, N, Hs, Ws, image_stride, row_stride, H, W, alpha_first, true, feather, lo, k, nullptr, 0))
        return rc;
    return launch_paste_rgb32<false>("frames_paste_rgb32_sim_kernel", src, N, Hs, Ws, dst, image_stride, row_stride, H, W, sim_dev, swap_rb,
                                     alpha_first, feather, lo, k, nullptr, 0, nullptr, stream);
}

int spk_frames_paste_rgb32_sim_blend(const float* src, int N, int Hs, int Ws, uint8_t* dst, int64_t image_stride, int64_t row_stride, int H, int W,
                                     const float* sim_dev, int swap_rb, int alpha_first, double feather, float lo, float k,
                                     const float* matte_dev, int matte_frames, const float* colour_dev, void* stream) {
    const char* who = "frames_paste_rgb32_sim_blend";
    if (int rc = check_paste_rgb32(who, src, dst, sim_dev, N, Hs, Ws, image_stride, row_stride, H, W, alpha_first, true, feather, lo, k, matte_dev,
                                   matte_frames))
        return rc;
    return launch_paste_rgb32<true>("frames_paste_rgb32_sim_blend_kernel", src, N, Hs, Ws, dst, image_stride, row_stride, H, W, sim_dev, swap_rb,
                                    alpha_first, feather, lo, k, matte_dev, matte_frames, colour_dev, stream);
}

int spk_paste_colour_match_rgb32_sim(const float* src, int N, int Hs, int Ws, const uint8_t* dst, int64_t image_stride, int64_t row_stride, int H,
                                     int W, const float* sim_dev, int swap_rb, int alpha_first, double feather, float lo, float k,
                                     const float* matte_dev, int matte_frames, double max_gain, double min_sigma, double min_weight,
                                     float* colour_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_match_rgb32_sim";
    if (int rc = check_paste_rgb32(who, src, dst, sim_dev, N, Hs, Ws, image_stride, row_stride, H, W, alpha_first, true, feather, lo, k, matte_dev,
                                   matte_frames))
        return rc;
    if (int rc = check_colour_match(who, N, max_gain, min_sigma, min_weight, colour_out_dev, workspace_dev, workspace_bytes)) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<rgb32>",
                                    Rgb32Background{dst, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, swap_rb, 8 * alpha_first}, src,
                                    N, Hs, Ws, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames, workspace_dev,
                                    ColourFinish{colour_out_dev, max_gain, min_sigma, min_weight, nullptr}, stream);
}

int spk_paste_colour_sums_rgb32_sim(const float* src, int N, int Hs, int Ws, const uint8_t* dst, int64_t image_stride, int64_t row_stride, int H,
                                    int W, const float* sim_dev, int swap_rb, int alpha_first, double feather, float lo, float k,
                                    const float* matte_dev, int matte_frames, double* sums_out_dev, void* workspace_dev, size_t workspace_bytes,
                                    void* stream) {
    const char* who = "paste_colour_sums_rgb32_sim";
    if (int rc = check_paste_rgb32(who, src, dst, sim_dev, N, Hs, Ws, image_stride, row_stride, H, W, alpha_first, true, feather, lo, k, matte_dev,
                                   matte_frames))
        return rc;
    if (int rc = check_colour_sums(who, N, sums_out_dev, workspace_dev, workspace_bytes)) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<rgb32>",
                                    Rgb32Background{dst, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, swap_rb, 8 * alpha_first}, src,
                                    N, Hs, Ws, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames, workspace_dev,
                                    ColourFinish{nullptr, 0.0, 0.0, 0.0, sums_out_dev}, stream);
}

}  // extern "C"
