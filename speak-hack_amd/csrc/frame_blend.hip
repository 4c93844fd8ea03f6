// Seamless paste-back for aligned crops (include/spk.h has the definitions): the paste of csrc/frame_sim.hip with a face-shaped
// alpha matte in generated-image coordinates and a per-channel gain / offset, and the statistics that gain and offset come from.
//   frames_paste_u8_sim_blend: inverse warp + quantise + (g, o) per channel + feather x matte blend into the full frames, one pass;
//   paste_colour_match_sim:    weighted mean / variance of the generated face and of the pixels it is about to replace, per frame
//                              and channel -> rows (g, o).  It reads the background and writes no frame.
//   paste_colour_sums_sim:     the same statistics handed back as their 13 sums per frame, for csrc/colour_window.hip to pool.
// Both kernels take every per-pixel quantity -- region test, taps, val, q, the feather ramp, the matte sample, m -- from ONE device
// function, region_pixel, so the weights of the statistics are the weights of the paste and the two cannot drift.  That function
// is the pixel loop body of frames_paste_u8_sim_kernel with the matte sum added beside the three channel sums: without a matte
// and without colour rows the paste here is that kernel's, bit for bit.  It lives in csrc/frame_blend_common.hpp, with the
// statistics' kernels, because the NV12 form of this file (csrc/frame_sim_nv12.hip) shares them.
//
// The statistics are 13 fp64 sums per frame.  A fixed number of workgroups per frame (PASTE_WGS, the paste's own decomposition)
// each reduce theirs in a fixed order -- per thread over its pixels, a butterfly over the wave, the waves in index order through
// LDS -- and store one partial; a second kernel adds a frame's partials in index order.  No atomics: an fp64 atomic add on global
// memory would make the order of the additions, and with it the last bits of a row, depend on the order workgroups happen to run
// in, and a row that changes from run to run shows as flicker.  Two calls on the same inputs give the same bits.
#include "frame_blend_common.hpp"

namespace {

using namespace spk::frame;

// The paste.  The decomposition of frames_paste_u8_sim_kernel: blockIdx.y walks the frames, the PASTE_WGS workgroups of blockIdx.x
// share a frame's bounding box, x fastest.  A thread reads the one background byte it overwrites.
__global__ __launch_bounds__(256) void frames_paste_u8_sim_blend_kernel(const float* __restrict__ src, int N, int Hs, int Ws, uint8_t* dst,
                                                                        long long image_stride, long long row_stride, int H, int W,
                                                                        const float* __restrict__ sim, int swap_rb, double feather, float lo,
                                                                        float k, const float* __restrict__ matte, int matte_frames,
                                                                        const float* __restrict__ colour) {
    const long long plane = (long long)Hs * Ws;
    for (long long n = blockIdx.y; n < N; n += gridDim.y) {
        const Sim m = load_sim(sim, n);
        if (!m.valid) continue;
        const RegionBox box = region_box(m, Hs, Ws, H, W);
        const int x_lo = box.x_lo, x_hi = box.x_hi, y_lo = box.y_lo, y_hi = box.y_hi;
        if (x_lo > x_hi || y_lo > y_hi) continue;
        const long long bw = x_hi - x_lo + 1, total = bw * (y_hi - y_lo + 1);
        const PixelConsts pc = pixel_consts(m, feather);
        const float* img = src + n * 3 * plane;
        const float* mt = matte ? matte + (matte_frames > 1 ? n : 0) * plane : nullptr;
        float g[3], o[3];
        load_colour(colour, n, g, o);
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const int X = x_lo + (int)(idx % bw), Y = y_lo + (int)(idx / bw);
            float q[3];
            double mm;
            if (!region_pixel(m, pc, X, Y, img, plane, Hs, Ws, mt, lo, k, q, mm)) continue;
            uint8_t* out = dst + n * image_stride + (long long)Y * row_stride + (long long)X * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int cd = swap_rb ? 2 - c : c;
                const float qc = colour ? fminf(fmaxf(fmaf(g[c], q[c], o[c]), 0.f), 255.f) : q[c];
                const double b = (double)out[cd];
                out[cd] = (uint8_t)(int)rint(fma(mm, (double)qc - b, b));     // m in [0, 1], q' and b in [0, 255]: so is the result
            }
        }
    }
}

// How the statistics read the background of a region pixel of packed frames: the three bytes of the pixel, by network channel.
struct RgbBackground {
    const uint8_t* dst;
    long long image_stride, row_stride;
    int swap_rb;
    __device__ __forceinline__ void load(long long n, int X, int Y, double (&b)[3]) const {
        const uint8_t* bg = dst + n * image_stride + (long long)Y * row_stride + (long long)X * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) b[c] = (double)bg[swap_rb ? 2 - c : c];
    }
};

// what the two entry points check alike
int check_paste(const char* who, const void* src, const void* dst, const float* sim_dev, int N, int Hs, int Ws, int64_t image_stride,
                int64_t row_stride, int H, int W, double feather, float lo, float k, const float* matte_dev, int matte_frames) {
    SPK_REQUIRE(src && dst, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(N >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1, "%s: N / H / W must be >= 1 (N %d, source %d x %d, frame %d x %d)", who, N,
                Hs, Ws, H, W);
    SPK_REQUIRE(row_stride >= 3ll * W, "%s: row stride %lld is smaller than 3 * W = %lld", who, (long long)row_stride, 3ll * W);
    SPK_REQUIRE(N == 1 || image_stride >= (long long)(H - 1) * row_stride + 3ll * W,
                "%s: image stride %lld makes the frames overlap (%d rows of stride %lld)", who, (long long)image_stride, H, (long long)row_stride);
    return check_blend_params(who, N, feather, lo, k, matte_dev, matte_frames);
}

}  // namespace

extern "C" {

int spk_frames_paste_u8_sim_blend(const float* src, int N, int Hs, int Ws, uint8_t* dst, int64_t image_stride, int64_t row_stride, int H, int W,
                                  const float* sim_dev, int swap_rb, double feather, float lo, float k, const float* matte_dev, int matte_frames,
                                  const float* colour_dev, void* stream) {
    const char* who = "frames_paste_u8_sim_blend";
    if (int rc = check_paste(who, src, dst, sim_dev, N, Hs, Ws, image_stride, row_stride, H, W, feather, lo, k, matte_dev, matte_frames)) return rc;
    hipLaunchKernelGGL(frames_paste_u8_sim_blend_kernel, dim3(PASTE_WGS, (unsigned)std::min(N, 65535)), dim3(256), 0, (hipStream_t)stream, src, N,
                       Hs, Ws, dst, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, H, W, sim_dev, swap_rb, feather, lo, k, matte_dev,
                       matte_frames, colour_dev);
    return spk::check_launch("frames_paste_u8_sim_blend_kernel");
}

int64_t spk_paste_colour_match_workspace_bytes(int N) { return colour_match_workspace_bytes(N); }

int spk_paste_colour_match_sim(const float* src, int N, int Hs, int Ws, const uint8_t* dst, int64_t image_stride, int64_t row_stride, int H,
                               int W, const float* sim_dev, int swap_rb, double feather, float lo, float k, const float* matte_dev,
                               int matte_frames, double max_gain, double min_sigma, double min_weight, float* colour_out_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_match_sim";
    if (int rc = check_paste(who, src, dst, sim_dev, N, Hs, Ws, image_stride, row_stride, H, W, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_match(who, N, max_gain, min_sigma, min_weight, colour_out_dev, workspace_dev, workspace_bytes)) return rc;
    const RgbBackground bg = {dst, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, swap_rb};
    hipLaunchKernelGGL(paste_colour_sums_kernel<RgbBackground>, dim3(PASTE_WGS, (unsigned)std::min(N, 65535)), dim3(256), 0, (hipStream_t)stream, src,
                       N, Hs, Ws, bg, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames, (double*)workspace_dev);
    if (int rc = spk::check_launch("paste_colour_sums_kernel")) return rc;
    hipLaunchKernelGGL(paste_colour_rows_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const double*)workspace_dev,
                       N, PASTE_WGS, sim_dev, max_gain, min_sigma * min_sigma, min_weight, colour_out_dev);
    return spk::check_launch("paste_colour_rows_kernel");
}

int spk_paste_colour_sums_sim(const float* src, int N, int Hs, int Ws, const uint8_t* dst, int64_t image_stride, int64_t row_stride, int H,
                              int W, const float* sim_dev, int swap_rb, double feather, float lo, float k, const float* matte_dev,
                              int matte_frames, double* sums_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_sums_sim";
    if (int rc = check_paste(who, src, dst, sim_dev, N, Hs, Ws, image_stride, row_stride, H, W, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_sums(who, N, sums_out_dev, workspace_dev, workspace_bytes)) return rc;
    const RgbBackground bg = {dst, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, swap_rb};
    hipLaunchKernelGGL(paste_colour_sums_kernel<RgbBackground>, dim3(PASTE_WGS, (unsigned)std::min(N, 65535)), dim3(256), 0, (hipStream_t)stream, src,
                       N, Hs, Ws, bg, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames, (double*)workspace_dev);
    if (int rc = spk::check_launch("paste_colour_sums_kernel")) return rc;
    hipLaunchKernelGGL(paste_colour_totals_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const double*)workspace_dev,
                       N, PASTE_WGS, sim_dev, sums_out_dev);
    return spk::check_launch("paste_colour_totals_kernel");
}

}  // extern "C"
