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
// and rows are those of csrc/frame_blend_common.hpp, the colour maps and the surface checks are csrc/frame_nv12_common.hpp's.  H and W are even, so
// frame pixel (Y, X) inside the frame has its chroma sample (Y >> 1, X >> 1) inside the UV plane, and a chroma block lies wholly
// inside the frame: the clamps of the shared geometry keep every load and store of this file in bounds.
#include "frame_blend_common.hpp"
#include "frame_nv12_common.hpp"

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

// How surfaces are read.  The way in: the three sums run over Y[iy][ix], U[iy >> 1][ix >> 1] and V[iy >> 1][ix >> 1]; luma is byte
// loads, a (U, V) pair is one 16-bit load that stays in a register while ix >> 1 does not change, so it serves the two taps above
// it; the matrix and the clamp follow the means.  The statistics: the background of a region pixel is what the way in makes of
// that pixel, by network channel.
struct Nv12Read {
    Nv12Planes p;
    Mat34 to_rgb;
    struct Row { const uint8_t* y; const uint8_t* c; unsigned pair; };
    __device__ __forceinline__ LaunchFrame frame(long long, int H, int W) const { return {H, W}; }
    __device__ __forceinline__ Row row(const LaunchFrame&, long long n, int iy) const {
        return {p.y + n * p.y_image_stride + (long long)iy * p.y_row_stride, p.uv + n * p.uv_image_stride + (long long)(iy >> 1) * p.uv_row_stride, 0u};
    }
    __device__ __forceinline__ void tap(Row& r, int ix, bool first, double w, double& a_y, double& a_u, double& a_v) const {
        if (first || !(ix & 1)) r.pair = *reinterpret_cast<const uint16_t*>(r.c + (ix & ~1));       // sample ix >> 1
        a_y = fma(w, (double)r.y[ix], a_y);
        a_u = fma(w, (double)(r.pair & 0xffu), a_u);
        a_v = fma(w, (double)(r.pair >> 8), a_v);
    }
    __device__ __forceinline__ void rgb(double y, double u, double v, double (&val)[3]) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) val[c] = fmin(fmax(affine_row(to_rgb, c, y, u, v), 0.0), 255.0);
    }
    __device__ __forceinline__ void load(const LaunchFrame&, long long n, int X, int Y, double (&b)[3]) const {
        const double y = (double)p.y[n * p.y_image_stride + (long long)Y * p.y_row_stride + X];
        const unsigned pair = *reinterpret_cast<const uint16_t*>(p.uv + n * p.uv_image_stride + (long long)(Y >> 1) * p.uv_row_stride + (X & ~1));
        rgb(y, (double)(pair & 0xffu), (double)(pair >> 8), b);
    }
};

// The way out.  The decomposition of frames_paste_u8_sim_kernel over CHROMA BLOCKS: blockIdx.y walks the frames, the
// PASTE_WGS workgroups of blockIdx.x share the blocks (x_lo >> 1 ... x_hi >> 1) x (y_lo >> 1 ... y_hi >> 1) of a frame's bounding
// box, x fastest.  A thread owns one chroma sample and the 2 x 2 luma pixels under it, as frames_paste_nv12_kernel does, and
// visits them in row-major order; a pixel takes part when region_pixel holds it.  It reads only bytes it writes -- a luma byte per
// region pixel, the one UV pair of a block that has a region pixel -- so the surfaces may be pasted in place.
__global__ __launch_bounds__(256) void frames_paste_nv12_sim_kernel(const float* __restrict__ src, int N, int Hs, int Ws, uint8_t* yp,
                                                                    long long y_image_stride, long long y_row_stride, uint8_t* uvp,
                                                                    long long uv_image_stride, long long uv_row_stride, int H, int W,
                                                                    const float* __restrict__ sim, double feather, float lo, float k,
                                                                    const float* __restrict__ matte, int matte_frames,
                                                                    const float* __restrict__ colour, Mat34 from_rgb) {
    const long long plane = (long long)Hs * Ws;
    for (long long n = blockIdx.y; n < N; n += gridDim.y) {
        const Sim m = load_sim(sim, n);
        if (!m.valid) continue;
        const RegionBox box = region_box(m, Hs, Ws, H, W);
        if (box.x_lo > box.x_hi || box.y_lo > box.y_hi) continue;
        const int cx_lo = box.x_lo >> 1, cy_lo = box.y_lo >> 1;
        const long long bw = (box.x_hi >> 1) - cx_lo + 1, total = bw * ((box.y_hi >> 1) - cy_lo + 1);
        const PixelConsts pc = pixel_consts(m, feather);
        const float* img = src + n * 3 * plane;
        const float* mt = matte ? matte + (matte_frames > 1 ? n : 0) * plane : nullptr;
        float g[3], o[3];
        load_colour(colour, n, g, o);
        uint8_t* luma = yp + n * y_image_stride;
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const int CX = cx_lo + (int)(idx % bw), CY = cy_lo + (int)(idx / bw);
            double acc_u = 0.0, acc_v = 0.0, S = 0.0;
            bool any = false;
#pragma unroll 1
            for (int d = 0; d < 4; ++d) {                        // row-major over the block
                const int Yf = 2 * CY + (d >> 1), Xf = 2 * CX + (d & 1);
                float q[3];
                double mm;
                if (!region_pixel(m, pc, Xf, Yf, img, plane, Hs, Ws, mt, lo, k, q, mm)) continue;
                if (colour) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) q[c] = fminf(fmaxf(fmaf(g[c], q[c], o[c]), 0.f), 255.f);
                }
                const double q0 = (double)q[0], q1 = (double)q[1], q2 = (double)q[2];
                const double e_y = affine_row(from_rgb, 0, q0, q1, q2), e_u = affine_row(from_rgb, 1, q0, q1, q2),
                             e_v = affine_row(from_rgb, 2, q0, q1, q2);
                uint8_t* py = luma + (long long)Yf * y_row_stride + Xf;
                *py = (uint8_t)(int)rint(fmin(fmax(fma(1.0 - mm, (double)*py, mm * e_y), 0.0), 255.0));
                const double qm = 0.25 * mm;
                acc_u = fma(qm, e_u, acc_u);
                acc_v = fma(qm, e_v, acc_v);
                S += qm;
                any = true;
            }
            if (!any) continue;
            uint16_t* pcv = reinterpret_cast<uint16_t*>(uvp + n * uv_image_stride + (long long)CY * uv_row_stride + (long long)CX * 2);
            const unsigned pair = *pcv;
            const unsigned u = (unsigned)(int)rint(fmin(fmax(fma(1.0 - S, (double)(pair & 0xffu), acc_u), 0.0), 255.0));
            const unsigned v = (unsigned)(int)rint(fmin(fmax(fma(1.0 - S, (double)(pair >> 8), acc_v), 0.0), 255.0));
            *pcv = (uint16_t)(u | v << 8);
        }
    }
}

// the two maps of a standard, either pointer may be null; refuses what spk_yuv_coeffs refuses (this file links without that one)
int colour_maps(const char* who, int standard, int full_range, double* to_rgb, double* from_rgb) {
    double kr, kb;
    SPK_REQUIRE(primaries(standard, &kr, &kb), "%s: standard must be 601 or 709 (got %d)", who, standard);
    SPK_REQUIRE(full_range == 0 || full_range == 1, "%s: full_range must be 0 or 1 (got %d)", who, full_range);
    yuv_coeffs(kr, kb, full_range != 0, to_rgb, from_rgb);
    return SPK_OK;
}

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
    Nv12Read in = {planes_of(y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N), {}};
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
    hipLaunchKernelGGL(frames_paste_nv12_sim_kernel, dim3(PASTE_WGS, (unsigned)std::min(N, 65535)), dim3(256), 0, (hipStream_t)stream, src, N, Hs,
                       Ws, y, p.y_image_stride, p.y_row_stride, uv, p.uv_image_stride, p.uv_row_stride, H, W, sim_dev, feather, lo, k, matte_dev,
                       matte_frames, colour_dev, M);
    return spk::check_launch("frames_paste_nv12_sim_kernel");
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
    Nv12Read bg = {planes_of(y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N), {}};
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
    Nv12Read bg = {planes_of(y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N), {}};
    if (int rc = colour_maps(who, standard, full_range, bg.to_rgb.m, nullptr)) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<nv12>", bg, src, N, Hs, Ws, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames,
                                    workspace_dev, ColourFinish{nullptr, 0.0, 0.0, 0.0, sums_out_dev}, stream);
}

}  // extern "C"
