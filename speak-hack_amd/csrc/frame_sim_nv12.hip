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
// are csrc/frame_sim_common.hpp's, every per-pixel quantity of the way out is region_pixel's and the sums and rows are those of
// csrc/frame_blend_common.hpp, the colour maps and the surface checks are csrc/frame_nv12_common.hpp's.  H and W are even, so
// frame pixel (Y, X) inside the frame has its chroma sample (Y >> 1, X >> 1) inside the UV plane, and a chroma block lies wholly
// inside the frame: the clamps of the shared geometry keep every load and store of this file in bounds.
#include "frame_blend_common.hpp"
#include "frame_nv12_common.hpp"

namespace {

using namespace spk::frame;

constexpr int TILE = 8;                 // a wave of the way in covers a TILE x TILE block of outputs, as frames_u8_to_f32_sim_kernel

struct Nv12Planes {                     // the two planes of N surfaces, strides in bytes
    const uint8_t* y;
    long long y_image_stride, y_row_stride;
    const uint8_t* uv;
    long long uv_image_stride, uv_row_stride;
};

// The way in.  The tile mapping, footprint and weights of frames_u8_to_f32_sim_kernel; the three sums run over Y[iy][ix],
// U[iy >> 1][ix >> 1] and V[iy >> 1][ix >> 1].  Luma is byte loads; a (U, V) pair is one 16-bit load that stays in a register
// while ix >> 1 does not change, so it serves the two taps above it.  The matrix, the clamp and the normalisation follow the sums.
__global__ __launch_bounds__(256) void frames_nv12_to_f32_sim_kernel(Nv12Planes in, int H, int W, const float* __restrict__ sim, int swap_rb,
                                                                     float* __restrict__ dst, int Hout, int Wout, int tiles_y, int tiles_x,
                                                                     long long tiles, Affine3 af, Mat34 to_rgb) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long tile = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); tile < tiles; tile += waves) {
        const int ox = (int)(tile % tiles_x) * TILE + (lane & 7);
        const int oy = (int)((tile / tiles_x) % tiles_y) * TILE + (lane >> 3);
        const long long n = tile / ((long long)tiles_x * tiles_y);
        if (ox >= Wout || oy >= Hout) continue;
        const Sim m = load_sim(sim, n);
        double acc_y = 0.0, acc_u = 0.0, acc_v = 0.0, wt = 0.0;
        if (m.valid) {
            const double u = ox + 0.5, v = oy + 0.5;
            const double px = m.a * u - m.c * v + m.tx, py = m.c * u + m.a * v + m.ty;
            const double S = fmax(m.s, 1.0);
            const double ia = m.a / (m.s * S), ic = m.c / (m.s * S);              // t_u = ia dx + ic dy,  t_v = -ic dx + ia dy
            const double ext = S * (fabs(m.a) + fabs(m.c)) / m.s;                // half the bounding box of the rotated square
            int y_lo, y_hi;
            int_range(py - ext - 0.5, py + ext - 0.5, H, y_lo, y_hi);             // pixel centres iy + 0.5 within ext of py
            const uint8_t* luma = in.y + n * in.y_image_stride;
            const uint8_t* chroma = in.uv + n * in.uv_image_stride;
            for (int iy = y_lo; iy <= y_hi; ++iy) {
                const double dy = (iy + 0.5) - py;
                // |ia dx + ic dy| < 1 and |-ic dx + ia dy| < 1 as intervals of dx, inside the bounding box
                double d_lo = -ext, d_hi = ext;
                if (ia != 0.0) {
                    const double r0 = (-1.0 - ic * dy) / ia, r1 = (1.0 - ic * dy) / ia;
                    d_lo = fmax(d_lo, fmin(r0, r1)), d_hi = fmin(d_hi, fmax(r0, r1));
                }
                if (ic != 0.0) {
                    const double r0 = (ia * dy - 1.0) / ic, r1 = (ia * dy + 1.0) / ic;
                    d_lo = fmax(d_lo, fmin(r0, r1)), d_hi = fmin(d_hi, fmax(r0, r1));
                }
                int x_lo, x_hi;
                int_range(px + d_lo - 0.5, px + d_hi - 0.5, W, x_lo, x_hi);
                const uint8_t* p = luma + (long long)iy * in.y_row_stride;
                const uint8_t* c = chroma + (long long)(iy >> 1) * in.uv_row_stride;
                unsigned pair = 0;
                for (int ix = x_lo; ix <= x_hi; ++ix) {
                    if (ix == x_lo || !(ix & 1)) pair = *reinterpret_cast<const uint16_t*>(c + (ix & ~1));       // sample ix >> 1
                    const double dx = (ix + 0.5) - px;
                    const double w = tri(fma(ia, dx, ic * dy)) * tri(fma(-ic, dx, ia * dy));
                    wt += w;
                    acc_y = fma(w, (double)p[ix], acc_y);
                    acc_u = fma(w, (double)(pair & 0xffu), acc_u);
                    acc_v = fma(w, (double)(pair >> 8), acc_v);
                }
            }
        }
        const bool hit = wt > 0.0;                                // an invalid row, or a footprint wholly outside the frame: rgb = 0
        const long long plane = (long long)Hout * Wout;
        float* out = dst + n * 3 * plane + (long long)oy * Wout + ox;
#pragma unroll
        for (int c = 0; c < 3; ++c) {                            // c: R, G, B
            const double rgb = hit ? fmin(fmax(affine_row(to_rgb, c, acc_y / wt, acc_u / wt, acc_v / wt), 0.0), 255.0) : 0.0;
            const int cd = swap_rb ? 2 - c : c;
            out[cd * plane] = (float)fma((double)af.scale[cd], rgb, (double)af.shift[cd]);
        }
    }
}

// The way out.  The decomposition of frames_paste_u8_sim_blend_kernel over CHROMA BLOCKS: blockIdx.y walks the frames, the
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

// How the statistics read the background of a region pixel of a surface: what the way in makes of that pixel, by network channel.
struct Nv12Background {
    Nv12Planes p;
    Mat34 to_rgb;
    __device__ __forceinline__ void load(long long n, int X, int Y, double (&b)[3]) const {
        const double y = (double)p.y[n * p.y_image_stride + (long long)Y * p.y_row_stride + X];
        const unsigned pair = *reinterpret_cast<const uint16_t*>(p.uv + n * p.uv_image_stride + (long long)(Y >> 1) * p.uv_row_stride + (X & ~1));
#pragma unroll
        for (int c = 0; c < 3; ++c) b[c] = fmin(fmax(affine_row(to_rgb, c, y, (double)(pair & 0xffu), (double)(pair >> 8)), 0.0), 255.0);
    }
};

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
    Mat34 M;
    if (int rc = colour_maps(who, standard, full_range, M.m, nullptr)) return rc;
    const int tiles_y = spk::ceil_div(Hout, TILE), tiles_x = spk::ceil_div(Wout, TILE);
    const long long tiles = (long long)N * tiles_y * tiles_x;
    const Nv12Planes in = {y, N > 1 ? (long long)y_image_stride : 0ll, (long long)y_row_stride, uv, N > 1 ? (long long)uv_image_stride : 0ll,
                           (long long)uv_row_stride};
    hipLaunchKernelGGL(frames_nv12_to_f32_sim_kernel, grid_for(tiles * 64), dim3(256), 0, (hipStream_t)stream, in, H, W, sim_dev, swap_rb, dst,
                       Hout, Wout, tiles_y, tiles_x, tiles, Affine3{{scale0, scale1, scale2}, {shift0, shift1, shift2}}, M);
    return spk::check_launch("frames_nv12_to_f32_sim_kernel");
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
    hipLaunchKernelGGL(frames_paste_nv12_sim_kernel, dim3(PASTE_WGS, (unsigned)std::min(N, 65535)), dim3(256), 0, (hipStream_t)stream, src, N, Hs,
                       Ws, y, N > 1 ? (long long)y_image_stride : 0ll, (long long)y_row_stride, uv, N > 1 ? (long long)uv_image_stride : 0ll,
                       (long long)uv_row_stride, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames, colour_dev, M);
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
    Nv12Background bg = {{y, N > 1 ? (long long)y_image_stride : 0ll, (long long)y_row_stride, uv, N > 1 ? (long long)uv_image_stride : 0ll,
                          (long long)uv_row_stride}, {}};
    if (int rc = colour_maps(who, standard, full_range, bg.to_rgb.m, nullptr)) return rc;
    hipLaunchKernelGGL(paste_colour_sums_kernel<Nv12Background>, dim3(PASTE_WGS, (unsigned)std::min(N, 65535)), dim3(256), 0, (hipStream_t)stream,
                       src, N, Hs, Ws, bg, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames, (double*)workspace_dev);
    if (int rc = spk::check_launch("paste_colour_sums_kernel<nv12>")) return rc;
    hipLaunchKernelGGL(paste_colour_rows_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const double*)workspace_dev,
                       N, PASTE_WGS, sim_dev, max_gain, min_sigma * min_sigma, min_weight, colour_out_dev);
    return spk::check_launch("paste_colour_rows_kernel");
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
    Nv12Background bg = {{y, N > 1 ? (long long)y_image_stride : 0ll, (long long)y_row_stride, uv, N > 1 ? (long long)uv_image_stride : 0ll,
                          (long long)uv_row_stride}, {}};
    if (int rc = colour_maps(who, standard, full_range, bg.to_rgb.m, nullptr)) return rc;
    hipLaunchKernelGGL(paste_colour_sums_kernel<Nv12Background>, dim3(PASTE_WGS, (unsigned)std::min(N, 65535)), dim3(256), 0, (hipStream_t)stream,
                       src, N, Hs, Ws, bg, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames, (double*)workspace_dev);
    if (int rc = spk::check_launch("paste_colour_sums_kernel<nv12>")) return rc;
    hipLaunchKernelGGL(paste_colour_totals_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const double*)workspace_dev,
                       N, PASTE_WGS, sim_dev, sums_out_dev);
    return spk::check_launch("paste_colour_totals_kernel");
}

}  // extern "C"
