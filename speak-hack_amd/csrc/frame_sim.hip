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
#include "frame_sim_common.hpp"

namespace {

using namespace spk::frame;

constexpr int TILE = 8;                 // a wave of the way in covers a TILE x TILE block of outputs: neighbouring footprints overlap

// The way in.  Lane l of a wave owns output (8 ty + (l >> 3), 8 tx + (l & 7)) of tile (ty, tx) of one frame, all three channels.
// Its footprint is the square |e_u|, |e_v| < S = max(s, 1) around p = sim(ox + 0.5, oy + 0.5), rotated with the crop: it walks the
// bounding rows of that square inside the frame and, per row, the pixels between the two pairs of edges (intersected before the
// loop: no tap of weight zero is loaded).  Weights and sums are fp64; no LDS, no scratch.
__global__ __launch_bounds__(256) void frames_u8_to_f32_sim_kernel(const uint8_t* __restrict__ src, long long image_stride, long long row_stride,
                                                                   int H, int W, const float* __restrict__ sim, int swap_rb,
                                                                   float* __restrict__ dst, int Hout, int Wout, int tiles_y, int tiles_x,
                                                                   long long tiles, Affine3 af) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long tile = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); tile < tiles; tile += waves) {
        const int ox = (int)(tile % tiles_x) * TILE + (lane & 7);
        const int oy = (int)((tile / tiles_x) % tiles_y) * TILE + (lane >> 3);
        const long long n = tile / ((long long)tiles_x * tiles_y);
        if (ox >= Wout || oy >= Hout) continue;
        const Sim m = load_sim(sim, n);
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, wt = 0.0;
        if (m.valid) {
            const double u = ox + 0.5, v = oy + 0.5;
            const double px = m.a * u - m.c * v + m.tx, py = m.c * u + m.a * v + m.ty;
            const double S = fmax(m.s, 1.0);
            const double ia = m.a / (m.s * S), ic = m.c / (m.s * S);              // t_u = ia dx + ic dy,  t_v = -ic dx + ia dy
            const double ext = S * (fabs(m.a) + fabs(m.c)) / m.s;                // half the bounding box of the rotated square
            int y_lo, y_hi;
            int_range(py - ext - 0.5, py + ext - 0.5, H, y_lo, y_hi);             // pixel centres iy + 0.5 within ext of py
            const uint8_t* img = src + n * image_stride;
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
                const uint8_t* p = img + (long long)iy * row_stride;
                for (int ix = x_lo; ix <= x_hi; ++ix) {
                    const double dx = (ix + 0.5) - px;
                    const double w = tri(fma(ia, dx, ic * dy)) * tri(fma(-ic, dx, ia * dy));
                    wt += w;
                    acc0 = fma(w, (double)p[3 * ix], acc0);
                    acc1 = fma(w, (double)p[3 * ix + 1], acc1);
                    acc2 = fma(w, (double)p[3 * ix + 2], acc2);
                }
            }
        }
        const bool hit = wt > 0.0;                                // an invalid row, or a footprint wholly outside the frame: V = 0
        const double val[3] = {hit ? acc0 / wt : 0.0, hit ? acc1 / wt : 0.0, hit ? acc2 / wt : 0.0};
        const long long plane = (long long)Hout * Wout;
        float* out = dst + n * 3 * plane + (long long)oy * Wout + ox;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int cd = swap_rb ? 2 - c : c;                  // source channel c lands in plane cd
            out[cd * plane] = (float)fma((double)af.scale[cd], val[c], (double)af.shift[cd]);
        }
    }
}

// The way out.  blockIdx.y walks the frames, the PASTE_WGS workgroups of blockIdx.x share one frame: each derives the bounding box
// of the region sim([0, Ws) x [0, Hs)) inside the frame from the row and strides over its pixels (x fastest).  A pixel whose
// (u, v) = sim^-1(X + 0.5, Y + 0.5) is outside the region is skipped; a region pixel takes the separable triangle sum of the fp32
// source around (u, v) -- at most 2 x 2 taps when the crop enlarges, (2 / s)^2 when it shrinks -- quantises in the fp32 order of
// quant_unrounded, reads the background byte it is about to overwrite, and no other, and stores rint(b + m (q - b)) in fp64.
__global__ __launch_bounds__(256) void frames_paste_u8_sim_kernel(const float* __restrict__ src, int N, int Hs, int Ws, uint8_t* dst,
                                                                  long long image_stride, long long row_stride, int H, int W,
                                                                  const float* __restrict__ sim, int swap_rb, double feather, float lo, float k) {
    const long long plane = (long long)Hs * Ws;
    for (long long n = blockIdx.y; n < N; n += gridDim.y) {
        const Sim m = load_sim(sim, n);
        if (!m.valid) continue;
        const RegionBox box = region_box(m, Hs, Ws, H, W);
        const int x_lo = box.x_lo, x_hi = box.x_hi, y_lo = box.y_lo, y_hi = box.y_hi;
        if (x_lo > x_hi || y_lo > y_hi) continue;
        const long long bw = x_hi - x_lo + 1, total = bw * (y_hi - y_lo + 1);
        const double is2 = 1.0 / (m.s * m.s), r = fmax(1.0, 1.0 / m.s), ir = 1.0 / r, fe = 1.0 / (feather + 1.0);
        const float* img = src + n * 3 * plane;
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const int X = x_lo + (int)(idx % bw), Y = y_lo + (int)(idx / bw);
            const double dx = (X + 0.5) - m.tx, dy = (Y + 0.5) - m.ty;
            const double u = (m.a * dx + m.c * dy) * is2, v = (-m.c * dx + m.a * dy) * is2;
            if (!(u >= 0.0 && u < (double)Ws && v >= 0.0 && v < (double)Hs)) continue;
            int i_lo, i_hi, j_lo, j_hi;                                   // taps with |i + 0.5 - u| < r: 2 x 2 when the crop enlarges
            int_range(u - r - 0.5, u + r - 0.5, Ws, i_lo, i_hi);
            int_range(v - r - 0.5, v + r - 0.5, Hs, j_lo, j_hi);
            double su = 0.0, sv = 0.0, v0 = 0.0, v1 = 0.0, v2 = 0.0;
            for (int i = i_lo; i <= i_hi; ++i) su += tri(((i + 0.5) - u) * ir);
            for (int j = j_lo; j <= j_hi; ++j) {
                const double wv = tri(((j + 0.5) - v) * ir);
                const float* p = img + (long long)j * Ws;
                double h0 = 0.0, h1 = 0.0, h2 = 0.0;
                for (int i = i_lo; i <= i_hi; ++i) {
                    const double wu = tri(((i + 0.5) - u) * ir);
                    h0 = fma(wu, (double)p[i], h0);
                    h1 = fma(wu, (double)p[plane + i], h1);
                    h2 = fma(wu, (double)p[2 * plane + i], h2);
                }
                sv += wv;
                v0 = fma(wv, h0, v0);
                v1 = fma(wv, h1, v1);
                v2 = fma(wv, h2, v2);
            }
            const double norm = su * sv;                                  // > 0: a centre lies within half a pixel of u and of v
            const double val[3] = {v0 / norm, v1 / norm, v2 / norm};
            const double a_u = fmin(1.0, (m.s * fmin(u, (double)Ws - u) + 0.5) * fe), a_v = fmin(1.0, (m.s * fmin(v, (double)Hs - v) + 0.5) * fe);
            const double mm = a_u * a_v;
            uint8_t* out = dst + n * image_stride + (long long)Y * row_stride + (long long)X * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int cd = swap_rb ? 2 - c : c;
                const float q = quant_unrounded((float)val[c], lo, k);
                const double b = (double)out[cd];
                out[cd] = (uint8_t)(int)rint(fma(mm, (double)q - b, b));      // m in (0, 1], q and b in [0, 255]: so is the result
            }
        }
    }
}

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
    const int tiles_y = spk::ceil_div(Hout, TILE), tiles_x = spk::ceil_div(Wout, TILE);
    const long long tiles = (long long)N * tiles_y * tiles_x;
    hipLaunchKernelGGL(frames_u8_to_f32_sim_kernel, grid_for(tiles * 64), dim3(256), 0, (hipStream_t)stream, src, (long long)image_stride,
                       (long long)row_stride, H, W, sim_dev, swap_rb, dst, Hout, Wout, tiles_y, tiles_x, tiles,
                       Affine3{{scale0, scale1, scale2}, {shift0, shift1, shift2}});
    return spk::check_launch("frames_u8_to_f32_sim_kernel");
}

int spk_frames_paste_u8_sim(const float* src, int N, int Hs, int Ws, uint8_t* dst, int64_t image_stride, int64_t row_stride, int H, int W,
                            const float* sim_dev, int swap_rb, double feather, float lo, float k, void* stream) {
    const char* who = "frames_paste_u8_sim";
    SPK_REQUIRE(src && dst, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(N >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1, "%s: N / H / W must be >= 1 (N %d, source %d x %d, frame %d x %d)", who, N,
                Hs, Ws, H, W);
    SPK_REQUIRE(row_stride >= 3ll * W, "%s: row stride %lld is smaller than 3 * W = %lld", who, (long long)row_stride, 3ll * W);
    SPK_REQUIRE(N == 1 || image_stride >= (long long)(H - 1) * row_stride + 3ll * W,
                "%s: image stride %lld makes the frames overlap (%d rows of stride %lld)", who, (long long)image_stride, H, (long long)row_stride);
    SPK_REQUIRE(std::isfinite(feather) && feather >= 0.0, "%s: feather must be a finite number >= 0 (got %g)", who, feather);
    if (int rc = check_range(who, lo, k)) return rc;
    hipLaunchKernelGGL(frames_paste_u8_sim_kernel, dim3(PASTE_WGS, (unsigned)std::min(N, 65535)), dim3(256), 0, (hipStream_t)stream, src, N, Hs, Ws,
                       dst, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, H, W, sim_dev, swap_rb, feather, lo, k);
    return spk::check_launch("frames_paste_u8_sim_kernel");
}

}  // extern "C"
