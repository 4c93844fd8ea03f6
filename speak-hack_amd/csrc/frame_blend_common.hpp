// What the seamless paste-back shares between pixel formats (csrc/frame_blend.hip: packed RGB; csrc/frame_sim_nv12.hip: NV12
// surfaces): the one device function every per-pixel quantity of the aligned paste comes from, and the statistics of the colour
// match -- 13 fp64 sums per frame, reduced in a fixed order -- with the kernel that turns the sums into rows.  A format's file holds
// where its background is read and how its bytes are written; the weights, the sums and the rows are written once, here, so the
// formats cannot drift and rows from either mean the same thing.
#pragma once

#include "colour_rows_common.hpp"
#include "frame_sim_common.hpp"

namespace spk::frame {

constexpr int STAT_WAVES = 4;           // waves of a workgroup of the statistics kernel (256 threads)

struct PixelConsts { double is2, r, ir, fe; };

__device__ __forceinline__ PixelConsts pixel_consts(const Sim& m, double feather) {
    return {1.0 / (m.s * m.s), fmax(1.0, 1.0 / m.s), 1.0 / fmax(1.0, 1.0 / m.s), 1.0 / (feather + 1.0)};
}

// Frame pixel (Y, X) of a frame with the valid row m.  false: the pixel is outside the region.  true: q[c] is the unmatched
// quantised value of network channel c (fp32, not rounded) and mm = a_u a_v Mt.  img: the frame's first source plane; mt: the
// frame's matte (Hs x Ws) or NULL (Mt = 1).  The matte sum runs beside the channel sums, over the same taps in the same order.
__device__ __forceinline__ bool region_pixel(const Sim& m, const PixelConsts& pc, int X, int Y, const float* __restrict__ img, long long plane,
                                             int Hs, int Ws, const float* __restrict__ mt, float lo, float k, float (&q)[3], double& mm) {
    const double is2 = pc.is2, r = pc.r, ir = pc.ir, fe = pc.fe;
    const double dx = (X + 0.5) - m.tx, dy = (Y + 0.5) - m.ty;
    const double u = (m.a * dx + m.c * dy) * is2, v = (-m.c * dx + m.a * dy) * is2;
    if (!(u >= 0.0 && u < (double)Ws && v >= 0.0 && v < (double)Hs)) return false;
    int i_lo, i_hi, j_lo, j_hi;                                   // taps with |i + 0.5 - u| < r: 2 x 2 when the crop enlarges
    int_range(u - r - 0.5, u + r - 0.5, Ws, i_lo, i_hi);
    int_range(v - r - 0.5, v + r - 0.5, Hs, j_lo, j_hi);
    double su = 0.0, sv = 0.0, v0 = 0.0, v1 = 0.0, v2 = 0.0, vm = 0.0;
    for (int i = i_lo; i <= i_hi; ++i) su += tri(((i + 0.5) - u) * ir);
    for (int j = j_lo; j <= j_hi; ++j) {
        const double wv = tri(((j + 0.5) - v) * ir);
        const float* p = img + (long long)j * Ws;
        double h0 = 0.0, h1 = 0.0, h2 = 0.0, hm = 0.0;
        for (int i = i_lo; i <= i_hi; ++i) {
            const double wu = tri(((i + 0.5) - u) * ir);
            h0 = fma(wu, (double)p[i], h0);
            h1 = fma(wu, (double)p[plane + i], h1);
            h2 = fma(wu, (double)p[2 * plane + i], h2);
            if (mt) {
                const float a = mt[(long long)j * Ws + i];
                hm = fma(wu, a == a ? (double)a : 0.0, hm);       // a NaN sample counts as 0
            }
        }
        sv += wv;
        v0 = fma(wv, h0, v0);
        v1 = fma(wv, h1, v1);
        v2 = fma(wv, h2, v2);
        vm = fma(wv, hm, vm);
    }
    const double norm = su * sv;                                  // > 0: a centre lies within half a pixel of u and of v
    const double val[3] = {v0 / norm, v1 / norm, v2 / norm};
    const double a_u = fmin(1.0, (m.s * fmin(u, (double)Ws - u) + 0.5) * fe), a_v = fmin(1.0, (m.s * fmin(v, (double)Hs - v) + 0.5) * fe);
    mm = a_u * a_v;
    if (mt) mm *= fmin(fmax(vm / norm, 0.0), 1.0);                // fmax returns its other operand for a NaN: clamp01(NaN) = 0
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = quant_unrounded((float)val[c], lo, k);
    return true;
}

// The colour rows of frame n as the paste applies them: (1, 0) without rows and for a row that is not finite.
__device__ __forceinline__ void load_colour(const float* __restrict__ colour, long long n, float (&g)[3], float (&o)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = 1.f, o[c] = 0.f;
    if (colour) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gc = colour[n * 6 + 2 * c], oc = colour[n * 6 + 2 * c + 1];
            if (isfinite(gc) && isfinite(oc)) g[c] = gc, o[c] = oc;
        }
    }
}

// The sum over the 64 lanes of a wave, in every lane: a butterfly, so the order of the additions is fixed.  Every lane executes it.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// The statistics, first kernel.  The paste's decomposition; workgroup g of frame n leaves its 13 sums in part[n][g][0..13), zeros
// when the row is invalid or the box is empty.  Every branch around the barriers depends on n alone: uniform in the workgroup.
// Background: how a format reads the background of region pixel (Y, X) of frame n -- bg.load(n, X, Y, b) leaves b[c], the value
// under NETWORK channel c, in byte units; everything else is the same code for every format.
template <class Background>
__global__ __launch_bounds__(256) void paste_colour_sums_kernel(const float* __restrict__ src, int N, int Hs, int Ws, Background bg, int H, int W,
                                                                const float* __restrict__ sim, double feather, float lo, float k,
                                                                const float* __restrict__ matte, int matte_frames, double* __restrict__ part) {
    __shared__ double red[STAT_WAVES][SUMS];
    const long long plane = (long long)Hs * Ws;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long n = blockIdx.y; n < N; n += gridDim.y) {
        double acc[SUMS];
#pragma unroll
        for (int t = 0; t < SUMS; ++t) acc[t] = 0.0;
        const Sim m = load_sim(sim, n);
        RegionBox box = {0, -1, 0, -1};
        if (m.valid) box = region_box(m, Hs, Ws, H, W);
        if (box.x_lo <= box.x_hi && box.y_lo <= box.y_hi) {
            const long long bw = box.x_hi - box.x_lo + 1, total = bw * (box.y_hi - box.y_lo + 1);
            const PixelConsts pc = pixel_consts(m, feather);
            const float* img = src + n * 3 * plane;
            const float* mt = matte ? matte + (matte_frames > 1 ? n : 0) * plane : nullptr;
            for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
                const int X = box.x_lo + (int)(idx % bw), Y = box.y_lo + (int)(idx / bw);
                float q[3];
                double mm;
                if (!region_pixel(m, pc, X, Y, img, plane, Hs, Ws, mt, lo, k, q, mm)) continue;
                double bc[3];
                bg.load(n, X, Y, bc);
                acc[0] += mm;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double qc = (double)q[c], b = bc[c];
                    const double mq = mm * qc, mb = mm * b;
                    acc[1 + 4 * c] += mq;
                    acc[2 + 4 * c] = fma(mq, qc, acc[2 + 4 * c]);
                    acc[3 + 4 * c] += mb;
                    acc[4 + 4 * c] = fma(mb, b, acc[4 + 4 * c]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < SUMS; ++t) acc[t] = wave_sum(acc[t]);
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < SUMS; ++t) red[wave][t] = acc[t];
        }
        __syncthreads();
        if (threadIdx.x < SUMS) {
            double s = red[0][threadIdx.x];
            for (int w = 1; w < STAT_WAVES; ++w) s += red[w][threadIdx.x];
            part[(n * gridDim.x + blockIdx.x) * SUMS + threadIdx.x] = s;
        }
        __syncthreads();                                              // red is written again for the next frame of this workgroup
    }
}

namespace {                             // a kernel that is no template: one copy per file that includes this, none of them exported

// The statistics, second kernel: a thread per frame adds the frame's partials in index order and writes its three rows.
__global__ __launch_bounds__(64) void paste_colour_rows_kernel(const double* __restrict__ part, int N, int groups, const float* __restrict__ sim,
                                                               double max_gain, double min_var, double min_weight, float* __restrict__ colour) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s[SUMS];
#pragma unroll
    for (int t = 0; t < SUMS; ++t) s[t] = 0.0;
    for (int g = 0; g < groups; ++g) {
#pragma unroll
        for (int t = 0; t < SUMS; ++t) s[t] += part[(n * groups + g) * SUMS + t];
    }
    const bool ok = load_sim(sim, n).valid && s[0] > min_weight;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float g, o;
        colour_row(s[0], s[1 + 4 * c], s[2 + 4 * c], s[3 + 4 * c], s[4 + 4 * c], ok, max_gain, min_var, g, o);
        colour[n * 6 + 2 * c] = g, colour[n * 6 + 2 * c + 1] = o;
    }
}

// The statistics as a result, second kernel: a thread per frame adds the frame's partials in the order of paste_colour_rows_kernel
// -- the totals are that kernel's s[] bit for bit -- and stores the 13 of them; 13 zeros for a frame whose row is invalid.
__global__ __launch_bounds__(64) void paste_colour_totals_kernel(const double* __restrict__ part, int N, int groups, const float* __restrict__ sim,
                                                                 double* __restrict__ sums) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s[SUMS];
#pragma unroll
    for (int t = 0; t < SUMS; ++t) s[t] = 0.0;
    for (int g = 0; g < groups; ++g) {
#pragma unroll
        for (int t = 0; t < SUMS; ++t) s[t] += part[(n * groups + g) * SUMS + t];
    }
    const bool valid = load_sim(sim, n).valid;
#pragma unroll
    for (int t = 0; t < SUMS; ++t) sums[n * SUMS + t] = valid ? s[t] : 0.0;
}

}  // namespace

// ---- host ----
inline int64_t colour_match_workspace_bytes(int N) {
    if (N < 1) return -1;
    return (int64_t)N * PASTE_WGS * SUMS * (int64_t)sizeof(double);
}

// the blend's arguments that do not depend on the pixel format (pointers, sizes and strides are the format's to check)
inline int check_blend_params(const char* who, int N, double feather, float lo, float k, const float* matte_dev, int matte_frames) {
    SPK_REQUIRE(std::isfinite(feather) && feather >= 0.0, "%s: feather must be a finite number >= 0 (got %g)", who, feather);
    if (int rc = check_range(who, lo, k)) return rc;
    SPK_REQUIRE(matte_dev ? (matte_frames == 1 || matte_frames == N) : matte_frames == 0,
                "%s: matte_frames must be 1 or N = %d with a matte and 0 without one (got %d)", who, N, matte_frames);
    return SPK_OK;
}

// the workspace of the partial sums of N frames
inline int check_colour_workspace(const char* who, int N, const void* workspace_dev, size_t workspace_bytes) {
    const int64_t need = colour_match_workspace_bytes(N);
    SPK_REQUIRE(workspace_dev && workspace_bytes >= (size_t)need, "%s: the workspace holds %zu bytes, %lld are needed", who,
                workspace_dev ? workspace_bytes : (size_t)0, (long long)need);
    SPK_REQUIRE((uintptr_t)workspace_dev % alignof(double) == 0, "%s: the workspace must be aligned to %zu bytes", who, alignof(double));
    return SPK_OK;
}

// the statistics' own arguments, alike for every format
inline int check_colour_match(const char* who, int N, double max_gain, double min_sigma, double min_weight, const float* colour_out_dev,
                              const void* workspace_dev, size_t workspace_bytes) {
    SPK_REQUIRE(colour_out_dev, "%s: null colour row array", who);
    if (int rc = check_match_params(who, max_gain, min_sigma, min_weight)) return rc;
    return check_colour_workspace(who, N, workspace_dev, workspace_bytes);
}

// and those of the statistics handed back as sums
inline int check_colour_sums(const char* who, int N, const double* sums_out_dev, const void* workspace_dev, size_t workspace_bytes) {
    SPK_REQUIRE(sums_out_dev, "%s: null sums array", who);
    SPK_REQUIRE((uintptr_t)sums_out_dev % alignof(double) == 0, "%s: the sums array must be aligned to %zu bytes", who, alignof(double));
    return check_colour_workspace(who, N, workspace_dev, workspace_bytes);
}

}  // namespace spk::frame
