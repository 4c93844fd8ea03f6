// Seamless paste-back for aligned crops (include/spk.h has the definitions): the paste of csrc/frame_sim.hip with a face-shaped
// alpha matte in generated-image coordinates and a per-channel gain / offset, and the statistics that gain and offset come from.
//   frames_paste_u8_sim_blend: inverse warp + quantise + (g, o) per channel + feather x matte blend into the full frames, one pass;
//   paste_colour_match_sim:    weighted mean / variance of the generated face and of the pixels it is about to replace, per frame
//                              and channel -> rows (g, o).  It reads the background and writes no frame.
// Both kernels take every per-pixel quantity -- region test, taps, val, q, the feather ramp, the matte sample, m -- from ONE device
// function, region_pixel, so the weights of the statistics are the weights of the paste and the two cannot drift.  That function
// is the pixel loop body of frames_paste_u8_sim_kernel with the matte sum added beside the three channel sums: without a matte
// and without colour rows the paste here is that kernel's, bit for bit.
//
// The statistics are 13 fp64 sums per frame.  A fixed number of workgroups per frame (PASTE_WGS, the paste's own decomposition)
// each reduce theirs in a fixed order -- per thread over its pixels, a butterfly over the wave, the waves in index order through
// LDS -- and store one partial; a second kernel adds a frame's partials in index order.  No atomics: an fp64 atomic add on global
// memory would make the order of the additions, and with it the last bits of a row, depend on the order workgroups happen to run
// in, and a row that changes from run to run shows as flicker.  Two calls on the same inputs give the same bits.
#include "frame_sim_common.hpp"

namespace {

using namespace spk::frame;

constexpr int SUMS = 13;                // S0, then (Sq, Sqq, Sb, Sbb) for each of the three channels
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
        float g[3] = {1.f, 1.f, 1.f}, o[3] = {0.f, 0.f, 0.f};
        if (colour) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float gc = colour[n * 6 + 2 * c], oc = colour[n * 6 + 2 * c + 1];
                if (isfinite(gc) && isfinite(oc)) g[c] = gc, o[c] = oc;
            }
        }
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

// The sum over the 64 lanes of a wave, in every lane: a butterfly, so the order of the additions is fixed.  Every lane executes it.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// The statistics, first kernel.  The paste's decomposition; workgroup g of frame n leaves its 13 sums in part[n][g][0..13), zeros
// when the row is invalid or the box is empty.  Every branch around the barriers depends on n alone: uniform in the workgroup.
__global__ __launch_bounds__(256) void paste_colour_sums_kernel(const float* __restrict__ src, int N, int Hs, int Ws, const uint8_t* __restrict__ dst,
                                                                long long image_stride, long long row_stride, int H, int W,
                                                                const float* __restrict__ sim, int swap_rb, double feather, float lo, float k,
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
                const uint8_t* bg = dst + n * image_stride + (long long)Y * row_stride + (long long)X * 3;
                acc[0] += mm;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double qc = (double)q[c], b = (double)bg[swap_rb ? 2 - c : c];
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
        float g = 1.f, o = 0.f;
        if (ok) {
            const double mu_q = s[1 + 4 * c] / s[0], var_q = fmax(s[2 + 4 * c] / s[0] - mu_q * mu_q, 0.0);
            const double mu_b = s[3 + 4 * c] / s[0], var_b = fmax(s[4 + 4 * c] / s[0] - mu_b * mu_b, 0.0);
            const double gain = var_q <= min_var ? 1.0 : fmin(fmax(sqrt(var_b / var_q), 1.0 / max_gain), max_gain);
            g = (float)gain, o = (float)(mu_b - gain * mu_q);
        }
        colour[n * 6 + 2 * c] = g, colour[n * 6 + 2 * c + 1] = o;
    }
}

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
    SPK_REQUIRE(std::isfinite(feather) && feather >= 0.0, "%s: feather must be a finite number >= 0 (got %g)", who, feather);
    if (int rc = check_range(who, lo, k)) return rc;
    SPK_REQUIRE(matte_dev ? (matte_frames == 1 || matte_frames == N) : matte_frames == 0,
                "%s: matte_frames must be 1 or N = %d with a matte and 0 without one (got %d)", who, N, matte_frames);
    return SPK_OK;
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

int64_t spk_paste_colour_match_workspace_bytes(int N) {
    if (N < 1) return -1;
    return (int64_t)N * PASTE_WGS * SUMS * (int64_t)sizeof(double);
}

int spk_paste_colour_match_sim(const float* src, int N, int Hs, int Ws, const uint8_t* dst, int64_t image_stride, int64_t row_stride, int H,
                               int W, const float* sim_dev, int swap_rb, double feather, float lo, float k, const float* matte_dev,
                               int matte_frames, double max_gain, double min_sigma, double min_weight, float* colour_out_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_match_sim";
    if (int rc = check_paste(who, src, dst, sim_dev, N, Hs, Ws, image_stride, row_stride, H, W, feather, lo, k, matte_dev, matte_frames)) return rc;
    SPK_REQUIRE(colour_out_dev, "%s: null colour row array", who);
    SPK_REQUIRE(std::isfinite(max_gain) && max_gain >= 1.0, "%s: max_gain must be a finite number >= 1 (got %g)", who, max_gain);
    SPK_REQUIRE(std::isfinite(min_sigma) && min_sigma >= 0.0, "%s: min_sigma must be a finite number >= 0 (got %g)", who, min_sigma);
    SPK_REQUIRE(std::isfinite(min_weight) && min_weight >= 0.0, "%s: min_weight must be a finite number >= 0 (got %g)", who, min_weight);
    const int64_t need = spk_paste_colour_match_workspace_bytes(N);
    SPK_REQUIRE(workspace_dev && workspace_bytes >= (size_t)need, "%s: the workspace holds %zu bytes, %lld are needed", who,
                workspace_dev ? workspace_bytes : (size_t)0, (long long)need);
    SPK_REQUIRE((uintptr_t)workspace_dev % alignof(double) == 0, "%s: the workspace must be aligned to %zu bytes", who, alignof(double));
    hipLaunchKernelGGL(paste_colour_sums_kernel, dim3(PASTE_WGS, (unsigned)std::min(N, 65535)), dim3(256), 0, (hipStream_t)stream, src, N, Hs, Ws,
                       dst, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, H, W, sim_dev, swap_rb, feather, lo, k, matte_dev,
                       matte_frames, (double*)workspace_dev);
    if (int rc = spk::check_launch("paste_colour_sums_kernel")) return rc;
    hipLaunchKernelGGL(paste_colour_rows_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const double*)workspace_dev,
                       N, PASTE_WGS, sim_dev, max_gain, min_sigma * min_sigma, min_weight, colour_out_dev);
    return spk::check_launch("paste_colour_rows_kernel");
}

}  // extern "C"
