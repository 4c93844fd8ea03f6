// What the seamless paste-back shares between pixel formats (csrc/frame_blend.hip: packed RGB; csrc/frame_sim_nv12.hip: NV12
// surfaces): the statistics of the colour match -- 13 fp64 sums per frame, reduced in a fixed order -- with the kernels that turn
// the sums into rows or hand them back, and the one host path that launches them.  A format's file holds where its background is
// read and how its bytes are written; the weights (region_pixel of csrc/frame_sim_common.hpp), the sums and the rows are written
// once, so the formats cannot drift and rows from either mean the same thing.
#pragma once

#include "colour_rows_common.hpp"
#include "frame_sim_common.hpp"

namespace spk::frame {

constexpr int STAT_WAVES = 4;           // waves of a workgroup of the statistics kernel (256 threads)

// The sum over the 64 lanes of a wave, in every lane: a butterfly, so the order of the additions is fixed.  Every lane executes it.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// The statistics, first kernel.  The paste's decomposition; workgroup g of frame n leaves its 13 sums in part[n][g][0..13), zeros
// when the row is invalid, the frame is absent or the box is empty.  Every branch around the barriers depends on n alone: uniform
// in the workgroup.  Background: how a format reads the background of region pixel (Y, X) of frame n -- bg.frame(n, H, W) is the
// frame (csrc/frame_sim_common.hpp), bg.load(frame, n, X, Y, b) leaves b[c], the value under NETWORK channel c, in byte units;
// everything else is the same code for every format.
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
        const auto fr = bg.frame(n, H, W);
        RegionBox box = {0, -1, 0, -1};
        if (m.valid && fr.usable()) box = region_box(m, Hs, Ws, fr.H, fr.W);
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
                bg.load(fr, n, X, Y, bc);
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

// What becomes of a frame's 13 sums: the rows of the colour match, or the totals themselves.
struct ColourFinish {
    float* colour_out;                  // rows: [N,3,2] to write, with the three parameters of the row formula; NULL: the totals
    double max_gain, min_sigma, min_weight;
    double* sums_out;                   // totals: [N,13] to write
};

// The statistics over checked arguments, for every format: the sums of each workgroup, then a frame's partials into rows or totals.
template <class Background>
int launch_colour_statistics(const char* kernel, const Background& bg, const float* src, int N, int Hs, int Ws, int H, int W, const float* sim_dev,
                             double feather, float lo, float k, const float* matte_dev, int matte_frames, void* workspace_dev,
                             const ColourFinish& fin, void* stream) {
    hipLaunchKernelGGL(paste_colour_sums_kernel<Background>, dim3(PASTE_WGS, (unsigned)std::min(N, 65535)), dim3(256), 0, (hipStream_t)stream, src, N,
                       Hs, Ws, bg, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames, (double*)workspace_dev);
    if (int rc = spk::check_launch(kernel)) return rc;
    const dim3 grid((unsigned)((N + 63) / 64));
    if (fin.colour_out) {
        hipLaunchKernelGGL(paste_colour_rows_kernel, grid, dim3(64), 0, (hipStream_t)stream, (const double*)workspace_dev, N, PASTE_WGS, sim_dev,
                           fin.max_gain, fin.min_sigma * fin.min_sigma, fin.min_weight, fin.colour_out);
        return spk::check_launch("paste_colour_rows_kernel");
    }
    hipLaunchKernelGGL(paste_colour_totals_kernel, grid, dim3(64), 0, (hipStream_t)stream, (const double*)workspace_dev, N, PASTE_WGS, sim_dev,
                       fin.sums_out);
    return spk::check_launch("paste_colour_totals_kernel");
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
