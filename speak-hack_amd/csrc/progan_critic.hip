// The ProGAN critic's own pointwise ops (stylegan.Discriminator, stylegan.py:181-263): the 2x2 average pool with the fade-in
// blend folded in, and the minibatch-std channel.  Both are HBM-bound (the pool) or tiny (the std, on the 4x4 tail); every
// sum runs in a fixed order with no atomics, so results are bitwise reproducible.  Citations per entry point in include/spk.h.
#include "spk_common.hpp"

#include <algorithm>
#include <climits>
#include <cstdint>

namespace {

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// one 2x2 window: ((x00 + x01) + (x10 + x11)), scaled by qa = a / 4, plus b * z -- the same expression on both paths
__device__ __forceinline__ float pool_blend(float x00, float x01, float x10, float x11, float qa, const float* z, float b, size_t zi) {
    const float v = qa * ((x00 + x01) + (x10 + x11));
    return z ? fmaf(b, z[zi], v) : v;
}

// 16-byte path (W % 8 == 0, x / y / z 16-byte aligned): one item = 4 outputs of one output row, read as 2 x 2 float4.
// With H = 2 Ho the input row pair of output row r (= plane * Ho + oy) starts at 2 r W, and output item i starts at 4 i.
__global__ __launch_bounds__(256) void avgpool2x_blend_vec_kernel(const float* __restrict__ x, const float* __restrict__ z,
                                                                 float* __restrict__ y, float qa, float b, unsigned items, unsigned Wq,
                                                                 unsigned W) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= items) return;
    const unsigned r = i / Wq, q = i - r * Wq;
    const float* r0 = x + (size_t)2 * r * W + 8 * (size_t)q;
    const float4 a0 = *(const float4*)r0, a1 = *(const float4*)(r0 + 4);
    const float4 b0 = *(const float4*)(r0 + W), b1 = *(const float4*)(r0 + W + 4);
    float4 o;
    o.x = qa * ((a0.x + a0.y) + (b0.x + b0.y));
    o.y = qa * ((a0.z + a0.w) + (b0.z + b0.w));
    o.z = qa * ((a1.x + a1.y) + (b1.x + b1.y));
    o.w = qa * ((a1.z + a1.w) + (b1.z + b1.w));
    if (z) {
        const float4 zz = *(const float4*)(z + 4 * (size_t)i);
        o.x = fmaf(b, zz.x, o.x); o.y = fmaf(b, zz.y, o.y); o.z = fmaf(b, zz.z, o.z); o.w = fmaf(b, zz.w, o.w);
    }
    *(float4*)(y + 4 * (size_t)i) = o;
}

// scalar path: one output pixel per thread
__global__ __launch_bounds__(256) void avgpool2x_blend_kernel(const float* __restrict__ x, const float* __restrict__ z,
                                                             float* __restrict__ y, float qa, float b, unsigned items, unsigned Wo,
                                                             unsigned W) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= items) return;
    const unsigned r = i / Wo, ox = i - r * Wo;
    const float* r0 = x + (size_t)2 * r * W + 2 * (size_t)ox;
    y[i] = pool_blend(r0[0], r0[1], r0[W], r0[W + 1], qa, z, b, i);
}

// adjoint, 16-byte path: one item = 4 gradient values -> 2 rows x 8 dx values, and 4 dz values
__global__ __launch_bounds__(256) void avgpool2x_blend_bwd_vec_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                                     float* __restrict__ dz, float qa, float b, unsigned items,
                                                                     unsigned Wq, unsigned W) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= items) return;
    const unsigned r = i / Wq, q = i - r * Wq;
    const float4 g = *(const float4*)(dy + 4 * (size_t)i);
    const float4 lo = make_float4(qa * g.x, qa * g.x, qa * g.y, qa * g.y), hi = make_float4(qa * g.z, qa * g.z, qa * g.w, qa * g.w);
    float* r0 = dx + (size_t)2 * r * W + 8 * (size_t)q;
    *(float4*)r0 = lo; *(float4*)(r0 + 4) = hi;
    *(float4*)(r0 + W) = lo; *(float4*)(r0 + W + 4) = hi;
    if (dz) *(float4*)(dz + 4 * (size_t)i) = make_float4(b * g.x, b * g.y, b * g.z, b * g.w);
}

__global__ __launch_bounds__(256) void avgpool2x_blend_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                                 float* __restrict__ dz, float qa, float b, unsigned items, unsigned Wo,
                                                                 unsigned W) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= items) return;
    const unsigned r = i / Wo, ox = i - r * Wo;
    const float g = dy[i], v = qa * g;
    float* r0 = dx + (size_t)2 * r * W + 2 * (size_t)ox;
    r0[0] = v; r0[1] = v; r0[W] = v; r0[W + 1] = v;
    if (dz) dz[i] = b * g;
}

// Minibatch std, launch 1: per position p of the C*HW positions, over the batch: mean, unbiased std (two passes; B = 1 gives
// 0/0 = NaN as torch.std does), and the copy of x into y[:, :C].  y is [B, C+1, HW], so y[b, p] sits at b (P + HW) + p.
__global__ __launch_bounds__(256) void mbstd_stats_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ mu,
                                                         float* __restrict__ sd, int B, long long P, long long HW) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    float m = 0.f;
    for (int b = 0; b < B; ++b) m += x[b * P + p];
    m = m / (float)B;
    float v = 0.f;
    for (int b = 0; b < B; ++b) {
        const float xv = x[b * P + p], d = xv - m;
        v += d * d;
        y[b * (P + HW) + p] = xv;
    }
    mu[p] = m;
    sd[p] = sqrtf(v / (float)(B - 1));
}

// fixed-order LDS tree over 1024 lanes; every lane gets the total
__device__ __forceinline__ float block_sum_1024(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const float t = red[0];
    __syncthreads();
    return t;
}

// launch 2 (one workgroup): s = mean_p sd[p], kept in the workspace and written to every y[b, C, hw]
__global__ __launch_bounds__(1024) void mbstd_mean_kernel(const float* __restrict__ sd, float* __restrict__ s_out, float* __restrict__ y,
                                                         int B, long long P, long long HW) {
    __shared__ float red[1024];
    float acc = 0.f;
    for (long long p = threadIdx.x; p < P; p += 1024) acc += sd[p];
    const float s = block_sum_1024(acc, red) / (float)P;
    if (threadIdx.x == 0) *s_out = s;
    for (long long i = threadIdx.x; i < (long long)B * HW; i += 1024) {
        const long long b = i / HW;
        y[b * (P + HW) + P + (i - b * HW)] = s;
    }
}

// adjoint: every workgroup first sums g = sum_{b,hw} dy[b, C, hw] in the same fixed order, then
//   dx[b, p] = dy[b, p] + g / P * (x[b, p] - mu[p]) / ((B - 1) sd[p])
__global__ __launch_bounds__(1024) void mbstd_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                        const float* __restrict__ mu, const float* __restrict__ sd, float* __restrict__ dx,
                                                        int B, long long P, long long HW) {
    __shared__ float red[1024];
    float acc = 0.f;
    for (long long i = threadIdx.x; i < (long long)B * HW; i += 1024) {
        const long long b = i / HW;
        acc += dy[b * (P + HW) + P + (i - b * HW)];
    }
    const float gp = block_sum_1024(acc, red) / (float)P;
    const float bm1 = (float)(B - 1);
    const long long n = (long long)B * P;
    for (long long i = (long long)blockIdx.x * 1024 + threadIdx.x; i < n; i += (long long)gridDim.x * 1024) {
        const long long b = i / P, p = i - b * P;
        dx[i] = dy[b * (P + HW) + p] + gp * ((x[i] - mu[p]) / (bm1 * sd[p]));
    }
}

inline unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" {

int spk_avgpool2x_blend_fwd(const float* x, const float* z, float* y, float a, float b, int64_t planes, int H, int W, void* stream) {
    SPK_REQUIRE(x && y && planes > 0 && H > 0 && W > 0, "avgpool2x_blend: bad arguments");
    SPK_REQUIRE(H % 2 == 0 && W % 2 == 0, "avgpool2x_blend: H and W must be even (got %d x %d)", H, W);
    const int Wo = W / 2;
    const long long outs = (long long)planes * (H / 2) * Wo;
    SPK_REQUIRE(outs <= INT_MAX, "avgpool2x_blend: %lld outputs exceed the 32-bit index range", outs);
    const float qa = 0.25f * a;
    if (W % 8 == 0 && al16(x) && al16(y) && (!z || al16(z))) {
        hipLaunchKernelGGL(avgpool2x_blend_vec_kernel, dim3(blocks256(outs / 4)), dim3(256), 0, (hipStream_t)stream, x, z, y, qa, b,
                           (unsigned)(outs / 4), (unsigned)(Wo / 4), (unsigned)W);
        return spk::check_launch("avgpool2x_blend_vec_kernel");
    }
    hipLaunchKernelGGL(avgpool2x_blend_kernel, dim3(blocks256(outs)), dim3(256), 0, (hipStream_t)stream, x, z, y, qa, b, (unsigned)outs,
                       (unsigned)Wo, (unsigned)W);
    return spk::check_launch("avgpool2x_blend_kernel");
}

int spk_avgpool2x_blend_bwd(const float* dy, float* dx, float* dz, float a, float b, int64_t planes, int H, int W, void* stream) {
    SPK_REQUIRE(dy && dx && planes > 0 && H > 0 && W > 0, "avgpool2x_blend_bwd: bad arguments");
    SPK_REQUIRE(H % 2 == 0 && W % 2 == 0, "avgpool2x_blend_bwd: H and W must be even (got %d x %d)", H, W);
    const int Wo = W / 2;
    const long long outs = (long long)planes * (H / 2) * Wo;
    SPK_REQUIRE(outs <= INT_MAX, "avgpool2x_blend_bwd: %lld gradient values exceed the 32-bit index range", outs);
    const float qa = 0.25f * a;
    if (W % 8 == 0 && al16(dy) && al16(dx) && (!dz || al16(dz))) {
        hipLaunchKernelGGL(avgpool2x_blend_bwd_vec_kernel, dim3(blocks256(outs / 4)), dim3(256), 0, (hipStream_t)stream, dy, dx, dz, qa, b,
                           (unsigned)(outs / 4), (unsigned)(Wo / 4), (unsigned)W);
        return spk::check_launch("avgpool2x_blend_bwd_vec_kernel");
    }
    hipLaunchKernelGGL(avgpool2x_blend_bwd_kernel, dim3(blocks256(outs)), dim3(256), 0, (hipStream_t)stream, dy, dx, dz, qa, b,
                       (unsigned)outs, (unsigned)Wo, (unsigned)W);
    return spk::check_launch("avgpool2x_blend_bwd_kernel");
}

int64_t spk_minibatch_std_workspace_bytes(int C, int64_t HW) {
    if (C <= 0 || HW <= 0) return -1;
    return (2 * (int64_t)C * HW + 4) * (int64_t)sizeof(float);
}

int spk_minibatch_std_fwd(const float* x, float* y, void* workspace, int B, int C, int64_t HW, void* stream) {
    SPK_REQUIRE(x && y && workspace && B > 0 && C > 0 && HW > 0, "minibatch_std: bad arguments");
    const long long P = (long long)C * HW;
    float* mu = (float*)workspace;
    float* sd = mu + P;
    float* s = sd + P;
    hipLaunchKernelGGL(mbstd_stats_kernel, dim3(blocks256(P)), dim3(256), 0, (hipStream_t)stream, x, y, mu, sd, B, P, (long long)HW);
    int rc = spk::check_launch("mbstd_stats_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(mbstd_mean_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, sd, s, y, B, P, (long long)HW);
    return spk::check_launch("mbstd_mean_kernel");
}

int spk_minibatch_std_bwd(const float* x, const float* dy, const void* workspace, float* dx, int B, int C, int64_t HW, void* stream) {
    SPK_REQUIRE(x && dy && workspace && dx && B > 0 && C > 0 && HW > 0, "minibatch_std_bwd: bad arguments");
    const long long P = (long long)C * HW, n = (long long)B * P;
    const float* mu = (const float*)workspace;
    const long long blocks = std::min((n + 1023) / 1024, 256ll);
    hipLaunchKernelGGL(mbstd_bwd_kernel, dim3((unsigned)blocks), dim3(1024), 0, (hipStream_t)stream, x, dy, mu, mu + P, dx, B, P,
                       (long long)HW);
    return spk::check_launch("mbstd_bwd_kernel");
}

}  // extern "C"
