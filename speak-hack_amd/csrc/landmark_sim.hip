// Landmarks to the rows of csrc/frame_sim.hip, on the device (include/spk.h has the definitions).
//
// A landmark network leaves points [N][K][2] on the device; the aligned edge wants one row sim = (a, c, tx, ty) per frame:
//   sim_fit_landmarks: the weighted least-squares similarity (no reflection) that carries a template [K][2] in network
//                      coordinates onto a frame's landmarks, centred sums in fp64, two passes;
//   sim_smooth:        a Gaussian window over the rows of neighbouring frames, fp64, rows that are not finite left out.
// A frame the fit cannot serve (fewer than two landmarks take part, a degenerate template, a result that is not finite) becomes
// four NaNs: the row both kernels of frame_sim.hip already treat as invalid, so a tracker drop-out needs no host branch.
#include "spk_common.hpp"
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

constexpr int K_MAX = 4096;             // landmarks per frame: a lane of the fit takes at most K_MAX / 64 of them
constexpr int FIT_WAVES = 4;            // frames per 256-thread workgroup of the fit: a wave each
constexpr int RADIUS_MAX = 64;          // frames on either side of the smoothing window
constexpr int GRID_CAP = 2048;          // workgroups per launch; the rest of the frames are a grid-stride trip

// The sum over the 64 lanes of a wave, in every lane: a butterfly, so lanes i and i ^ m add the same two numbers and all 64 end
// with the same bits.  Every lane of the wave must execute it.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

struct Landmark { double w, u, v, x, y; bool part; };

// landmark k of one frame (p: its points, w: its weights or NULL) with the template: takes part when its weight is finite and > 0
// and its coordinates are finite
__device__ __forceinline__ Landmark load_landmark(const float* __restrict__ p, const float* __restrict__ w, const float* __restrict__ tmpl,
                                                  int k, double offset) {
    Landmark m;
    m.w = w ? (double)w[k] : 1.0;
    m.x = (double)p[2 * k] + offset, m.y = (double)p[2 * k + 1] + offset;
    m.u = (double)tmpl[2 * k], m.v = (double)tmpl[2 * k + 1];
    m.part = isfinite(m.w) && m.w > 0.0 && isfinite(m.x) && isfinite(m.y);
    return m;
}

// A wave per frame.  Lane l takes landmarks l, l + 64, ... (coalesced), keeps its partial sums in fp64, and a butterfly leaves the
// wave's sum in every lane: the centroids of the first pass need no broadcast for the second.  A frame's row depends on its own
// K landmarks and on the lane a landmark falls to, and on nothing else: the same frame alone and in a batch gives the same bits.
__global__ __launch_bounds__(256) void sim_fit_landmarks_kernel(const float* __restrict__ pts, const float* __restrict__ weights,
                                                                long long weight_stride, const float* __restrict__ tmpl, int N, int K,
                                                                double offset, float* __restrict__ sim) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * FIT_WAVES;
    for (long long n = (long long)blockIdx.x * FIT_WAVES + (threadIdx.x >> 6); n < N; n += waves) {       // wave-uniform
        const float* p = pts + n * 2 * K;
        const float* w = weights ? weights + n * weight_stride : nullptr;
        double sw = 0.0, su = 0.0, sv = 0.0, sx = 0.0, sy = 0.0, cnt = 0.0;
        for (int k = lane; k < K; k += 64) {
            const Landmark m = load_landmark(p, w, tmpl, k, offset);
            if (m.part) {
                sw += m.w, cnt += 1.0;
                su = fma(m.w, m.u, su), sv = fma(m.w, m.v, sv);
                sx = fma(m.w, m.x, sx), sy = fma(m.w, m.y, sy);
            }
        }
        sw = wave_sum(sw), cnt = wave_sum(cnt);
        su = wave_sum(su), sv = wave_sum(sv), sx = wave_sum(sx), sy = wave_sum(sy);
        const double mu = su / sw, mv = sv / sw, mx = sx / sw, my = sy / sw;          // cnt = 0: NaN, and no landmark below takes part
        double sd = 0.0, sa = 0.0, sc = 0.0;
        for (int k = lane; k < K; k += 64) {
            const Landmark m = load_landmark(p, w, tmpl, k, offset);
            if (m.part) {
                const double du = m.u - mu, dv = m.v - mv, dx = m.x - mx, dy = m.y - my;
                sd = fma(m.w, du * du + dv * dv, sd);
                sa = fma(m.w, du * dx + dv * dy, sa);
                sc = fma(m.w, du * dy - dv * dx, sc);
            }
        }
        sd = wave_sum(sd), sa = wave_sum(sa), sc = wave_sum(sc);
        const double a = sa / sd, c = sc / sd;
        const float r0 = (float)a, r1 = (float)c, r2 = (float)(mx - (a * mu - c * mv)), r3 = (float)(my - (c * mu + a * mv));
        const bool ok = cnt >= 2.0 && sd > 0.0 && isfinite(r0) && isfinite(r1) && isfinite(r2) && isfinite(r3);
        if (lane == 0) {
            const float bad = __builtin_nanf("");
            float* out = sim + 4 * n;
            out[0] = ok ? r0 : bad, out[1] = ok ? r1 : bad, out[2] = ok ? r2 : bad, out[3] = ok ? r3 : bad;
        }
    }
}

// A thread per frame: the window d = -radius ... radius in that order over the rows that exist and are finite, fp64.
__global__ __launch_bounds__(256) void sim_smooth_kernel(const float* __restrict__ in, int N, int radius, double k, float* __restrict__ out) {
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long long)gridDim.x * blockDim.x) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, sg = 0.0;
        for (int d = -radius; d <= radius; ++d) {
            const long long j = n + d;
            if (j < 0 || j >= N) continue;
            const double r0 = (double)in[4 * j], r1 = (double)in[4 * j + 1], r2 = (double)in[4 * j + 2], r3 = (double)in[4 * j + 3];
            if (!(isfinite(r0) && isfinite(r1) && isfinite(r2) && isfinite(r3))) continue;
            const double g = exp(k * (double)(d * d));                    // k = -1 / (2 sigma^2); g(0) = 1 exactly
            if (sg == 0.0) {                                              // the first row starts the sums: a -0 survives radius = 0
                s0 = g * r0, s1 = g * r1, s2 = g * r2, s3 = g * r3;
            } else {
                s0 = fma(g, r0, s0), s1 = fma(g, r1, s1), s2 = fma(g, r2, s2), s3 = fma(g, r3, s3);
            }
            sg += g;
        }
        const bool hit = sg > 0.0;                                        // no row took part (or every g underflowed: sigma << 1)
        const float bad = __builtin_nanf("");
        float* o = out + 4 * n;
        o[0] = hit ? (float)(s0 / sg) : bad, o[1] = hit ? (float)(s1 / sg) : bad;
        o[2] = hit ? (float)(s2 / sg) : bad, o[3] = hit ? (float)(s3 / sg) : bad;
    }
}

}  // namespace

extern "C" {

int spk_sim_fit_landmarks(const float* pts_dev, const float* weights_dev, int64_t weight_stride, const float* tmpl_dev, int N, int K,
                          double offset, float* sim_dev, void* stream) {
    const char* who = "sim_fit_landmarks";
    SPK_REQUIRE(pts_dev && tmpl_dev, "%s: null landmark or template pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(N >= 1, "%s: N must be >= 1 (got %d)", who, N);
    SPK_REQUIRE(K >= 2 && K <= K_MAX, "%s: K must be in [2, %d] (got %d)", who, K_MAX, K);
    SPK_REQUIRE(weight_stride == 0 || weight_stride >= K, "%s: weight stride %lld is neither 0 (one set for all frames) nor >= K = %d", who,
                (long long)weight_stride, K);
    SPK_REQUIRE(std::isfinite(offset), "%s: offset must be finite (got %g)", who, offset);
    const unsigned blocks = (unsigned)std::min(((long long)N + FIT_WAVES - 1) / FIT_WAVES, (long long)GRID_CAP);
    hipLaunchKernelGGL(sim_fit_landmarks_kernel, dim3(blocks), dim3(64 * FIT_WAVES), 0, (hipStream_t)stream, pts_dev, weights_dev,
                       (long long)weight_stride, tmpl_dev, N, K, offset, sim_dev);
    return spk::check_launch("sim_fit_landmarks_kernel");
}

int spk_sim_smooth(const float* sim_in_dev, int N, int radius, double sigma, float* sim_out_dev, void* stream) {
    const char* who = "sim_smooth";
    SPK_REQUIRE(sim_in_dev && sim_out_dev, "%s: null transform array", who);
    SPK_REQUIRE(N >= 1, "%s: N must be >= 1 (got %d)", who, N);
    SPK_REQUIRE(radius >= 0 && radius <= RADIUS_MAX, "%s: radius must be in [0, %d] (got %d)", who, RADIUS_MAX, radius);
    SPK_REQUIRE(std::isfinite(sigma) && sigma > 0.0, "%s: sigma must be a finite number > 0 (got %g)", who, sigma);
    const uint64_t pi = (uint64_t)(uintptr_t)sim_in_dev, po = (uint64_t)(uintptr_t)sim_out_dev;
    SPK_REQUIRE((pi > po ? pi - po : po - pi) >= 16ull * (uint64_t)N, "%s: the two arrays of %d rows overlap", who, N);
    const unsigned blocks = (unsigned)std::min(((long long)N + 255) / 256, (long long)GRID_CAP);
    hipLaunchKernelGGL(sim_smooth_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, sim_in_dev, N, radius, -0.5 / (sigma * sigma),
                       sim_out_dev);
    return spk::check_launch("sim_smooth_kernel");
}

}  // extern "C"
