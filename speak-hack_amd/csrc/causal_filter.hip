// The causal counterparts of the temporal windows (include/spk.h has the definitions): what a live feed can use, where frame t + 1
// does not exist yet.  Both keep their state in device memory, read it when a call starts and write it when it ends, so N frames in
// one call and the same frames in any split of calls are the same unrounded fp64 recursion and give the same bits.
//   causal_filter:      a one-euro filter per group of 1 ... 4 components (a landmark is a group of 2): a first-order low-pass whose
//                       cut-off rises with the signal's own filtered speed, with the fit's rule for who takes part, a hold over short
//                       drop-outs and a clean restart after long ones;
//   colour_rows_causal: the 13 sums of the colour match with exponential forgetting, then the row formula of
//                       csrc/colour_rows_common.hpp on the pooled sums.
//
// Both are bound by latency, not by bandwidth: a call is a handful of frames (one, live) of a few hundred numbers.  A thread walks
// the N frames in order and the parallelism is across groups; workgroups of one wave, so that the groups of a feature vector spread
// over the CUs.  The group size is a template parameter: the estimates of a group stay in registers.
#include "colour_rows_common.hpp"
#include <algorithm>
#include <cstdint>

namespace {

using namespace spk::frame;

constexpr int FILTER_THREADS = 64;
constexpr int GRID_CAP = 4096;          // workgroups per launch; the rest of the groups are a grid-stride trip
constexpr double TWO_PI = 6.283185307179586476925286766559;

__device__ __forceinline__ double alpha(double cutoff, double Te) { return 1.0 / (1.0 + 1.0 / (TWO_PI * cutoff * Te)); }

// x and y may be one array (every thread reads the components of a frame before it writes them), so neither is __restrict__.
template <int GR>
__global__ __launch_bounds__(FILTER_THREADS) void causal_filter_kernel(const float* x, const float* w, long long weight_stride, int N, long long G,
                                                                       double rate, double min_cutoff, double beta, double d_cutoff, double hold,
                                                                       double* __restrict__ state, float* y, float* wy) {
    constexpr int SW = 2 + 2 * GR;                                        // (k, w_last, xh[GR], dh[GR])
    const long long D = G * GR;
    for (long long g = (long long)blockIdx.x * FILTER_THREADS + threadIdx.x; g < G; g += (long long)gridDim.x * FILTER_THREADS) {
        double* st = state + g * SW;
        double k = st[0], w_last = st[1], xh[GR], dh[GR];
#pragma unroll
        for (int i = 0; i < GR; ++i) xh[i] = st[2 + i], dh[i] = st[2 + GR + i];
        for (int n = 0; n < N; ++n) {
            const double wn = w ? (double)w[n * weight_stride + g] : 1.0;
            double xn[GR];
            bool part = isfinite(wn) && wn > 0.0;
#pragma unroll
            for (int i = 0; i < GR; ++i) xn[i] = (double)x[n * D + g * GR + i], part = part && isfinite(xn[i]);
            bool out = true;                                              // the frame's output is the estimate (else NaN)
            double w_out = wn;
            if (part) {
                if (k == 0.0 || k - 1.0 > hold) {                         // nothing held, or held too long: the sample itself
#pragma unroll
                    for (int i = 0; i < GR; ++i) xh[i] = xn[i], dh[i] = 0.0;
                } else {
                    const double Te = k / rate, ad = alpha(d_cutoff, Te);
                    double speed2 = 0.0;
#pragma unroll
                    for (int i = 0; i < GR; ++i) {
                        const double d = (xn[i] - xh[i]) / Te;
                        dh[i] = ad * d + (1.0 - ad) * dh[i];
                        speed2 += dh[i] * dh[i];
                    }
                    const double ax = alpha(min_cutoff + beta * sqrt(speed2), Te);
#pragma unroll
                    for (int i = 0; i < GR; ++i) xh[i] = ax * xn[i] + (1.0 - ax) * xh[i];
                }
                w_last = wn, k = 1.0;
            } else {
                out = k >= 1.0 && k <= hold;                              // held; else expired or never seen
                w_out = out ? w_last : 0.0;
                k = k >= 1.0 ? k + 1.0 : k;
            }
            const float bad = __builtin_nanf("");
#pragma unroll
            for (int i = 0; i < GR; ++i) y[n * D + g * GR + i] = out ? (float)xh[i] : bad;
            if (wy) wy[n * G + g] = (float)w_out;
        }
        st[0] = k, st[1] = w_last;
#pragma unroll
        for (int i = 0; i < GR; ++i) st[2 + i] = xh[i], st[2 + GR + i] = dh[i];
    }
}

// Channel c of one feed: the lane walks the feed's N frames -- `stride` frames of 13 sums apart in `sums`, `stride` colour rows
// apart in `rows` -- with the whole of P, and makes the rows of its own channel.  The lane of channel 0 writes the state.  The three
// lanes of a feed run in one wave: all three have read P before one of them writes it.
__device__ __forceinline__ void colour_feed_walk(const double* __restrict__ sums, long long stride, int N, int c, double decay, double max_gain,
                                                 double min_var, double min_weight, double* __restrict__ state, float* __restrict__ rows) {
    double P[SUMS];
#pragma unroll
    for (int i = 0; i < SUMS; ++i) P[i] = state[i];
    for (long long n = 0; n < N; ++n) {
        const double* s = sums + n * stride * SUMS;
        double v[SUMS];
        bool finite = true;
#pragma unroll
        for (int i = 0; i < SUMS; ++i) v[i] = s[i], finite = finite && isfinite(v[i]);
        const bool part = v[0] > min_weight && finite;                    // a NaN S0 fails the comparison
#pragma unroll
        for (int i = 0; i < SUMS; ++i) P[i] = part ? fma(decay, P[i], v[i]) : P[i];
        float g, o;
        colour_row(P[0], P[1 + 4 * c], P[2 + 4 * c], P[3 + 4 * c], P[4 + 4 * c], P[0] > min_weight, max_gain, min_var, g, o);
        rows[n * stride * 6 + 2 * c] = g, rows[n * stride * 6 + 2 * c + 1] = o;
    }
    if (c == 0) {
#pragma unroll
        for (int i = 0; i < SUMS; ++i) state[i] = P[i];
    }
}

// One wave, of which lanes 0, 1, 2 work: each walks the N frames with the whole of P (the same loads in the three lanes: one
// fetch) and makes the rows of its own channel, so the three row formulas of a frame -- divisions and a square root in fp64, the
// long part of a frame -- run side by side.  Lane 0 writes the state.
__global__ __launch_bounds__(64) void colour_rows_causal_kernel(const double* __restrict__ sums, int N, double decay, double max_gain, double min_var,
                                                                double min_weight, double* __restrict__ state, float* __restrict__ rows) {
    const int c = threadIdx.x;
    if (c >= 3) return;
    colour_feed_walk(sums, 1, N, c, decay, max_gain, min_var, min_weight, state, rows);
}

// S feeds side by side, sums [N][S][13], state [S][13], rows [N][S][3][2]: workgroups of one wave whose lanes 3 f + c, f < 21, are
// channel c of feed 21 * block + f (lane 63 idles), so the three lanes of a feed never sit in two waves.  A lane touches its own
// feed's sums, state and rows only.
constexpr int FEEDS_PER_WAVE = 21;
__global__ __launch_bounds__(64) void colour_rows_causal_feeds_kernel(const double* __restrict__ sums, int N, int S, double decay, double max_gain,
                                                                      double min_var, double min_weight, double* __restrict__ state,
                                                                      float* __restrict__ rows) {
    const int f = threadIdx.x / 3, c = threadIdx.x - 3 * f;
    const long long s = (long long)blockIdx.x * FEEDS_PER_WAVE + f;
    if (f >= FEEDS_PER_WAVE || s >= S) return;
    colour_feed_walk(sums + s * SUMS, S, N, c, decay, max_gain, min_var, min_weight, state + s * SUMS, rows + s * 6);
}

// [p, p + bytes) and [q, q + qbytes) share a byte (a null q: no)
inline bool overlap(const void* p, uint64_t bytes, const void* q, uint64_t qbytes) {
    if (!q) return false;
    const uint64_t a = (uint64_t)(uintptr_t)p, b = (uint64_t)(uintptr_t)q;
    return a < b ? b - a < bytes : a - b < qbytes;
}

}  // namespace

extern "C" {

int spk_causal_filter(const float* x_dev, const float* w_dev, int64_t weight_stride, int N, int D, int group, double rate, double min_cutoff,
                      double beta, double d_cutoff, int hold, double* state_dev, float* y_dev, float* wy_dev, void* stream) {
    const char* who = "causal_filter";
    SPK_REQUIRE(x_dev && y_dev, "%s: null signal or output pointer", who);
    SPK_REQUIRE(state_dev, "%s: null state pointer", who);
    SPK_REQUIRE((uintptr_t)state_dev % alignof(double) == 0, "%s: the state must be aligned to %zu bytes", who, alignof(double));
    SPK_REQUIRE(N >= 1, "%s: N must be >= 1 (got %d)", who, N);
    SPK_REQUIRE(D >= 1, "%s: D must be >= 1 (got %d)", who, D);
    SPK_REQUIRE(group >= 1 && group <= 4 && D % group == 0, "%s: group must be 1, 2, 3 or 4 and divide D = %d (got %d)", who, D, group);
    const int64_t G = D / group;
    SPK_REQUIRE(weight_stride == 0 || weight_stride >= G, "%s: weight stride %lld is neither 0 (one set for all frames) nor >= G = %lld", who,
                (long long)weight_stride, (long long)G);
    SPK_REQUIRE(std::isfinite(rate) && rate > 0.0, "%s: rate must be a finite number > 0 (got %g)", who, rate);
    SPK_REQUIRE(std::isfinite(min_cutoff) && min_cutoff > 0.0, "%s: min_cutoff must be a finite number > 0 (got %g)", who, min_cutoff);
    SPK_REQUIRE(std::isfinite(d_cutoff) && d_cutoff > 0.0, "%s: d_cutoff must be a finite number > 0 (got %g)", who, d_cutoff);
    SPK_REQUIRE(std::isfinite(beta) && beta >= 0.0, "%s: beta must be a finite number >= 0 (got %g)", who, beta);
    SPK_REQUIRE(hold >= 0, "%s: hold must be >= 0 (got %d)", who, hold);
    const uint64_t state_bytes = (uint64_t)G * (2 + 2 * group) * sizeof(double), sig_bytes = (uint64_t)N * (uint64_t)D * sizeof(float);
    const uint64_t w_bytes = ((uint64_t)(N - 1) * (uint64_t)weight_stride + (uint64_t)G) * sizeof(float);
    SPK_REQUIRE(!overlap(state_dev, state_bytes, x_dev, sig_bytes) && !overlap(state_dev, state_bytes, y_dev, sig_bytes) &&
                    !overlap(state_dev, state_bytes, w_dev, w_bytes) &&
                    !overlap(state_dev, state_bytes, wy_dev, (uint64_t)N * (uint64_t)G * sizeof(float)),
                "%s: the state of %lld groups overlaps the signal, the weights or an output", who, (long long)G);
    const dim3 grid((unsigned)std::min((G + FILTER_THREADS - 1) / FILTER_THREADS, (int64_t)GRID_CAP)), block(FILTER_THREADS);
    hipStream_t s = (hipStream_t)stream;
#define SPK_FILTER(GR)                                                                                                                    \
    hipLaunchKernelGGL(causal_filter_kernel<GR>, grid, block, 0, s, x_dev, w_dev, (long long)weight_stride, N, (long long)G, rate, min_cutoff, \
                       beta, d_cutoff, (double)hold, state_dev, y_dev, wy_dev)
    switch (group) {
        case 1: SPK_FILTER(1); break;
        case 2: SPK_FILTER(2); break;
        case 3: SPK_FILTER(3); break;
        default: SPK_FILTER(4); break;
    }
#undef SPK_FILTER
    return spk::check_launch("causal_filter_kernel");
}

int spk_colour_rows_causal(const double* sums_dev, int N, double decay, double max_gain, double min_sigma, double min_weight, double* state_dev,
                           float* rows_out_dev, void* stream) {
    const char* who = "colour_rows_causal";
    SPK_REQUIRE(sums_dev, "%s: null sums array", who);
    SPK_REQUIRE(state_dev, "%s: null state pointer", who);
    SPK_REQUIRE(rows_out_dev, "%s: null colour row array", who);
    SPK_REQUIRE((uintptr_t)sums_dev % alignof(double) == 0 && (uintptr_t)state_dev % alignof(double) == 0,
                "%s: the sums array and the state must be aligned to %zu bytes", who, alignof(double));
    SPK_REQUIRE(N >= 1, "%s: N must be >= 1 (got %d)", who, N);
    SPK_REQUIRE(decay >= 0.0 && decay <= 1.0, "%s: decay must be in [0, 1] (got %g)", who, decay);      // a NaN fails both
    if (int rc = check_match_params(who, max_gain, min_sigma, min_weight)) return rc;
    const uint64_t state_bytes = SUMS * sizeof(double), sums_bytes = (uint64_t)N * SUMS * sizeof(double), rows_bytes = (uint64_t)N * 6 * sizeof(float);
    SPK_REQUIRE(!overlap(state_dev, state_bytes, sums_dev, sums_bytes) && !overlap(state_dev, state_bytes, rows_out_dev, rows_bytes) &&
                    !overlap(sums_dev, sums_bytes, rows_out_dev, rows_bytes),
                "%s: the sums of %d frames, the state and the rows overlap", who, N);
    hipLaunchKernelGGL(colour_rows_causal_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums_dev, N, decay, max_gain, min_sigma * min_sigma,
                       min_weight, state_dev, rows_out_dev);
    return spk::check_launch("colour_rows_causal_kernel");
}

int spk_colour_rows_causal_feeds(const double* sums_dev, int N, int S, double decay, double max_gain, double min_sigma, double min_weight,
                                 double* state_dev, float* rows_out_dev, void* stream) {
    const char* who = "colour_rows_causal_feeds";
    SPK_REQUIRE(sums_dev, "%s: null sums array", who);
    SPK_REQUIRE(state_dev, "%s: null state pointer", who);
    SPK_REQUIRE(rows_out_dev, "%s: null colour row array", who);
    SPK_REQUIRE((uintptr_t)sums_dev % alignof(double) == 0 && (uintptr_t)state_dev % alignof(double) == 0,
                "%s: the sums array and the state must be aligned to %zu bytes", who, alignof(double));
    SPK_REQUIRE(N >= 1, "%s: N must be >= 1 (got %d)", who, N);
    SPK_REQUIRE(S >= 1, "%s: S must be >= 1 (got %d)", who, S);
    SPK_REQUIRE((int64_t)N * S <= INT32_MAX / SUMS, "%s: %d frames of %d feeds are 2^31 sums or more", who, N, S);
    SPK_REQUIRE(decay >= 0.0 && decay <= 1.0, "%s: decay must be in [0, 1] (got %g)", who, decay);      // a NaN fails both
    if (int rc = check_match_params(who, max_gain, min_sigma, min_weight)) return rc;
    const uint64_t frames = (uint64_t)N * (uint64_t)S;                    // (< 2^31 / 13: no product below wraps)
    const uint64_t state_bytes = (uint64_t)S * SUMS * sizeof(double), sums_bytes = frames * SUMS * sizeof(double), rows_bytes = frames * 6 * sizeof(float);
    SPK_REQUIRE(!overlap(state_dev, state_bytes, sums_dev, sums_bytes) && !overlap(state_dev, state_bytes, rows_out_dev, rows_bytes) &&
                    !overlap(sums_dev, sums_bytes, rows_out_dev, rows_bytes),
                "%s: the sums of %d frames of %d feeds, the states and the rows overlap", who, N, S);
    hipLaunchKernelGGL(colour_rows_causal_feeds_kernel, dim3((unsigned)((S + FEEDS_PER_WAVE - 1) / FEEDS_PER_WAVE)), dim3(64), 0, (hipStream_t)stream,
                       sums_dev, N, S, decay, max_gain, min_sigma * min_sigma, min_weight, state_dev, rows_out_dev);
    return spk::check_launch("colour_rows_causal_feeds_kernel");
}

}  // extern "C"
