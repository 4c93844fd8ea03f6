// Colour rows from a window of sums (include/spk.h has the definitions): the 13 fp64 sums per frame that paste_colour_sums_sim and
// its NV12 form hand back, pooled over the frames t - radius ... t + radius with a Gaussian weight, then the row formula of
// csrc/frame_blend_common.hpp (paste_colour_rows_kernel) on the pooled sums.  The sums are linear, so a window over them is again a set of sums of the same
// meaning -- the statistics of the face over a stretch of video, every frame weighing in with its own weighted area -- and a frame
// that has nothing to say (an invalid row, a matte that is all zero) simply takes no part.  Smoothing the rows (g, o) instead would
// drag the neighbours of such a frame towards the identity it got by rule, and would average o = mu_b - g mu_q as if it did not
// depend on g.
//
// A thread per frame: the work is (2 radius + 1) x 13 fp64 loads from an array of a few kilobytes that stays in L2, far too
// little for a wave per frame to pay.  The window's weights are computed once per workgroup into LDS; the loop body has no branch
// (a clamped index, a select per sum), so the loads of neighbouring iterations overlap.  Plain loads and stores, no atomics: the
// additions run in ascending d whatever the launch, and a frame's row depends on (sums, T, t, radius, sigma, parameters) alone --
// a sub-range [n0, n0 + n) gives the bits the whole clip gives.
#include "colour_rows_common.hpp"
#include <cstdint>

namespace {

using namespace spk::frame;

constexpr int RADIUS_MAX = 64;          // frames on either side of the window: the bound of spk_sim_smooth
constexpr int WINDOW_THREADS = 64;

__global__ __launch_bounds__(WINDOW_THREADS) void colour_rows_window_kernel(const double* __restrict__ sums, int T, int n0, int n, int radius,
                                                                            double kexp, double max_gain, double min_var, double min_weight,
                                                                            float* __restrict__ rows) {
    __shared__ double kd[2 * RADIUS_MAX + 1];
    for (int i = threadIdx.x; i <= 2 * radius; i += WINDOW_THREADS) {
        const int d = i - radius;
        kd[i] = exp(kexp * (double)(d * d));                              // kexp = -1 / (2 sigma^2); k_0 = exp(-0) = 1 exactly
    }
    __syncthreads();
    const int r = blockIdx.x * WINDOW_THREADS + threadIdx.x;
    if (r >= n) return;
    const int t = n0 + r;
    double P[SUMS];
#pragma unroll
    for (int i = 0; i < SUMS; ++i) P[i] = 0.0;
    bool any = false;
    for (int d = -radius; d <= radius; ++d) {
        const int j = t + d, jc = min(max(j, 0), T - 1);                  // the load is in bounds whatever j; `part` decides its use
        const double* s = sums + (long long)jc * SUMS;
        double v[SUMS];
        bool finite = true;
#pragma unroll
        for (int i = 0; i < SUMS; ++i) v[i] = s[i], finite = finite && isfinite(v[i]);
        const bool part = j == jc && v[0] > min_weight && (d == 0 || finite);      // a NaN S0 fails the comparison
        const double k = kd[d + radius];
        any = any || part;
#pragma unroll
        for (int i = 0; i < SUMS; ++i) P[i] = part ? fma(k, v[i], P[i]) : P[i];
    }
    // the row formula of paste_colour_rows_kernel, on P
    float* out = rows + (long long)r * 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float g, o;
        colour_row(P[0], P[1 + 4 * c], P[2 + 4 * c], P[3 + 4 * c], P[4 + 4 * c], any, max_gain, min_var, g, o);
        out[2 * c] = g, out[2 * c + 1] = o;
    }
}

}  // namespace

extern "C" {

int spk_colour_rows_window(const double* sums_dev, int T, int n0, int n, int radius, double sigma, double max_gain, double min_sigma,
                           double min_weight, float* rows_out_dev, void* stream) {
    const char* who = "colour_rows_window";
    SPK_REQUIRE(sums_dev, "%s: null sums array", who);
    SPK_REQUIRE(rows_out_dev, "%s: null colour row array", who);
    SPK_REQUIRE((uintptr_t)sums_dev % alignof(double) == 0, "%s: the sums array must be aligned to %zu bytes", who, alignof(double));
    SPK_REQUIRE(T >= 1, "%s: T must be >= 1 (got %d)", who, T);
    SPK_REQUIRE(n >= 1 && n0 >= 0 && (long long)n0 + n <= T, "%s: frames [%d, %d + %d) are not a range of a clip of %d frames", who, n0, n0, n, T);
    SPK_REQUIRE(radius >= 0 && radius <= RADIUS_MAX, "%s: radius must be in [0, %d] (got %d)", who, RADIUS_MAX, radius);
    SPK_REQUIRE(std::isfinite(sigma) && sigma > 0.0, "%s: sigma must be a finite number > 0 (got %g)", who, sigma);
    if (int rc = check_match_params(who, max_gain, min_sigma, min_weight)) return rc;
    hipLaunchKernelGGL(colour_rows_window_kernel, dim3((unsigned)((n + WINDOW_THREADS - 1) / WINDOW_THREADS)), dim3(WINDOW_THREADS), 0,
                       (hipStream_t)stream, sums_dev, T, n0, n, radius, -0.5 / (sigma * sigma), max_gain, min_sigma * min_sigma, min_weight,
                       rows_out_dev);
    return spk::check_launch("colour_rows_window_kernel");
}

}  // extern "C"
