// A face matte per frame from the landmarks' contour, on the device (include/spk.h has the definitions).
//
// The paste of csrc/frame_blend.hip takes a matte [N][Hs][Ws] in generated-image coordinates.  A landmark network leaves points
// [N][K][2] in FRAME coordinates on the device, and csrc/landmark_sim.hip the rows that carry the generated image into the frame.
// One launch makes the matte from the two:
//   the Kc contour landmarks of a frame's window go back through their own frame's row into the generated image, fp64;
//   a Gaussian window over the neighbouring frames (the rule of sim_smooth) steadies every contour point;
//   every pixel takes its signed distance d to the closed outline (even-odd parity decides the sign) and M = clamp01((d + grow) / softness).
// A point no frame of the window can give comes from a fallback outline; without one the frame's matte is zeros.
#include "frame_sim_common.hpp"
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

using namespace spk::frame;

constexpr int K_MAX = 4096;             // landmarks per frame, as the fit of csrc/landmark_sim.hip
constexpr int KC_MIN = 3, KC_MAX = 128; // points of the outline
constexpr int RADIUS_MAX = 64;          // frames on either side of the window, as sim_smooth
constexpr int SIZE_MAX_HW = 4096;       // Hs, Ws
constexpr int THREADS = 256;
constexpr int BAND_PIXELS = 1024;       // a workgroup's band of rows holds about this many pixels: four per thread

struct Contour { int32_t idx[KC_MAX]; };                                  // travels by value: no allocation, no upload

// An edge (A, B) of the outline as a pixel uses it: E = B - A, inv = 1 / |E|^2 (0 for a degenerate edge: it counts as the point A),
// slope = E.x / E.y (read only where the crossing test has found A.y and B.y on two sides of the pixel, so E.y != 0 there).
// B.y is kept as it is: A.y + E.y may round to another number, and the crossing test must see a vertex on one side for both its edges.
struct Edges { double ax[KC_MAX], ay[KC_MAX], by[KC_MAX], ex[KC_MAX], ey[KC_MAX], inv[KC_MAX], slope[KC_MAX]; };

// A workgroup per band of rows of one frame.  Its first Kc threads each build one point of the smoothed outline -- a thread walks
// the window d = -radius ... radius of its own landmark -- and then one edge's constants in LDS; thread 0 adds the outline's bounding
// box.  Every thread then walks its pixels over the Kc edges: the LDS reads are broadcasts (all lanes one address).  The band's
// floats are contiguous in the matte, so consecutive lanes store consecutive addresses.  All in fp64; no scratch, no atomics.
// A frame's outline depends on the frames of its window and on nothing else, and a pixel on its outline and its own centre.
__global__ __launch_bounds__(THREADS) void matte_from_landmarks_kernel(const float* __restrict__ pts, int N, int K, double offset,
                                                                       const float* __restrict__ sim, const Contour contour, int Kc,
                                                                       const float* __restrict__ fallback, int radius, double gk,
                                                                       double softness, double grow, float* __restrict__ matte, int Hs,
                                                                       int Ws, int band, int bands, long long units) {
    __shared__ Edges e;
    __shared__ double px_[KC_MAX], py_[KC_MAX];
    __shared__ double box[4];
    __shared__ int hole;                                                  // a point of the outline is missing: the matte is zeros
    const int tid = threadIdx.x;
    for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {  // uniform in the workgroup, as every branch around a barrier
        const long long n = unit / bands;
        const int j0 = (int)(unit % bands) * band;
        const int rows = min(band, Hs - j0);
        if (tid == 0) hole = 0;
        __syncthreads();
        if (tid < Kc) {
            const int k = contour.idx[tid];
            double su = 0.0, sv = 0.0, sg = 0.0;
            for (int d = -radius; d <= radius; ++d) {
                const long long f = n + d;
                if (f < 0 || f >= N) continue;
                const Sim m = load_sim(sim, f);
                const double x = (double)pts[(f * K + k) * 2] + offset, y = (double)pts[(f * K + k) * 2 + 1] + offset;
                if (!(m.valid && isfinite(x) && isfinite(y))) continue;
                const double dx = x - m.tx, dy = y - m.ty, s2 = m.a * m.a + m.c * m.c;
                const double u = (m.a * dx + m.c * dy) / s2, v = (-m.c * dx + m.a * dy) / s2;
                const double g = exp(gk * (double)(d * d));               // gk = -1 / (2 sigma^2); g(0) = 1 exactly
                if (sg == 0.0) {                                          // the first point starts the sums: radius = 0 is the point itself
                    su = g * u, sv = g * v;
                } else {
                    su = fma(g, u, su), sv = fma(g, v, sv);
                }
                sg += g;
            }
            double u, v;
            if (sg > 0.0) {
                u = su / sg, v = sv / sg;
            } else if (fallback) {                                        // no point took part (or every g underflowed: sigma << 1)
                u = (double)fallback[2 * tid], v = (double)fallback[2 * tid + 1];
            } else {
                u = v = __builtin_nan("");
            }
            if (!(isfinite(u) && isfinite(v))) hole = 1, u = v = 0.0;     // every writer stores the same 1
            px_[tid] = u, py_[tid] = v;
        }
        __syncthreads();
        if (tid < Kc) {
            const int nx = tid + 1 == Kc ? 0 : tid + 1;
            const double ax = px_[tid], ay = py_[tid], ex = px_[nx] - ax, ey = py_[nx] - ay;
            const double len2 = ex * ex + ey * ey;
            e.ax[tid] = ax, e.ay[tid] = ay, e.by[tid] = py_[nx], e.ex[tid] = ex, e.ey[tid] = ey;
            e.inv[tid] = len2 > 0.0 ? 1.0 / len2 : 0.0;
            e.slope[tid] = ey != 0.0 ? ex / ey : 0.0;
        }
        if (tid == 0) {
            double x_lo = px_[0], x_hi = px_[0], y_lo = py_[0], y_hi = py_[0];
            for (int k = 1; k < Kc; ++k) {
                x_lo = fmin(x_lo, px_[k]), x_hi = fmax(x_hi, px_[k]);
                y_lo = fmin(y_lo, py_[k]), y_hi = fmax(y_hi, py_[k]);
            }
            const double reach = fmax(grow, 0.0);                         // farther than this outside the box: (d + grow) < 0, M = 0 exactly
            box[0] = x_lo - reach, box[1] = x_hi + reach, box[2] = y_lo - reach, box[3] = y_hi + reach;
        }
        __syncthreads();
        const bool zeros = hole != 0;
        const double x_lo = box[0], x_hi = box[1], y_lo = box[2], y_hi = box[3];
        float* out = matte + (n * Hs + j0) * (long long)Ws;               // the band's rows * Ws floats are contiguous
        const int pixels = rows * Ws;                                     // <= band * Ws < BAND_PIXELS + 4096
        for (int q = tid; q < pixels; q += THREADS) {
            const double x = (q % Ws) + 0.5, y = (j0 + q / Ws) + 0.5;
            float M = 0.0f;
            if (!zeros && x >= x_lo && x <= x_hi && y >= y_lo && y <= y_hi) {
                double best = INFINITY;
                bool inside = false;
                for (int k = 0; k < Kc; ++k) {
                    const double ax = e.ax[k], ay = e.ay[k], ex = e.ex[k], ey = e.ey[k];
                    const double rx = x - ax, ry = y - ay;
                    const double t = fmin(fmax((rx * ex + ry * ey) * e.inv[k], 0.0), 1.0);
                    const double qx = rx - t * ex, qy = ry - t * ey;
                    best = fmin(best, qx * qx + qy * qy);
                    if ((ay > y) != (e.by[k] > y) && x < ax + ry * e.slope[k]) inside = !inside;
                }
                const double dist = sqrt(best);
                M = (float)fmin(fmax(((inside ? dist : -dist) + grow) / softness, 0.0), 1.0);
            }
            out[q] = M;
        }
        __syncthreads();                                                  // the pixels are done with the edges and the flag before the next unit
    }
}

}  // namespace

extern "C" {

int spk_matte_from_landmarks(const float* pts_dev, int N, int K, double offset, const float* sim_dev, const int32_t* contour_host, int Kc,
                             const float* fallback_dev, int radius, double sigma, double softness, double grow, float* matte_dev, int Hs,
                             int Ws, void* stream) {
    const char* who = "matte_from_landmarks";
    SPK_REQUIRE(pts_dev && sim_dev, "%s: null landmark or transform pointer", who);
    SPK_REQUIRE(contour_host, "%s: null contour", who);
    SPK_REQUIRE(matte_dev, "%s: null matte", who);
    SPK_REQUIRE(N >= 1, "%s: N must be >= 1 (got %d)", who, N);
    SPK_REQUIRE(K >= 1 && K <= K_MAX, "%s: K must be in [1, %d] (got %d)", who, K_MAX, K);
    SPK_REQUIRE(Kc >= KC_MIN && Kc <= KC_MAX, "%s: Kc must be in [%d, %d] (got %d)", who, KC_MIN, KC_MAX, Kc);
    SPK_REQUIRE(Hs >= 1 && Hs <= SIZE_MAX_HW && Ws >= 1 && Ws <= SIZE_MAX_HW, "%s: Hs and Ws must be in [1, %d] (got %d x %d)", who,
                SIZE_MAX_HW, Hs, Ws);
    SPK_REQUIRE(radius >= 0 && radius <= RADIUS_MAX, "%s: radius must be in [0, %d] (got %d)", who, RADIUS_MAX, radius);
    SPK_REQUIRE(std::isfinite(sigma) && sigma > 0.0, "%s: sigma must be a finite number > 0 (got %g)", who, sigma);
    SPK_REQUIRE(std::isfinite(softness) && softness > 0.0, "%s: softness must be a finite number > 0 (got %g)", who, softness);
    SPK_REQUIRE(std::isfinite(grow), "%s: grow must be finite (got %g)", who, grow);
    SPK_REQUIRE(std::isfinite(offset), "%s: offset must be finite (got %g)", who, offset);
    Contour contour = {};
    for (int k = 0; k < Kc; ++k) {
        SPK_REQUIRE(contour_host[k] >= 0 && contour_host[k] < K, "%s: contour[%d] = %d is not a landmark index in [0, %d)", who, k,
                    contour_host[k], K);
        contour.idx[k] = contour_host[k];
    }
    const int band = std::min(Hs, (BAND_PIXELS + Ws - 1) / Ws), bands = (Hs + band - 1) / band;
    const long long units = (long long)N * bands;
    const unsigned blocks = (unsigned)std::min(units, (long long)GRID_CAP);      // the rest of the bands are a grid-stride trip
    hipLaunchKernelGGL(matte_from_landmarks_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, pts_dev, N, K, offset, sim_dev,
                       contour, Kc, fallback_dev, radius, -0.5 / (sigma * sigma), softness, grow, matte_dev, Hs, Ws, band, bands, units);
    return spk::check_launch("matte_from_landmarks_kernel");
}

}  // extern "C"
