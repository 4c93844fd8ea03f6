// What the kernels of the aligned video edge share (csrc/frame_sim.hip: warp in, paste out; csrc/frame_blend.hip: the paste with a
// matte and a colour match, and the statistics of that match; csrc/frame_sim_nv12.hip: all of these on NV12 surfaces): how a row (a, c, tx, ty) is read and judged, the triangle, the
// clamped integer ranges and the bounding box of a row's region inside the frame.  Written once, so that the files agree on
// which pixels a row touches and on every weight, to the bit.
#pragma once

#include "frame_common.hpp"

namespace spk::frame {

constexpr double S_MIN = 1.0 / 16.0, S_MAX = 16.0;
constexpr int PASTE_WGS = 64;           // workgroups per frame of the way out (the host cannot see a device row's region)

struct Sim { double a, c, tx, ty, s; bool valid; };

__device__ __forceinline__ Sim load_sim(const float* __restrict__ sim, long long n) {
    Sim m;
    m.a = (double)sim[4 * n], m.c = (double)sim[4 * n + 1], m.tx = (double)sim[4 * n + 2], m.ty = (double)sim[4 * n + 3];
    m.s = sqrt(m.a * m.a + m.c * m.c);
    m.valid = isfinite(m.a) && isfinite(m.c) && isfinite(m.tx) && isfinite(m.ty) && m.s >= S_MIN && m.s <= S_MAX;
    return m;
}

__device__ __forceinline__ double tri(double t) { return fmax(0.0, 1.0 - fabs(t)); }

// The integers i with v_lo <= i <= v_hi, cut to [0, n): first = ceil(v_lo) and last = floor(v_hi) are clamped while still
// doubles and only then become ints, so no value overflows; an empty range has first > last.  The callers' bounds are where a
// triangle reaches zero, so an integer a rounding leaves out had a weight of the size of that rounding.
__device__ __forceinline__ void int_range(double v_lo, double v_hi, int n, int& first, int& last) {
    first = (int)fmin(fmax(ceil(v_lo), 0.0), (double)n);
    last = (int)fmin(fmax(floor(v_hi), -1.0), (double)(n - 1));
}

// The bounding box, inside the H x W frame, of the region sim([0, Ws) x [0, Hs)) of a valid row; empty: x_lo > x_hi or y_lo > y_hi.
struct RegionBox { int x_lo, x_hi, y_lo, y_hi; };

__device__ __forceinline__ RegionBox region_box(const Sim& m, int Hs, int Ws, int H, int W) {
    // the corners of the region in the frame
    const double cx[4] = {m.tx, m.a * Ws + m.tx, -m.c * Hs + m.tx, m.a * Ws - m.c * Hs + m.tx};
    const double cy[4] = {m.ty, m.c * Ws + m.ty, m.a * Hs + m.ty, m.c * Ws + m.a * Hs + m.ty};
    const double min_x = fmin(fmin(cx[0], cx[1]), fmin(cx[2], cx[3])), max_x = fmax(fmax(cx[0], cx[1]), fmax(cx[2], cx[3]));
    const double min_y = fmin(fmin(cy[0], cy[1]), fmin(cy[2], cy[3])), max_y = fmax(fmax(cy[0], cy[1]), fmax(cy[2], cy[3]));
    // pixel centres X + 0.5 in [min, max] with a pixel of slack on both sides (the region test decides), inside the frame
    RegionBox b;
    int_range(min_x - 1.5, max_x + 0.5, W, b.x_lo, b.x_hi);
    int_range(min_y - 1.5, max_y + 0.5, H, b.y_lo, b.y_hi);
    return b;
}

}  // namespace spk::frame
