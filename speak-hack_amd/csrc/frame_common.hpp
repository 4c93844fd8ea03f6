// What the kernels of the video-frame edge share, whatever the pixel format (csrc/frame_io.hip: packed RGB; csrc/frame_nv12.hip:
// NV12): the work decomposition of the table-driven resize, the window clamps, the fp64 separable sums, the fp32 quantise chain
// and the argument checks.  The bit-exactness contracts of the edge ("the same tables, the same order of additions",
// "frames_to_u8 of the fp32 result") rest on these being written once; a format's file holds where its bytes are read and written.
#pragma once

#include "spk_common.hpp"
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace spk::frame {

constexpr int STRIP = 8;            // output rows a thread of the resize owns
constexpr int GRID_CAP = 2048;      // workgroups per launch; the rest of the work is a grid-stride trip

struct Affine3 { float scale[3], shift[3]; };

struct ResizeTables {               // DEVICE copies of spk_resize_table's tables for both axes (fp32 weights, rows of taps_y / taps_x)
    const int *first_y, *count_y; const float* w_y;
    const int *first_x, *count_x; const float* w_x;
    int taps_y, taps_x;
};

// ---- device ----
// the tables are the caller's: clamp a window [first, first + count) into [0, n) so that no table can send a load out of bounds
__device__ __forceinline__ void clamp_window(int first, int count, int taps, int n, int& f, int& c) {
    f = min(max(first, 0), n - 1);
    c = max(min(min(count, taps), n - f), 0);
}

// The work item of the input kernels: output column ox of the STRIP-row strip at row oy0 of frame n, its clamped horizontal window
// [fx, fx + cx), the clamped vertical windows of its rows (cy = 0 for a row past Hout) and the input rows [row_lo, row_hi) they cover.
struct Strip {
    long long n;
    int ox, oy0, fx, cx, fy[STRIP], cy[STRIP], row_lo, row_hi;
};

__device__ __forceinline__ Strip strip_prologue(long long idx, const ResizeTables& t, int Hin, int Win, int Hout, int Wout, int strips) {
    Strip s;
    s.ox = (int)(idx % Wout);
    s.oy0 = (int)((idx / Wout) % strips) * STRIP;
    s.n = idx / ((long long)Wout * strips);
    clamp_window(t.first_x[s.ox], t.count_x[s.ox], t.taps_x, Win, s.fx, s.cx);
    s.row_lo = Hin, s.row_hi = 0;
#pragma unroll
    for (int k = 0; k < STRIP; ++k) {
        const int oy = min(s.oy0 + k, Hout - 1);
        clamp_window(t.first_y[oy], t.count_y[oy], t.taps_y, Hin, s.fy[k], s.cy[k]);
        if (s.oy0 + k >= Hout) s.cy[k] = 0;
        if (s.cy[k] > 0) { s.row_lo = min(s.row_lo, s.fy[k]); s.row_hi = max(s.row_hi, s.fy[k] + s.cy[k]); }
    }
    return s;
}

// the horizontal sums (h0, h1, h2) of input row iy, added into the accumulators of the strip's rows whose window holds the row
__device__ __forceinline__ void strip_accumulate(double (&acc)[STRIP][3], const Strip& s, const ResizeTables& t, int iy, double h0, double h1, double h2) {
#pragma unroll
    for (int k = 0; k < STRIP; ++k) {
        const int j = iy - s.fy[k];
        if ((unsigned)j < (unsigned)s.cy[k]) {
            const double w = (double)t.w_y[(long long)(s.oy0 + k) * t.taps_y + j];
            acc[k][0] = fma(w, h0, acc[k][0]);
            acc[k][1] = fma(w, h1, acc[k][1]);
            acc[k][2] = fma(w, h2, acc[k][2]);
        }
    }
}

// Pixel (y, x) of the resize of one fp32 CHW image (img: its first plane, Hs x Ws, the planes `plane` apart) in fp64: per source
// row the horizontal sum of each channel, then the vertical sum of those -- the sums of the input kernels, in their order.
__device__ __forceinline__ void resize_point(const float* __restrict__ img, long long plane, int Hs, int Ws, const ResizeTables& t, int y, int x,
                                             double& v0, double& v1, double& v2) {
    int fx, cx, fy, cy;
    clamp_window(t.first_x[x], t.count_x[x], t.taps_x, Ws, fx, cx);
    clamp_window(t.first_y[y], t.count_y[y], t.taps_y, Hs, fy, cy);
    const float* wx = t.w_x + (long long)x * t.taps_x;
    const float* wy = t.w_y + (long long)y * t.taps_y;
    const float* in = img + (long long)fy * Ws + fx;
    v0 = v1 = v2 = 0.0;
    for (int i = 0; i < cy; ++i) {
        const float* p = in + (long long)i * Ws;
        double h0 = 0.0, h1 = 0.0, h2 = 0.0;
        for (int j = 0; j < cx; ++j) {
            const double wj = (double)wx[j];
            h0 = fma(wj, (double)p[j], h0);
            h1 = fma(wj, (double)p[plane + j], h1);
            h2 = fma(wj, (double)p[2 * plane + j], h2);
        }
        const double wi = (double)wy[i];
        v0 = fma(wi, h0, v0);
        v1 = fma(wi, h1, v1);
        v2 = fma(wi, h2, v2);
    }
}

// min(max((x - lo) * k, 0), 255) in exactly this order of fp32 operations (a subtraction and a multiplication cannot contract
// into an FMA): torch's ((x - lo) * k).clamp(0, 255); with quant_u8's rounding the bits of its .round().to(torch.uint8).  fmaxf
// returns its other operand for a NaN: NaN -> 0.
__device__ __forceinline__ float quant_unrounded(float x, float lo, float k) {
    return fminf(fmaxf(__fmul_rn(__fsub_rn(x, lo), k), 0.f), 255.f);
}

__device__ __forceinline__ unsigned quant_u8(float x, float lo, float k) { return (unsigned)rintf(quant_unrounded(x, lo, k)); }  // ties to even

// the box origin of frame n: (y0, x0) by value or, with boxes_yx, frame n's pair of a device array
struct Origin { int y, x; };
__device__ __forceinline__ Origin box_origin(const int* __restrict__ boxes_yx, long long n, int y0, int x0) {
    return {boxes_yx ? boxes_yx[2 * n] : y0, boxes_yx ? boxes_yx[2 * n + 1] : x0};
}

// ---- host ----
inline dim3 grid_for(long long total) { return dim3((unsigned)std::min((total + 255) / 256, (long long)GRID_CAP)); }

inline int check_tables(const char* who, const ResizeTables& t) {
    SPK_REQUIRE(t.first_y && t.count_y && t.w_y && t.first_x && t.count_x && t.w_x, "%s: null table pointer", who);
    SPK_REQUIRE(t.taps_y >= 1 && t.taps_x >= 1, "%s: tap count must be >= 1 (got %d, %d)", who, t.taps_y, t.taps_x);
    return SPK_OK;
}

inline int check_range(const char* who, float lo, float k) {
    SPK_REQUIRE(std::isfinite(lo) && std::isfinite(k) && k > 0.f, "%s: the value range must be finite and increasing", who);
    return SPK_OK;
}

}  // namespace spk::frame
