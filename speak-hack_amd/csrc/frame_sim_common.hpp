// What the kernels of the aligned video edge share (csrc/frame_sim.hip: warp in, paste out; csrc/frame_blend.hip: the paste with a
// matte and a colour match, and the statistics of that match; csrc/frame_sim_nv12.hip: all of these on NV12 surfaces): how a row
// (a, c, tx, ty) is read and judged, the triangle, the clamped integer ranges, the bounding box of a row's region inside the frame;
// the one device function every per-pixel quantity of the paste comes from, and the paste into packed frames; and the way in, a
// kernel over a format's Source.  Written once, so that the files agree on which pixels a row touches and on every weight, to the
// bit: a format's file holds where its bytes are read and written.
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

// ---- where a frame is: the size and the byte addresses of frame n come from the format's policy ----
// Every policy of this edge (a Source of the way in, a Background of the statistics, a Target of the paste) answers frame(n, H, W)
// with what it needs to address frame n -- at least its size H x W and usable() -- once per frame, outside the pixel loops.  The
// strided formats (packed frames, NV12 planes) hold one size for the launch: their answer is the launch's H and W, always usable,
// and their addresses stay functions of n and the launch's strides.  A tabled format loads entry n of a device table instead
// (csrc/frame_table.hip); a frame that is not usable() is treated exactly like an invalid row.
struct LaunchFrame {
    int H, W;
    __device__ __forceinline__ bool usable() const { return true; }
};

// Packed pixels: three byte loads per tap of the way in, the three means are R, G, B as they stand; the background of a region
// pixel by network channel.
struct RgbTaps {
    __device__ __forceinline__ void tap(const uint8_t* p, int ix, bool, double w, double& a0, double& a1, double& a2) const {
        a0 = fma(w, (double)p[3 * ix], a0);
        a1 = fma(w, (double)p[3 * ix + 1], a1);
        a2 = fma(w, (double)p[3 * ix + 2], a2);
    }
    __device__ __forceinline__ void rgb(double m0, double m1, double m2, double (&val)[3]) const { val[0] = m0, val[1] = m1, val[2] = m2; }
};

__device__ __forceinline__ void rgb_background(const uint8_t* bg, int swap_rb, double (&b)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = (double)bg[swap_rb ? 2 - c : c];
}

// The paste's target in packed frames addressed by byte strides: out.pixel(frame, n, X, Y) is where pixel (Y, X) of frame n lives.
struct RgbTarget {
    uint8_t* dst;
    long long image_stride, row_stride;
    __device__ __forceinline__ LaunchFrame frame(long long, int H, int W) const { return {H, W}; }
    __device__ __forceinline__ uint8_t* pixel(const LaunchFrame&, long long n, int X, int Y) const {
        return dst + n * image_stride + (long long)Y * row_stride + (long long)X * 3;
    }
};

// ---- the way out: every per-pixel quantity of the aligned paste, and the paste into packed frames ----
struct PixelConsts { double is2, r, ir, fe; };

__device__ __forceinline__ PixelConsts pixel_consts(const Sim& m, double feather) {
    return {1.0 / (m.s * m.s), fmax(1.0, 1.0 / m.s), 1.0 / fmax(1.0, 1.0 / m.s), 1.0 / (feather + 1.0)};
}

// Frame pixel (Y, X) of a frame with the valid row m: nothing happens when the pixel is outside the region; inside it,
// body(q, mm) is called with q[c], the unmatched quantised value of network channel c (fp32, not rounded), and mm = a_u a_v Mt.
// img: the frame's first source plane; mt: the frame's matte (Hs x Ws) or NULL (Mt = 1).  The matte sum runs beside the channel
// sums, over the same taps in the same order.
template <class Body>
__device__ __forceinline__ void with_region_pixel(const Sim& m, const PixelConsts& pc, int X, int Y, const float* __restrict__ img, long long plane,
                                                  int Hs, int Ws, const float* __restrict__ mt, float lo, float k, Body&& body) {
    const double is2 = pc.is2, r = pc.r, ir = pc.ir, fe = pc.fe;
    const double dx = (X + 0.5) - m.tx, dy = (Y + 0.5) - m.ty;
    const double u = (m.a * dx + m.c * dy) * is2, v = (-m.c * dx + m.a * dy) * is2;
    if (!(u >= 0.0 && u < (double)Ws && v >= 0.0 && v < (double)Hs)) return;
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
    double mm = a_u * a_v;
    if (mt) mm *= fmin(fmax(vm / norm, 0.0), 1.0);                // fmax returns its other operand for a NaN: clamp01(NaN) = 0
    float q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = quant_unrounded((float)val[c], lo, k);
    body(q, mm);
}

// The same as a question: false when the pixel is outside the region, else true with q and mm filled in.
__device__ __forceinline__ bool region_pixel(const Sim& m, const PixelConsts& pc, int X, int Y, const float* __restrict__ img, long long plane,
                                             int Hs, int Ws, const float* __restrict__ mt, float lo, float k, float (&q)[3], double& mm) {
    bool inside = false;
    with_region_pixel(m, pc, X, Y, img, plane, Hs, Ws, mt, lo, k, [&](const float (&q_)[3], double mm_) {
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = q_[c];
        mm = mm_, inside = true;
    });
    return inside;
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

// The three bytes of a region pixel: the colour row of its frame applied to q when the frame is matched, then rint(b + m (q' - b)).
__device__ __forceinline__ void blend_pixel(uint8_t* out, int swap_rb, bool matched, const float (&g)[3], const float (&o)[3], const float (&q)[3],
                                            double mm) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int cd = swap_rb ? 2 - c : c;
        const float qc = matched ? fminf(fmaxf(fmaf(g[c], q[c], o[c]), 0.f), 255.f) : q[c];
        const double b = (double)out[cd];
        out[cd] = (uint8_t)(int)rint(fma(mm, (double)qc - b, b));         // m in [0, 1], q' and b in [0, 255]: so is the result
    }
}

// The paste into packed frames.  blockIdx.y walks the frames, the PASTE_WGS workgroups of blockIdx.x share one frame: each derives
// the bounding box of the region sim([0, Ws) x [0, Hs)) inside the frame from the row and strides over its pixels (x fastest).  A
// pixel that region_pixel holds -- at most 2 x 2 taps when the crop enlarges, (2 / s)^2 when it shrinks -- reads the background
// byte it is about to overwrite, and no other, and stores rint(b + m (q' - b)) in fp64.  SEAMLESS: matte and colour may be given
// (either may be NULL: csrc/frame_blend.hip); false: they are absent at compile time, and what is left is the plain paste of
// csrc/frame_sim.hip, with the registers of a kernel that never had them.  The plain instance hands its store to the pixel
// function and the seamless one asks it: the same arithmetic, and the form in which each compiles to the code it had as a kernel
// of its own (asked, the plain instance is 15 instructions longer and 6 % slower).  Target: where the frames are (RgbTarget: byte
// strides; csrc/frame_table.hip: a device table); the launch's H and W are what a strided target answers with.
template <bool SEAMLESS, class Target>
__global__ __launch_bounds__(256) void frames_paste_u8_sim_kernel(const float* __restrict__ src, int N, int Hs, int Ws, Target out_frames, int H,
                                                                  int W, const float* __restrict__ sim, int swap_rb, double feather, float lo, float k,
                                                                  const float* __restrict__ matte, int matte_frames,
                                                                  const float* __restrict__ colour) {
    const long long plane = (long long)Hs * Ws;
    for (long long n = blockIdx.y; n < N; n += gridDim.y) {
        const Sim m = load_sim(sim, n);
        if (!m.valid) continue;
        const auto fr = out_frames.frame(n, H, W);
        if (!fr.usable()) continue;
        const RegionBox box = region_box(m, Hs, Ws, fr.H, fr.W);
        const int x_lo = box.x_lo, x_hi = box.x_hi, y_lo = box.y_lo, y_hi = box.y_hi;
        if (x_lo > x_hi || y_lo > y_hi) continue;
        const long long bw = x_hi - x_lo + 1, total = bw * (y_hi - y_lo + 1);
        const PixelConsts pc = pixel_consts(m, feather);
        const float* img = src + n * 3 * plane;
        const float* mt = SEAMLESS && matte ? matte + (matte_frames > 1 ? n : 0) * plane : nullptr;
        const bool matched = SEAMLESS && colour;
        float g[3], o[3];
        load_colour(matched ? colour : nullptr, n, g, o);
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const int X = x_lo + (int)(idx % bw), Y = y_lo + (int)(idx / bw);
            const auto out = out_frames.pixel(fr, n, X, Y);      // what blend_pixel writes: packed bytes, or a format's own pixel
            if constexpr (SEAMLESS) {
                float q[3];
                double mm;
                if (!region_pixel(m, pc, X, Y, img, plane, Hs, Ws, mt, lo, k, q, mm)) continue;
                blend_pixel(out, swap_rb, matched, g, o, q, mm);
            } else {
                with_region_pixel(m, pc, X, Y, img, plane, Hs, Ws, mt, lo, k,
                                  [&](const float (&q)[3], double mm) { blend_pixel(out, swap_rb, false, g, o, q, mm); });
            }
        }
    }
}

// ---- the way in ----
constexpr int TILE = 8;                 // a wave of the way in covers a TILE x TILE block of outputs: neighbouring footprints overlap

// The way in.  Lane l of a wave owns output (8 ty + (l >> 3), 8 tx + (l & 7)) of tile (ty, tx) of one frame, all three channels.
// Its footprint is the square |e_u|, |e_v| < S = max(s, 1) around p = sim(ox + 0.5, oy + 0.5), rotated with the crop: it walks the
// bounding rows of that square inside the frame and, per row, the pixels between the two pairs of edges (intersected before the
// loop: no tap of weight zero is loaded).  Weights and sums are fp64; no LDS, no scratch.
// Source: where a format's bytes are read.  in.frame(n, H, W) is frame n (above); in.row(frame, n, iy) opens its row iy;
// in.tap(row, ix, first, w, a0, a1, a2) adds tap ix of that row, of weight w, to the three sums (first: the row's first tap; taps
// come with ix rising); in.rgb(m0, m1, m2, val) makes R, G, B in byte units of the three means.  Everything else is the same code
// for every format.
template <class Source>
__global__ __launch_bounds__(256) void frames_to_f32_sim_kernel(Source in, int H, int W, const float* __restrict__ sim, int swap_rb,
                                                                float* __restrict__ dst, int Hout, int Wout, int tiles_y, int tiles_x,
                                                                long long tiles, Affine3 af) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long tile = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); tile < tiles; tile += waves) {
        const int ox = (int)(tile % tiles_x) * TILE + (lane & 7);
        const int oy = (int)((tile / tiles_x) % tiles_y) * TILE + (lane >> 3);
        const long long n = tile / ((long long)tiles_x * tiles_y);
        if (ox >= Wout || oy >= Hout) continue;
        const Sim m = load_sim(sim, n);
        const auto fr = in.frame(n, H, W);                        // n is the wave's: one answer per tile
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, wt = 0.0;
        if (m.valid && fr.usable()) {
            const double u = ox + 0.5, v = oy + 0.5;
            const double px = m.a * u - m.c * v + m.tx, py = m.c * u + m.a * v + m.ty;
            const double S = fmax(m.s, 1.0);
            const double ia = m.a / (m.s * S), ic = m.c / (m.s * S);              // t_u = ia dx + ic dy,  t_v = -ic dx + ia dy
            const double ext = S * (fabs(m.a) + fabs(m.c)) / m.s;                // half the bounding box of the rotated square
            int y_lo, y_hi;
            int_range(py - ext - 0.5, py + ext - 0.5, fr.H, y_lo, y_hi);            // pixel centres iy + 0.5 within ext of py
            for (int iy = y_lo; iy <= y_hi; ++iy) {
                const double dy = (iy + 0.5) - py;
                // |ia dx + ic dy| < 1 and |-ic dx + ia dy| < 1 as intervals of dx, inside the bounding box
                double d_lo = -ext, d_hi = ext;
                if (ia != 0.0) {
                    const double r0 = (-1.0 - ic * dy) / ia, r1 = (1.0 - ic * dy) / ia;
                    d_lo = fmax(d_lo, fmin(r0, r1)), d_hi = fmin(d_hi, fmax(r0, r1));
                }
                if (ic != 0.0) {
                    const double r0 = (ia * dy - 1.0) / ic, r1 = (ia * dy + 1.0) / ic;
                    d_lo = fmax(d_lo, fmin(r0, r1)), d_hi = fmin(d_hi, fmax(r0, r1));
                }
                int x_lo, x_hi;
                int_range(px + d_lo - 0.5, px + d_hi - 0.5, fr.W, x_lo, x_hi);
                auto row = in.row(fr, n, iy);
                for (int ix = x_lo; ix <= x_hi; ++ix) {
                    const double dx = (ix + 0.5) - px;
                    const double w = tri(fma(ia, dx, ic * dy)) * tri(fma(-ic, dx, ia * dy));
                    wt += w;
                    in.tap(row, ix, ix == x_lo, w, acc0, acc1, acc2);
                }
            }
        }
        double val[3] = {0.0, 0.0, 0.0};                          // an invalid row, or a footprint wholly outside the frame: V = 0
        if (wt > 0.0) in.rgb(acc0 / wt, acc1 / wt, acc2 / wt, val);
        const long long plane = (long long)Hout * Wout;
        float* out = dst + n * 3 * plane + (long long)oy * Wout + ox;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int cd = swap_rb ? 2 - c : c;                  // network channel c lands in plane cd
            out[cd * plane] = (float)fma((double)af.scale[cd], val[c], (double)af.shift[cd]);
        }
    }
}

// ---- host ----
// the launch of the way in over the checked arguments of a format's entry point
template <class Source>
int launch_frames_to_f32_sim(const char* kernel, const Source& in, int N, int H, int W, const float* sim_dev, int swap_rb, float* dst, int Hout,
                             int Wout, const Affine3& af, void* stream) {
    const int tiles_y = spk::ceil_div(Hout, TILE), tiles_x = spk::ceil_div(Wout, TILE);
    const long long tiles = (long long)N * tiles_y * tiles_x;
    hipLaunchKernelGGL(frames_to_f32_sim_kernel<Source>, grid_for(tiles * 64), dim3(256), 0, (hipStream_t)stream, in, H, W, sim_dev, swap_rb, dst,
                       Hout, Wout, tiles_y, tiles_x, tiles, af);
    return spk::check_launch(kernel);
}

// the blend's arguments that do not depend on the pixel format (pointers, sizes and strides are the format's to check)
inline int check_blend_params(const char* who, int N, double feather, float lo, float k, const float* matte_dev, int matte_frames) {
    SPK_REQUIRE(std::isfinite(feather) && feather >= 0.0, "%s: feather must be a finite number >= 0 (got %g)", who, feather);
    if (int rc = check_range(who, lo, k)) return rc;
    SPK_REQUIRE(matte_dev ? (matte_frames == 1 || matte_frames == N) : matte_frames == 0,
                "%s: matte_frames must be 1 or N = %d with a matte and 0 without one (got %d)", who, N, matte_frames);
    return SPK_OK;
}

// what the entry points of the packed paste and its statistics check alike
inline int check_paste_u8(const char* who, const void* src, const void* dst, const float* sim_dev, int N, int Hs, int Ws, int64_t image_stride,
                          int64_t row_stride, int H, int W, double feather, float lo, float k, const float* matte_dev, int matte_frames) {
    SPK_REQUIRE(src && dst, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(N >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1, "%s: N / H / W must be >= 1 (N %d, source %d x %d, frame %d x %d)", who, N,
                Hs, Ws, H, W);
    SPK_REQUIRE(row_stride >= 3ll * W, "%s: row stride %lld is smaller than 3 * W = %lld", who, (long long)row_stride, 3ll * W);
    SPK_REQUIRE(N == 1 || image_stride >= (long long)(H - 1) * row_stride + 3ll * W,
                "%s: image stride %lld makes the frames overlap (%d rows of stride %lld)", who, (long long)image_stride, H, (long long)row_stride);
    return check_blend_params(who, N, feather, lo, k, matte_dev, matte_frames);
}

// the launch of the paste into a target's frames over checked arguments (H, W: the launch's size, which a tabled target ignores)
template <bool SEAMLESS, class Target>
int launch_paste_sim(const char* kernel, const float* src, int N, int Hs, int Ws, const Target& out_frames, int H, int W, const float* sim_dev,
                     int swap_rb, double feather, float lo, float k, const float* matte_dev, int matte_frames, const float* colour_dev,
                     void* stream) {
    hipLaunchKernelGGL((frames_paste_u8_sim_kernel<SEAMLESS, Target>), dim3(PASTE_WGS, (unsigned)std::min(N, 65535)), dim3(256), 0,
                       (hipStream_t)stream, src, N, Hs, Ws, out_frames, H, W, sim_dev, swap_rb, feather, lo, k, matte_dev, matte_frames, colour_dev);
    return spk::check_launch(kernel);
}

// ... into packed frames addressed by byte strides
template <bool SEAMLESS>
int launch_paste_u8_sim(const char* kernel, const float* src, int N, int Hs, int Ws, uint8_t* dst, int64_t image_stride, int64_t row_stride, int H,
                        int W, const float* sim_dev, int swap_rb, double feather, float lo, float k, const float* matte_dev, int matte_frames,
                        const float* colour_dev, void* stream) {
    return launch_paste_sim<SEAMLESS>(kernel, src, N, Hs, Ws, RgbTarget{dst, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride}, H, W,
                                      sim_dev, swap_rb, feather, lo, k, matte_dev, matte_frames, colour_dev, stream);
}

}  // namespace spk::frame
