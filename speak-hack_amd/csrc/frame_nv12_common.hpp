// What the NV12 kernels of the video-frame edge share (csrc/frame_nv12.hip and, on three planes, csrc/frame_i420.hip: boxes through
// host-built tables, the kernels of csrc/frame_nv12_axis_common.hpp; csrc/frame_sim_nv12.hip:
// aligned crops through a similarity transform per frame; csrc/frame_i420_common.hpp: the same crops on three planes): the 3 x 4 colour maps and how a row of one is applied, the primaries of
// a standard, and the checks every surface argument gets.  Written once, so that the two files agree on every colour coefficient
// and on the order of every operation, to the bit; each file still links alone (the host functions are inline).
#pragma once

#include "frame_common.hpp"

namespace spk::frame {

struct Mat34 { double m[12]; };     // three rows [a0 a1 a2 offset], byte units

// row c of a 3 x 4 affine map applied to (p0, p1, p2, 1): one fp64 fma chain that starts from the offset
__device__ __forceinline__ double affine_row(const Mat34& M, int c, double p0, double p1, double p2) {
    return fma(M.m[4 * c + 2], p2, fma(M.m[4 * c + 1], p1, fma(M.m[4 * c], p0, M.m[4 * c + 3])));
}

// What one tap and one pixel of a Y, U, V surface are worth, for every layout of the three fields (interleaved chroma: Nv12Taps
// below; three planes: I420Taps of csrc/frame_i420_common.hpp): the three fma of a tap, the matrix and the clamp behind the means,
// the background of a region pixel.  Written once, so that the layouts agree to the bit: a layout holds which loads bring l, u, v.
// Policy: the deriving struct, which holds to_rgb (a Mat34).
template <class Policy>
struct YuvTaps {
    __device__ __forceinline__ static void add_tap(double w, unsigned l, unsigned u, unsigned v, double& a_y, double& a_u, double& a_v) {
        a_y = fma(w, (double)l, a_y);
        a_u = fma(w, (double)u, a_u);
        a_v = fma(w, (double)v, a_v);
    }
    __device__ __forceinline__ void rgb(double y, double u, double v, double (&val)[3]) const {
        const Mat34& to_rgb = static_cast<const Policy*>(this)->to_rgb;
#pragma unroll
        for (int c = 0; c < 3; ++c) val[c] = fmin(fmax(affine_row(to_rgb, c, y, u, v), 0.0), 255.0);
    }
    // the pixel with the bytes (l, u, v) as R, G, B
    __device__ __forceinline__ void background_of(unsigned l, unsigned u, unsigned v, double (&b)[3]) const { rgb((double)l, (double)u, (double)v, b); }
};

// How the bytes of a surface become the sums of the way in and the background of the statistics, for every policy that says where
// a surface is (csrc/frame_sim_nv12.hip: planes and strides; csrc/frame_table_nv12.hip: an entry of a device table), as RgbTaps of
// csrc/frame_sim_common.hpp is for packed bytes.  The way in: the three sums run over Y[iy][ix], U[iy >> 1][ix >> 1] and
// V[iy >> 1][ix >> 1]; luma is byte loads, a (U, V) pair is one 16-bit load that stays in a register while ix >> 1 does not change,
// so it serves the two taps above it; the matrix and the clamp follow the means.  The statistics: the background of a region pixel
// is what the way in makes of that pixel, by network channel.  The arithmetic is YuvTaps'.
struct Nv12Row { const uint8_t* y; const uint8_t* c; unsigned pair; };

template <class Policy>
struct Nv12Taps : YuvTaps<Policy> {
    using Row = Nv12Row;
    // row iy of a frame whose planes begin at y and uv
    __device__ __forceinline__ static Row open_row(const uint8_t* y, long long y_row_stride, const uint8_t* uv, long long uv_row_stride, int iy) {
        return {y + (long long)iy * y_row_stride, uv + (long long)(iy >> 1) * uv_row_stride, 0u};
    }
    __device__ __forceinline__ void tap(Row& r, int ix, bool first, double w, double& a_y, double& a_u, double& a_v) const {
        if (first || !(ix & 1)) r.pair = *reinterpret_cast<const uint16_t*>(r.c + (ix & ~1));       // sample ix >> 1
        this->add_tap(w, r.y[ix], r.pair & 0xffu, r.pair >> 8, a_y, a_u, a_v);
    }
    // pixel (Y, X) of a frame whose planes begin at y and uv, as R, G, B
    __device__ __forceinline__ void background(const uint8_t* y, long long y_row_stride, const uint8_t* uv, long long uv_row_stride, int X, int Y,
                                               double (&b)[3]) const {
        const unsigned l = y[(long long)Y * y_row_stride + X];
        const unsigned pair = *reinterpret_cast<const uint16_t*>(uv + (long long)(Y >> 1) * uv_row_stride + (X & ~1));
        this->background_of(l, pair & 0xffu, pair >> 8, b);
    }
};

// (Kr, Kb) of a standard; false: unknown
inline bool primaries(int standard, double* kr, double* kb) {
    if (standard == 601) { *kr = 0.299; *kb = 0.114; return true; }
    if (standard == 709) { *kr = 0.2126; *kb = 0.0722; return true; }
    return false;
}

inline void yuv_coeffs(double kr, double kb, bool full, double* to_rgb, double* from_rgb) {
    const double kg = 1.0 - kr - kb;
    const double sy = full ? 1.0 : 219.0 / 255.0, sc = full ? 1.0 : 224.0 / 255.0, oy = full ? 0.0 : 16.0;
    if (from_rgb) {
        const double cb = sc / (2.0 * (1.0 - kb)), cr = sc / (2.0 * (1.0 - kr));
        const double f[12] = {sy * kr, sy * kg, sy * kb, oy,
                              -kr * cb, -kg * cb, (1.0 - kb) * cb, 128.0,
                              (1.0 - kr) * cr, -kg * cr, -kb * cr, 128.0};
        std::copy(f, f + 12, from_rgb);
    }
    if (to_rgb) {
        const double ay = 1.0 / sy, rv = 2.0 * (1.0 - kr) / sc, bu = 2.0 * (1.0 - kb) / sc;
        const double gu = -kb * bu / kg, gv = -kr * rv / kg;
        const double t[12] = {ay, 0.0, rv, -(ay * oy + 128.0 * rv),
                              ay, gu, gv, -(ay * oy + 128.0 * (gu + gv)),
                              ay, bu, 0.0, -(ay * oy + 128.0 * bu)};
        std::copy(t, t + 12, to_rgb);
    }
}

// the two maps of a standard, either pointer may be null; refuses what spk_yuv_coeffs refuses (for the files that link without
// csrc/frame_nv12.hip, which defines that one)
inline int colour_maps(const char* who, int standard, int full_range, double* to_rgb, double* from_rgb) {
    double kr, kb;
    SPK_REQUIRE(primaries(standard, &kr, &kb), "%s: standard must be 601 or 709 (got %d)", who, standard);
    SPK_REQUIRE(full_range == 0 || full_range == 1, "%s: full_range must be 0 or 1 (got %d)", who, full_range);
    yuv_coeffs(kr, kb, full_range != 0, to_rgb, from_rgb);
    return SPK_OK;
}

// the checks every NV12 surface argument gets; 0: fine
inline int check_surface(const char* who, const void* y, int64_t y_image_stride, int64_t y_row_stride, const void* uv, int64_t uv_image_stride,
                         int64_t uv_row_stride, int N, int H, int W, bool written) {
    SPK_REQUIRE(y && uv, "%s: null plane pointer", who);
    SPK_REQUIRE(N >= 1 && H >= 2 && W >= 2, "%s: N must be >= 1 and H, W >= 2 (N %d, %d x %d)", who, N, H, W);
    SPK_REQUIRE(H % 2 == 0 && W % 2 == 0, "%s: NV12 frames have an even height and width (got %d x %d)", who, H, W);
    SPK_REQUIRE((uintptr_t)uv % 2 == 0, "%s: the UV plane must be 2-byte aligned", who);
    SPK_REQUIRE(uv_row_stride % 2 == 0 && uv_image_stride % 2 == 0, "%s: the UV strides must be even (row %lld, image %lld)", who,
                (long long)uv_row_stride, (long long)uv_image_stride);
    SPK_REQUIRE(y_row_stride >= (long long)W, "%s: Y row stride %lld is smaller than W = %d", who, (long long)y_row_stride, W);
    SPK_REQUIRE(uv_row_stride >= (long long)W, "%s: UV row stride %lld is smaller than the row's %d bytes", who, (long long)uv_row_stride, W);
    if (written) {
        SPK_REQUIRE(N == 1 || (y_image_stride >= (long long)(H - 1) * y_row_stride + W && uv_image_stride >= (long long)(H / 2 - 1) * uv_row_stride + W),
                    "%s: image strides %lld / %lld make the frames overlap (%d rows of stride %lld / %lld)", who, (long long)y_image_stride,
                    (long long)uv_image_stride, H, (long long)y_row_stride, (long long)uv_row_stride);
    } else {
        SPK_REQUIRE(y_image_stride >= 0 && uv_image_stride >= 0, "%s: negative image stride", who);
    }
    return SPK_OK;
}

}  // namespace spk::frame
