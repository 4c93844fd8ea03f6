// What the I420 files share (csrc/frame_sim_i420.hip: aligned crops on N surfaces of one size behind three pointers and nine strides;
// csrc/frame_table_i420.hip: every surface an entry of a device table; csrc/frame_i420.hip: the axis-aligned edge, which takes
// PlanarPair and check_planar_surface from here): how the bytes of a three-plane surface are read, how a
// chroma block of one is written, and the checks every planar surface argument gets.  An I420 surface is the NV12 surface with the
// same Y bytes and UV[cy][cx] = (U[cy][cx], V[cy][cx]) behind another way to say where its bytes are: the arithmetic is YuvTaps'
// (csrc/frame_nv12_common.hpp), the kernels are the templates the NV12 files instantiate, so the two layouts agree to the bit.
// Chroma is read and written as BYTES, one load and one store per plane: a U or V plane may begin at an odd address and have an
// odd pitch (a packed plane of a width with W / 2 odd has one), which a 16-bit access could not follow.
#pragma once

#include "frame_nv12_common.hpp"

namespace spk::frame {

// How the bytes of a surface become the sums of the way in and the background of the statistics, as Nv12Taps does for interleaved
// chroma.  The way in: luma is byte loads; the U and V bytes of sample ix >> 1 are two byte loads that stay in registers while
// ix >> 1 does not change, so they serve the two taps above the sample.  Policy: the deriving struct, which holds to_rgb.
struct I420Row { const uint8_t* y; const uint8_t* u; const uint8_t* v; unsigned cu, cv; };

template <class Policy>
struct I420Taps : YuvTaps<Policy> {
    using Row = I420Row;
    // row iy of a frame whose planes begin at y, u and v
    __device__ __forceinline__ static Row open_row(const uint8_t* y, long long y_row_stride, const uint8_t* u, long long u_row_stride,
                                                   const uint8_t* v, long long v_row_stride, int iy) {
        return {y + (long long)iy * y_row_stride, u + (long long)(iy >> 1) * u_row_stride, v + (long long)(iy >> 1) * v_row_stride, 0u, 0u};
    }
    __device__ __forceinline__ void tap(Row& r, int ix, bool first, double w, double& a_y, double& a_u, double& a_v) const {
        if (first || !(ix & 1)) r.cu = r.u[ix >> 1], r.cv = r.v[ix >> 1];
        this->add_tap(w, r.y[ix], r.cu, r.cv, a_y, a_u, a_v);
    }
    // pixel (Y, X) of a frame whose planes begin at y, u and v, as R, G, B
    __device__ __forceinline__ void background(const uint8_t* y, long long y_row_stride, const uint8_t* u, long long u_row_stride, const uint8_t* v,
                                               long long v_row_stride, int X, int Y, double (&b)[3]) const {
        this->background_of(y[(long long)Y * y_row_stride + X], u[(long long)(Y >> 1) * u_row_stride + (X >> 1)],
                            v[(long long)(Y >> 1) * v_row_stride + (X >> 1)], b);
    }
};

// The (U, V) of a chroma sample whose bytes are at pu and pv: what load_chroma / store_chroma of a three-plane Target do
// (csrc/frame_sim_nv12_common.hpp has the kernel).  Lane l of a wave holds sample CX + l of a row: 64 consecutive bytes per plane.
struct PlanarPair {
    __device__ __forceinline__ static void load(const uint8_t* pu, const uint8_t* pv, unsigned& u, unsigned& v) { u = *pu, v = *pv; }
    __device__ __forceinline__ static void store(uint8_t* pu, uint8_t* pv, unsigned u, unsigned v) { *pu = (uint8_t)u, *pv = (uint8_t)v; }
};

// the checks every I420 surface argument gets, the counterpart of check_surface; 0: fine.  No alignment or parity is asked of a
// chroma plane; the planes may lie in any order and in separate allocations.
inline int check_planar_surface(const char* who, const void* y, int64_t y_image_stride, int64_t y_row_stride, const void* u, int64_t u_image_stride,
                                int64_t u_row_stride, const void* v, int64_t v_image_stride, int64_t v_row_stride, int N, int H, int W,
                                bool written) {
    SPK_REQUIRE(y && u && v, "%s: null plane pointer", who);
    SPK_REQUIRE(N >= 1 && H >= 2 && W >= 2, "%s: N must be >= 1 and H, W >= 2 (N %d, %d x %d)", who, N, H, W);
    SPK_REQUIRE(H % 2 == 0 && W % 2 == 0, "%s: I420 frames have an even height and width (got %d x %d)", who, H, W);
    SPK_REQUIRE(y_row_stride >= (long long)W, "%s: Y row stride %lld is smaller than W = %d", who, (long long)y_row_stride, W);
    SPK_REQUIRE(u_row_stride >= (long long)(W / 2), "%s: U row stride %lld is smaller than the row's %d bytes", who, (long long)u_row_stride, W / 2);
    SPK_REQUIRE(v_row_stride >= (long long)(W / 2), "%s: V row stride %lld is smaller than the row's %d bytes", who, (long long)v_row_stride, W / 2);
    if (written) {
        SPK_REQUIRE(N == 1 || (y_image_stride >= (long long)(H - 1) * y_row_stride + W &&
                               u_image_stride >= (long long)(H / 2 - 1) * u_row_stride + W / 2 &&
                               v_image_stride >= (long long)(H / 2 - 1) * v_row_stride + W / 2),
                    "%s: image strides %lld / %lld / %lld make the frames overlap (%d rows of stride %lld / %lld / %lld)", who, (long long)y_image_stride,
                    (long long)u_image_stride, (long long)v_image_stride, H, (long long)y_row_stride, (long long)u_row_stride, (long long)v_row_stride);
    } else {
        SPK_REQUIRE(y_image_stride >= 0 && u_image_stride >= 0 && v_image_stride >= 0, "%s: negative image stride", who);
    }
    return SPK_OK;
}

}  // namespace spk::frame
