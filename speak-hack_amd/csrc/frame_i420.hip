// The axis-aligned video-frame edge on I420 surfaces (include/spk.h has the definitions): what csrc/frame_nv12.hip does for a
// hardware decoder's surfaces, for what a software decoder / encoder and WebRTC's frame buffer hold -- a Y plane and a U and a V
// plane at half resolution, each with a base address and a pitch of its own, chroma sited by replication -- without interleaving
// the chroma into a scratch NV12 surface and splitting it again.
//   frames_i420_to_f32:  the way in of frames_nv12_to_f32 (boxes through host-built tables, origins by value or per frame);
//   frames_paste_i420:   its paste, one thread per chroma block (2 x 2 luma pixels, one U byte, one V byte);
//   frames_f32_to_i420:  the whole-frame case without tables.
// This file holds where the chroma bytes of a surface are read and written and nothing else: the kernels are the templates the NV12
// file instantiates (csrc/frame_nv12_axis_common.hpp), the colour maps are csrc/frame_nv12_common.hpp's, the surface checks and the
// byte-wise chroma access csrc/frame_i420_common.hpp's.  So an I420 surface and the NV12 surface with the same Y bytes and
// UV[cy][cx] = (U[cy][cx], V[cy][cx]) give the same fp32 bits and the same bytes.  Chroma is loaded and stored as bytes: no plane
// needs an alignment or an even pitch, and V may come before U.  H and W are even, so frame pixel (Y, X) has its chroma sample
// (Y >> 1, X >> 1) inside both chroma planes and a chroma block lies wholly inside the frame: the clamps of the shared kernels keep
// every load and store of this file in bounds.  Links without any other file.
#include "frame_i420_common.hpp"
#include "frame_nv12_axis_common.hpp"

namespace {

using namespace spk::frame;

// Where the chroma of an I420 surface is: the way in does one byte load from U and one from V at X >> 1 when the sample changes
// and keeps them in registers for the tap above the same sample (the rule of I420Taps::tap); the paste reads and writes one byte
// in each of U and V (PlanarPair).
struct I420Surface {
    AxisPlane y, u, v;
    struct Row { const uint8_t* u; const uint8_t* v; unsigned cu, cv; };
    __device__ __forceinline__ Row chroma_row(long long n, long long cy) const {
        return {u.p + n * u.image_stride + cy * u.row_stride, v.p + n * v.image_stride + cy * v.row_stride, 0u, 0u};
    }
    __device__ __forceinline__ static void tap(Row& r, int X, bool first, unsigned& cu, unsigned& cv) {
        if (first || !(X & 1)) r.cu = r.u[X >> 1], r.cv = r.v[X >> 1];
        cu = r.cu, cv = r.cv;
    }
    __device__ __forceinline__ static uint8_t* at(const AxisPlane& q, long long n, long long CY, long long CX) {
        return q.p + n * q.image_stride + CY * q.row_stride + CX;
    }
    __device__ __forceinline__ void load_chroma(long long n, long long CY, long long CX, unsigned& cu, unsigned& cv) const {
        PlanarPair::load(at(u, n, CY, CX), at(v, n, CY, CX), cu, cv);
    }
    __device__ __forceinline__ void store_chroma(long long n, long long CY, long long CX, unsigned cu, unsigned cv) const {
        PlanarPair::store(at(u, n, CY, CX), at(v, n, CY, CX), cu, cv);
    }
};

struct Planes {                         // the nine surface arguments of an entry point
    const uint8_t* y; int64_t y_image_stride, y_row_stride;
    const uint8_t* u; int64_t u_image_stride, u_row_stride;
    const uint8_t* v; int64_t v_image_stride, v_row_stride;
    int check(const char* who, int N, int H, int W, bool written) const {
        return check_planar_surface(who, y, y_image_stride, y_row_stride, u, u_image_stride, u_row_stride, v, v_image_stride, v_row_stride, N, H, W,
                                    written);
    }
    I420Surface surface(int N) const {
        return {axis_plane(y, y_image_stride, y_row_stride, N), axis_plane(u, u_image_stride, u_row_stride, N),
                axis_plane(v, v_image_stride, v_row_stride, N)};
    }
};

}  // namespace

extern "C" {

int spk_frames_i420_to_f32(const uint8_t* y, int64_t y_image_stride, int64_t y_row_stride, const uint8_t* u, int64_t u_image_stride,
                           int64_t u_row_stride, const uint8_t* v, int64_t v_image_stride, int64_t v_row_stride, int N, int H, int W,
                           const int32_t* boxes_yx, int y0, int x0, int Hin, int Win, int swap_rb, int standard, int full_range,
                           const int32_t* first_y, const int32_t* count_y, const float* w_y, int taps_y, const int32_t* first_x,
                           const int32_t* count_x, const float* w_x, int taps_x, float* dst, int Hout, int Wout, float scale0, float scale1,
                           float scale2, float shift0, float shift1, float shift2, void* stream) {
    const char* who = "frames_i420_to_f32";
    const ResizeTables t = {first_y, count_y, w_y, first_x, count_x, w_x, taps_y, taps_x};
    const Planes s = {y, y_image_stride, y_row_stride, u, u_image_stride, u_row_stride, v, v_image_stride, v_row_stride};
    if (int rc = s.check(who, N, H, W, false)) return rc;
    if (int rc = check_axis_in(who, dst, t, H, W, Hin, Win, Hout, Wout)) return rc;
    Mat34 M;
    if (int rc = colour_maps(who, standard, full_range, M.m, nullptr)) return rc;
    return launch_axis_in("frames_nv12_to_f32_kernel<i420>", s.surface(N), N, H, W, boxes_yx, y0, x0, Hin, Win, swap_rb, t, dst, Hout, Wout,
                          Affine3{{scale0, scale1, scale2}, {shift0, shift1, shift2}}, M, stream);
}

int spk_frames_paste_i420(const float* src, int N, int Hs, int Ws, uint8_t* y, int64_t y_image_stride, int64_t y_row_stride, uint8_t* u,
                          int64_t u_image_stride, int64_t u_row_stride, uint8_t* v, int64_t v_image_stride, int64_t v_row_stride, int H, int W,
                          int h, int w, int y0, int x0, const int32_t* boxes_yx, int standard, int full_range, const int32_t* first_y,
                          const int32_t* count_y, const float* w_y, int taps_y, const int32_t* first_x, const int32_t* count_x, const float* w_x,
                          int taps_x, const float* a_y, const float* a_x, float lo, float k, void* stream) {
    const char* who = "frames_paste_i420";
    const ResizeTables t = {first_y, count_y, w_y, first_x, count_x, w_x, taps_y, taps_x};
    const Planes s = {y, y_image_stride, y_row_stride, u, u_image_stride, u_row_stride, v, v_image_stride, v_row_stride};
    SPK_REQUIRE(src, "%s: null frame pointer", who);
    if (int rc = s.check(who, N, H, W, true)) return rc;
    if (int rc = check_axis_paste(who, t, a_y, a_x, Hs, Ws, h, w, lo, k)) return rc;
    Mat34 M;
    if (int rc = colour_maps(who, standard, full_range, nullptr, M.m)) return rc;
    return launch_axis_paste("frames_paste_nv12_kernel<i420>", src, N, Hs, Ws, s.surface(N), H, W, h, w, y0, x0, boxes_yx, t, a_y, a_x, lo, k, M,
                             stream);
}

int spk_frames_f32_to_i420(const float* src, int N, int H, int W, uint8_t* y, int64_t y_image_stride, int64_t y_row_stride, uint8_t* u,
                           int64_t u_image_stride, int64_t u_row_stride, uint8_t* v, int64_t v_image_stride, int64_t v_row_stride, int standard,
                           int full_range, float lo, float k, void* stream) {
    const char* who = "frames_f32_to_i420";
    const Planes s = {y, y_image_stride, y_row_stride, u, u_image_stride, u_row_stride, v, v_image_stride, v_row_stride};
    SPK_REQUIRE(src, "%s: null frame pointer", who);
    if (int rc = s.check(who, N, H, W, true)) return rc;
    if (int rc = check_range(who, lo, k)) return rc;
    Mat34 M;
    if (int rc = colour_maps(who, standard, full_range, nullptr, M.m)) return rc;
    return launch_axis_whole("frames_paste_nv12_kernel<i420, whole frame>", src, N, H, W, s.surface(N), lo, k, M, stream);
}

}  // extern "C"
