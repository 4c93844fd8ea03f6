// The video-frame edge in NV12 form: what a hardware decoder / encoder holds in device memory -- a full-resolution Y plane and a
// half-resolution interleaved UV plane, each with its own row pitch -- in and out of the network without a packed-RGB detour.
//   frames_nv12_to_f32: crop (origin by value or per frame from a device array) + antialiased bilinear resize of the three
//   component fields + YUV -> RGB + normalise -> CHW, one pass, no scratch;
//   frames_paste_nv12: resize to the box + quantise + RGB -> YUV + feather-blend into the surface the box came from, one pass,
//   one thread per chroma block (2 x 2 luma pixels); frames_f32_to_nv12 is its whole-frame case without tables.
// Definitions (siting, colour matrices, the order of every operation) are in include/spk.h.  The resize tables are those of
// csrc/frame_io.hip (spk_resize_table, spk_feather_table): this file holds no filter arithmetic and links without that one; what
// the two share is in csrc/frame_common.hpp, and what this file shares with the aligned NV12 edge (csrc/frame_sim_nv12.hip) --
// the colour maps, affine_row, the surface checks -- in csrc/frame_nv12_common.hpp.  The two kernels are templates over how a
// surface's chroma is addressed (csrc/frame_nv12_axis_common.hpp), which csrc/frame_i420.hip instantiates for three planes: this
// file holds where the bytes of an interleaved UV plane are.
#include "frame_nv12_axis_common.hpp"

namespace {

using namespace spk::frame;

// Where the chroma of an NV12 surface is (csrc/frame_nv12_axis_common.hpp has the kernels): (U, V) pairs, 2-byte aligned.  The way
// in does one 16-bit load of the pair at X & ~1, which serves the two luma columns above it; the paste reads and writes the one
// pair of its block (16 bits).
struct Nv12Surface {
    AxisPlane y, uv;
    struct Row { const uint8_t* c; unsigned pair; };
    __device__ __forceinline__ Row chroma_row(long long n, long long cy) const { return {uv.p + n * uv.image_stride + cy * uv.row_stride, 0u}; }
    __device__ __forceinline__ static void tap(Row& r, int X, bool first, unsigned& u, unsigned& v) {
        if (first || !(X & 1)) r.pair = *reinterpret_cast<const uint16_t*>(r.c + (X & ~1));
        u = r.pair & 0xffu, v = r.pair >> 8;
    }
    __device__ __forceinline__ uint16_t* pair_at(long long n, long long CY, long long CX) const {
        return reinterpret_cast<uint16_t*>(uv.p + n * uv.image_stride + CY * uv.row_stride + CX * 2);
    }
    __device__ __forceinline__ void load_chroma(long long n, long long CY, long long CX, unsigned& u, unsigned& v) const {
        const unsigned pair = *pair_at(n, CY, CX);
        u = pair & 0xffu, v = pair >> 8;
    }
    __device__ __forceinline__ void store_chroma(long long n, long long CY, long long CX, unsigned u, unsigned v) const {
        *pair_at(n, CY, CX) = (uint16_t)(u | v << 8);
    }
};

Nv12Surface surface_of(const uint8_t* y, int64_t y_image_stride, int64_t y_row_stride, const uint8_t* uv, int64_t uv_image_stride,
                       int64_t uv_row_stride, int N) {
    return {axis_plane(y, y_image_stride, y_row_stride, N), axis_plane(uv, uv_image_stride, uv_row_stride, N)};
}

}  // namespace

extern "C" {

int spk_yuv_coeffs(int standard, int full_range, double to_rgb[12], double from_rgb[12]) {
    double kr, kb;
    SPK_REQUIRE(primaries(standard, &kr, &kb), "yuv_coeffs: standard must be 601 or 709 (got %d)", standard);
    SPK_REQUIRE(full_range == 0 || full_range == 1, "yuv_coeffs: full_range must be 0 or 1 (got %d)", full_range);
    SPK_REQUIRE(to_rgb || from_rgb, "yuv_coeffs: null matrix pointers");
    yuv_coeffs(kr, kb, full_range != 0, to_rgb, from_rgb);
    return SPK_OK;
}

int spk_frames_nv12_to_f32(const uint8_t* y, int64_t y_image_stride, int64_t y_row_stride, const uint8_t* uv, int64_t uv_image_stride,
                           int64_t uv_row_stride, int N, int H, int W, const int32_t* boxes_yx, int y0, int x0, int Hin, int Win, int swap_rb,
                           int standard, int full_range, const int32_t* first_y, const int32_t* count_y, const float* w_y, int taps_y,
                           const int32_t* first_x, const int32_t* count_x, const float* w_x, int taps_x, float* dst, int Hout, int Wout,
                           float scale0, float scale1, float scale2, float shift0, float shift1, float shift2, void* stream) {
    const char* who = "frames_nv12_to_f32";
    const ResizeTables t = {first_y, count_y, w_y, first_x, count_x, w_x, taps_y, taps_x};
    if (int rc = check_surface(who, y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N, H, W, false)) return rc;
    if (int rc = check_axis_in(who, dst, t, H, W, Hin, Win, Hout, Wout)) return rc;
    Mat34 M;
    if (int rc = spk_yuv_coeffs(standard, full_range, M.m, nullptr)) return rc;
    return launch_axis_in("frames_nv12_to_f32_kernel", surface_of(y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N), N, H, W,
                          boxes_yx, y0, x0, Hin, Win, swap_rb, t, dst, Hout, Wout, Affine3{{scale0, scale1, scale2}, {shift0, shift1, shift2}}, M,
                          stream);
}

int spk_frames_paste_nv12(const float* src, int N, int Hs, int Ws, uint8_t* y, int64_t y_image_stride, int64_t y_row_stride, uint8_t* uv,
                          int64_t uv_image_stride, int64_t uv_row_stride, int H, int W, int h, int w, int y0, int x0, const int32_t* boxes_yx,
                          int standard, int full_range, const int32_t* first_y, const int32_t* count_y, const float* w_y, int taps_y,
                          const int32_t* first_x, const int32_t* count_x, const float* w_x, int taps_x, const float* a_y, const float* a_x,
                          float lo, float k, void* stream) {
    const char* who = "frames_paste_nv12";
    const ResizeTables t = {first_y, count_y, w_y, first_x, count_x, w_x, taps_y, taps_x};
    SPK_REQUIRE(src, "%s: null frame pointer", who);
    if (int rc = check_surface(who, y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N, H, W, true)) return rc;
    if (int rc = check_axis_paste(who, t, a_y, a_x, Hs, Ws, h, w, lo, k)) return rc;
    Mat34 M;
    if (int rc = spk_yuv_coeffs(standard, full_range, nullptr, M.m)) return rc;
    return launch_axis_paste("frames_paste_nv12_kernel", src, N, Hs, Ws, surface_of(y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N),
                             H, W, h, w, y0, x0, boxes_yx, t, a_y, a_x, lo, k, M, stream);
}

int spk_frames_f32_to_nv12(const float* src, int N, int H, int W, uint8_t* y, int64_t y_image_stride, int64_t y_row_stride, uint8_t* uv,
                           int64_t uv_image_stride, int64_t uv_row_stride, int standard, int full_range, float lo, float k, void* stream) {
    SPK_REQUIRE(src, "frames_f32_to_nv12: null frame pointer");
    if (int rc = check_surface("frames_f32_to_nv12", y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N, H, W, true)) return rc;
    if (int rc = check_range("frames_f32_to_nv12", lo, k)) return rc;
    Mat34 M;
    if (int rc = spk_yuv_coeffs(standard, full_range, nullptr, M.m)) return rc;
    return launch_axis_whole("frames_paste_nv12_kernel<whole frame>", src, N, H, W,
                             surface_of(y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N), lo, k, M, stream);
}

}  // extern "C"
