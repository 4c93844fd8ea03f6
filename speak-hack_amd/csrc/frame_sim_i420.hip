// Aligned crops on I420 surfaces (include/spk.h has the definitions): what csrc/frame_sim_nv12.hip does for a hardware decoder's
// surfaces, for what a software decoder / encoder and WebRTC's frame buffer hold -- a Y plane and a U and a V plane at half
// resolution, each with a base address and a pitch of its own, chroma sited by replication -- without interleaving the chroma
// into a scratch NV12 surface and splitting it again.
//   frames_i420_to_f32_sim:       the way in of frames_nv12_to_f32_sim;
//   frames_paste_i420_sim:        its paste, one thread per chroma block (2 x 2 luma pixels, one U byte, one V byte);
//   paste_colour_match_i420_sim:  its statistics as rows;
//   paste_colour_sums_i420_sim:   its statistics as their 13 sums per frame.
// This file holds where the bytes of a surface are read and written and nothing else: the kernels are the templates the NV12 file
// instantiates (csrc/frame_sim_common.hpp, csrc/frame_blend_common.hpp, csrc/frame_sim_nv12_common.hpp), the colour arithmetic is
// YuvTaps' (csrc/frame_nv12_common.hpp), the taps and the surface checks are csrc/frame_i420_common.hpp's.  So an I420 surface
// and the NV12 surface with the same Y bytes and UV[cy][cx] = (U[cy][cx], V[cy][cx]) give the same fp32 bits, the same sums and
// the same bytes.  Chroma is loaded and stored as bytes: no plane needs an alignment or an even pitch.  H and W are even, so
// frame pixel (Y, X) has its chroma sample (Y >> 1, X >> 1) inside both chroma planes and a chroma block lies wholly inside the
// frame: the clamps of the shared geometry keep every load and store of this file in bounds.
#include "frame_i420_common.hpp"
#include "frame_sim_nv12_common.hpp"

namespace {

using namespace spk::frame;

struct Plane {                          // one plane of N surfaces, strides in bytes
    const uint8_t* p;
    long long image_stride, row_stride;
};

// a plane as the kernels walk it: one frame has no image stride (the caller's may be anything)
Plane plane_of(const uint8_t* p, int64_t image_stride, int64_t row_stride, int N) {
    return {p, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride};
}

// How surfaces are read: the arithmetic is I420Taps'; frame n begins n image strides behind each plane.
struct I420Read : I420Taps<I420Read> {
    Plane y, u, v;
    Mat34 to_rgb;
    __device__ __forceinline__ LaunchFrame frame(long long, int H, int W) const { return {H, W}; }
    __device__ __forceinline__ Row row(const LaunchFrame&, long long n, int iy) const {
        return open_row(y.p + n * y.image_stride, y.row_stride, u.p + n * u.image_stride, u.row_stride, v.p + n * v.image_stride, v.row_stride, iy);
    }
    __device__ __forceinline__ void load(const LaunchFrame&, long long n, int X, int Y, double (&b)[3]) const {
        background(y.p + n * y.image_stride, y.row_stride, u.p + n * u.image_stride, u.row_stride, v.p + n * v.image_stride, v.row_stride, X, Y, b);
    }
};

// The paste's target (csrc/frame_sim_nv12_common.hpp has the kernel): the planes of a surface that is written
struct I420Target {
    Plane y, u, v;
    __device__ __forceinline__ LaunchFrame frame(long long, int H, int W) const { return {H, W}; }
    __device__ __forceinline__ static uint8_t* at(const Plane& q, long long n, int X, int Y) {
        return const_cast<uint8_t*>(q.p) + n * q.image_stride + (long long)Y * q.row_stride + X;
    }
    __device__ __forceinline__ uint8_t* luma(const LaunchFrame&, long long n, int X, int Y) const { return at(y, n, X, Y); }
    __device__ __forceinline__ void load_chroma(const LaunchFrame&, long long n, int CX, int CY, unsigned& cu, unsigned& cv) const {
        PlanarPair::load(at(u, n, CX, CY), at(v, n, CX, CY), cu, cv);
    }
    __device__ __forceinline__ void store_chroma(const LaunchFrame&, long long n, int CX, int CY, unsigned cu, unsigned cv) const {
        PlanarPair::store(at(u, n, CX, CY), at(v, n, CX, CY), cu, cv);
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
    I420Read read(int N) const {
        return {{}, plane_of(y, y_image_stride, y_row_stride, N), plane_of(u, u_image_stride, u_row_stride, N), plane_of(v, v_image_stride, v_row_stride, N), {}};
    }
    I420Target target(int N) const {
        return {plane_of(y, y_image_stride, y_row_stride, N), plane_of(u, u_image_stride, u_row_stride, N), plane_of(v, v_image_stride, v_row_stride, N)};
    }
};

// what the paste and its statistics check alike
int check_paste(const char* who, const void* src, const Planes& s, const float* sim_dev, int N, int Hs, int Ws, int H, int W, bool written,
                double feather, float lo, float k, const float* matte_dev, int matte_frames) {
    SPK_REQUIRE(src, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    if (int rc = s.check(who, N, H, W, written)) return rc;
    SPK_REQUIRE(Hs >= 1 && Ws >= 1, "%s: the source size must be >= 1 (got %d x %d)", who, Hs, Ws);
    return check_blend_params(who, N, feather, lo, k, matte_dev, matte_frames);
}

}  // namespace

extern "C" {

int spk_frames_i420_to_f32_sim(const uint8_t* y, int64_t y_image_stride, int64_t y_row_stride, const uint8_t* u, int64_t u_image_stride,
                               int64_t u_row_stride, const uint8_t* v, int64_t v_image_stride, int64_t v_row_stride, int N, int H, int W,
                               const float* sim_dev, int swap_rb, int standard, int full_range, float* dst, int Hout, int Wout, float scale0,
                               float scale1, float scale2, float shift0, float shift1, float shift2, void* stream) {
    const char* who = "frames_i420_to_f32_sim";
    const Planes s = {y, y_image_stride, y_row_stride, u, u_image_stride, u_row_stride, v, v_image_stride, v_row_stride};
    if (int rc = s.check(who, N, H, W, false)) return rc;
    SPK_REQUIRE(dst, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(Hout >= 1 && Wout >= 1, "%s: the output size must be >= 1 (got %d x %d)", who, Hout, Wout);
    I420Read in = s.read(N);
    if (int rc = colour_maps(who, standard, full_range, in.to_rgb.m, nullptr)) return rc;
    return launch_frames_to_f32_sim("frames_i420_to_f32_sim_kernel", in, N, H, W, sim_dev, swap_rb, dst, Hout, Wout,
                                    Affine3{{scale0, scale1, scale2}, {shift0, shift1, shift2}}, stream);
}

int spk_frames_paste_i420_sim(const float* src, int N, int Hs, int Ws, uint8_t* y, int64_t y_image_stride, int64_t y_row_stride, uint8_t* u,
                              int64_t u_image_stride, int64_t u_row_stride, uint8_t* v, int64_t v_image_stride, int64_t v_row_stride, int H, int W,
                              const float* sim_dev, int standard, int full_range, double feather, float lo, float k, const float* matte_dev,
                              int matte_frames, const float* colour_dev, void* stream) {
    const char* who = "frames_paste_i420_sim";
    const Planes s = {y, y_image_stride, y_row_stride, u, u_image_stride, u_row_stride, v, v_image_stride, v_row_stride};
    if (int rc = check_paste(who, src, s, sim_dev, N, Hs, Ws, H, W, true, feather, lo, k, matte_dev, matte_frames)) return rc;
    Mat34 M;
    if (int rc = colour_maps(who, standard, full_range, nullptr, M.m)) return rc;
    return launch_paste_nv12_sim("frames_paste_nv12_sim_kernel<i420>", src, N, Hs, Ws, s.target(N), H, W, sim_dev, feather, lo, k, matte_dev,
                                 matte_frames, colour_dev, M, stream);
}

int spk_paste_colour_match_i420_sim(const float* src, int N, int Hs, int Ws, const uint8_t* y, int64_t y_image_stride, int64_t y_row_stride,
                                    const uint8_t* u, int64_t u_image_stride, int64_t u_row_stride, const uint8_t* v, int64_t v_image_stride,
                                    int64_t v_row_stride, int H, int W, const float* sim_dev, int standard, int full_range, double feather, float lo,
                                    float k, const float* matte_dev, int matte_frames, double max_gain, double min_sigma, double min_weight,
                                    float* colour_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_match_i420_sim";
    const Planes s = {y, y_image_stride, y_row_stride, u, u_image_stride, u_row_stride, v, v_image_stride, v_row_stride};
    if (int rc = check_paste(who, src, s, sim_dev, N, Hs, Ws, H, W, false, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_match(who, N, max_gain, min_sigma, min_weight, colour_out_dev, workspace_dev, workspace_bytes)) return rc;
    I420Read bg = s.read(N);
    if (int rc = colour_maps(who, standard, full_range, bg.to_rgb.m, nullptr)) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<i420>", bg, src, N, Hs, Ws, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames,
                                    workspace_dev, ColourFinish{colour_out_dev, max_gain, min_sigma, min_weight, nullptr}, stream);
}

int spk_paste_colour_sums_i420_sim(const float* src, int N, int Hs, int Ws, const uint8_t* y, int64_t y_image_stride, int64_t y_row_stride,
                                   const uint8_t* u, int64_t u_image_stride, int64_t u_row_stride, const uint8_t* v, int64_t v_image_stride,
                                   int64_t v_row_stride, int H, int W, const float* sim_dev, int standard, int full_range, double feather, float lo,
                                   float k, const float* matte_dev, int matte_frames, double* sums_out_dev, void* workspace_dev,
                                   size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_sums_i420_sim";
    const Planes s = {y, y_image_stride, y_row_stride, u, u_image_stride, u_row_stride, v, v_image_stride, v_row_stride};
    if (int rc = check_paste(who, src, s, sim_dev, N, Hs, Ws, H, W, false, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_sums(who, N, sums_out_dev, workspace_dev, workspace_bytes)) return rc;
    I420Read bg = s.read(N);
    if (int rc = colour_maps(who, standard, full_range, bg.to_rgb.m, nullptr)) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<i420>", bg, src, N, Hs, Ws, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames,
                                    workspace_dev, ColourFinish{nullptr, 0.0, 0.0, 0.0, sums_out_dev}, stream);
}

}  // extern "C"
