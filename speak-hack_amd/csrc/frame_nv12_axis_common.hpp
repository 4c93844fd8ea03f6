// What the two axis-aligned Y, U, V files share (csrc/frame_nv12.hip: interleaved chroma behind one pointer; csrc/frame_i420.hip:
// a U and a V plane, each with a base and a pitch of its own): the two kernels of the box edge as templates over how a surface's
// chroma is addressed, their launches and the argument checks of their entry points.  The strip decomposition, the fp64 separable
// sums, the colour matrix, the block decode, the resize_point / quant_unrounded chain, the row-major chroma accumulation and the
// blend are written here once, so an I420 surface and the NV12 surface with the same Y bytes and
// UV[cy][cx] = (U[cy][cx], V[cy][cx]) give the same fp32 bits on the way in and the same Y, U and V bytes on the way out.  A file
// holds where the chroma bytes of its surfaces are, and nothing else.
//
// Surface: N frames of H x W pixels.  Its luma plane is an AxisPlane member y (every layout has one); what a layout says is
//   Surface::Row            the chroma of one chroma row on the way in: where it is and the sample held in registers;
//   s.chroma_row(n, cy)     row cy of frame n's chroma;
//   Surface::tap(r, X, first, u, v)   the (U, V) of sample X >> 1 for the tap at frame column X: loaded when the sample changes
//                           (first, or X even) and kept for the tap above the same sample (the rule of Nv12Taps / I420Taps::tap);
//   s.load_chroma(n, CY, CX, u, v) / s.store_chroma(n, CY, CX, u, v)   the one sample a thread of the paste reads and writes.
#pragma once

#include "frame_nv12_common.hpp"

namespace spk::frame {

struct AxisPlane {                      // one plane of N frames, strides in bytes
    uint8_t* p;
    long long image_stride, row_stride;
};

// a plane as the kernels walk it: one frame has no image stride (the caller's may be anything)
inline AxisPlane axis_plane(const uint8_t* p, int64_t image_stride, int64_t row_stride, int N) {
    return {const_cast<uint8_t*>(p), N > 1 ? (long long)image_stride : 0ll, (long long)row_stride};
}

// ---- in ----
// A thread owns output column ox of one STRIP-row strip of one frame, as frames_u8_to_f32_kernel does, and carries the three
// component fields Y, U, V of the box through the separable sum in fp64 (same tables, same order of additions); the colour matrix,
// the clamp and the normalisation follow the resize (both are linear, so they commute up to the clamp: see include/spk.h).  Per
// input row the luma window is byte loads (a box column has no alignment); the chroma window is Surface::tap's loads, a sample
// serving the two luma columns above it, and its horizontal sums are formed once per chroma row: a chroma row serves two luma
// rows.  The origin is clamped so that the Hin x Win box lies inside the H x W frame and every window is clamped into the box, so
// neither a tracker's origin nor a foreign table can send a load out of bounds.
template <class Surface>
__global__ __launch_bounds__(256) void frames_nv12_to_f32_kernel(Surface in, const int* __restrict__ boxes_yx, int y0, int x0, int H, int W, int Hin,
                                                                 int Win, int swap_rb, ResizeTables t, float* __restrict__ dst, int Hout, int Wout,
                                                                 int strips, long long total, Affine3 af, Mat34 to_rgb) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const Strip s = strip_prologue(idx, t, Hin, Win, Hout, Wout, strips);
        double acc[STRIP][3];
#pragma unroll
        for (int k = 0; k < STRIP; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
        const Origin o = box_origin(boxes_yx, s.n, y0, x0);
        const int Y0 = min(max(o.y, 0), H - Hin), X0 = min(max(o.x, 0), W - Win);
        const int Xs = X0 + s.fx;                                // frame column of the window's first tap
        const uint8_t* luma = in.y.p + s.n * in.y.image_stride + Xs;
        const float* wx = t.w_x + (long long)s.ox * t.taps_x;
        double hu = 0.0, hv = 0.0;
        for (int iy = s.row_lo; iy < s.row_hi; ++iy) {
            const int Yf = Y0 + iy;
            if (iy == s.row_lo || !(Yf & 1)) {                   // a new chroma row: its sums serve this luma row and the next
                typename Surface::Row c = in.chroma_row(s.n, Yf >> 1);
                hu = hv = 0.0;
                for (int j = 0; j < s.cx; ++j) {
                    unsigned cu, cv;
                    Surface::tap(c, Xs + j, j == 0, cu, cv);
                    const double w = (double)wx[j];
                    hu = fma(w, (double)cu, hu);
                    hv = fma(w, (double)cv, hv);
                }
            }
            const uint8_t* p = luma + (long long)Yf * in.y.row_stride;
            double hy = 0.0;
            for (int j = 0; j < s.cx; ++j) hy = fma((double)wx[j], (double)p[j], hy);
            strip_accumulate(acc, s, t, iy, hy, hu, hv);
        }
        const long long plane = (long long)Hout * Wout;
        float* out = dst + s.n * 3 * plane + s.ox;
#pragma unroll
        for (int k = 0; k < STRIP; ++k) {
            if (s.oy0 + k >= Hout) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) {                        // c: R, G, B
                const double rgb = fmin(fmax(affine_row(to_rgb, c, acc[k][0], acc[k][1], acc[k][2]), 0.0), 255.0);
                const int cd = swap_rb ? 2 - c : c;
                out[cd * plane + (long long)(s.oy0 + k) * Wout] = (float)fma((double)af.scale[cd], rgb, (double)af.shift[cd]);
            }
        }
    }
}

// ---- out ----
// A thread owns one chroma sample of one frame and the 2 x 2 luma pixels under it (x fastest: a wave writes 64 consecutive chroma
// samples and two runs of 128 consecutive Y bytes).  blocks_y x blocks_x = (h / 2 + 1) x (w / 2 + 1) blocks per frame cover a box of
// either parity (with device origins the host cannot know it); block (by, bx) is chroma sample (floor(Y0 / 2) + by,
// floor(X0 / 2) + bx).  H and W are even, so a block lies wholly inside or wholly outside the frame: a block outside is skipped
// before any load, and so is every pixel of a block that the box does not hold.  Per pixel: the fp64 resize of the fp32 source with
// the tables and sums of frames_paste_u8_kernel (RESIZE false: the source pixel itself, which is what identity tables give), the
// fp32 quantise chain without its rounding, RGB -> YUV in fp64, the luma byte blended and stored; the chroma terms are added up
// over the block's pixels in row-major order and blended into the one sample the thread reads and writes (load_chroma /
// store_chroma: 16 bits of an interleaved plane, a byte of U and a byte of V of a three-plane surface).  A thread reads no byte it
// does not write, so the surfaces may be pasted in place.
template <class Surface, bool RESIZE>
__global__ __launch_bounds__(256) void frames_paste_nv12_kernel(const float* __restrict__ src, int Hs, int Ws, Surface out, int H, int W, int h, int w,
                                                                int y0, int x0, const int* __restrict__ boxes_yx, ResizeTables t,
                                                                const float* __restrict__ a_y, const float* __restrict__ a_x, float lo, float k,
                                                                int blocks_y, int blocks_x, long long total, Mat34 from_rgb) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int bx = (int)(idx % blocks_x);
        const int by = (int)((idx / blocks_x) % blocks_y);
        const long long n = idx / ((long long)blocks_x * blocks_y);
        const Origin o = box_origin(boxes_yx, n, y0, x0);
        const long long Y0 = o.y, X0 = o.x;
        const long long CY = (Y0 - (Y0 & 1)) / 2 + by, CX = (X0 - (X0 & 1)) / 2 + bx;       // floor(origin / 2) + block
        if (CY < 0 || CY >= H / 2 || CX < 0 || CX >= W / 2) continue;
        const long long plane = (long long)Hs * Ws;
        const float* img = src + n * 3 * plane;
        uint8_t* luma = out.y.p + n * out.y.image_stride;
        double acc_u = 0.0, acc_v = 0.0, S = 0.0;
        bool any = false;
#pragma unroll
        for (int d = 0; d < 4; ++d) {                            // row-major over the block
            const long long Yf = 2 * CY + (d >> 1), Xf = 2 * CX + (d & 1);
            const long long yl = Yf - Y0, xl = Xf - X0;
            if (yl < 0 || yl >= h || xl < 0 || xl >= w) continue;
            const int y = (int)yl, x = (int)xl;
            double v0 = 0.0, v1 = 0.0, v2 = 0.0;
            if (RESIZE) {
                resize_point(img, plane, Hs, Ws, t, y, x, v0, v1, v2);
            } else {
                const float* in = img + (long long)y * Ws + x;
                v0 = (double)in[0]; v1 = (double)in[plane]; v2 = (double)in[2 * plane];
            }
            const double q0 = (double)quant_unrounded((float)v0, lo, k);
            const double q1 = (double)quant_unrounded((float)v1, lo, k);
            const double q2 = (double)quant_unrounded((float)v2, lo, k);
            const double e_y = affine_row(from_rgb, 0, q0, q1, q2), e_u = affine_row(from_rgb, 1, q0, q1, q2),
                         e_v = affine_row(from_rgb, 2, q0, q1, q2);
            const double m = a_y ? (double)a_y[y] * (double)a_x[x] : 1.0;
            uint8_t* py = luma + Yf * out.y.row_stride + Xf;
            *py = (uint8_t)(int)rint(fmin(fmax(fma(1.0 - m, (double)*py, m * e_y), 0.0), 255.0));
            const double qm = 0.25 * m;
            acc_u = fma(qm, e_u, acc_u);
            acc_v = fma(qm, e_v, acc_v);
            S += qm;
            any = true;
        }
        if (!any) continue;
        unsigned bu, bv;
        out.load_chroma(n, CY, CX, bu, bv);
        const unsigned u = (unsigned)(int)rint(fmin(fmax(fma(1.0 - S, (double)bu, acc_u), 0.0), 255.0));
        const unsigned v = (unsigned)(int)rint(fmin(fmax(fma(1.0 - S, (double)bv, acc_v), 0.0), 255.0));
        out.store_chroma(n, CY, CX, u, v);
    }
}

// ---- host ----
// what the way in refuses behind its surface check
inline int check_axis_in(const char* who, const void* dst, const ResizeTables& t, int H, int W, int Hin, int Win, int Hout, int Wout) {
    SPK_REQUIRE(dst, "%s: null frame pointer", who);
    if (int rc = check_tables(who, t)) return rc;
    SPK_REQUIRE(Hin >= 1 && Win >= 1 && Hout >= 1 && Wout >= 1, "%s: box and output sizes must be >= 1 (%d x %d -> %d x %d)", who, Hin, Win, Hout,
                Wout);
    SPK_REQUIRE(H >= Hin && W >= Win, "%s: the %d x %d box does not fit the %d x %d frame", who, Hin, Win, H, W);
    return SPK_OK;
}

// what the paste refuses behind its source pointer and its surface check
inline int check_axis_paste(const char* who, const ResizeTables& t, const float* a_y, const float* a_x, int Hs, int Ws, int h, int w, float lo,
                            float k) {
    if (int rc = check_tables(who, t)) return rc;
    SPK_REQUIRE((a_y == nullptr) == (a_x == nullptr), "%s: the feather tables are both given or both null", who);
    SPK_REQUIRE(Hs >= 1 && Ws >= 1 && h >= 1 && w >= 1, "%s: source and box sizes must be >= 1 (source %d x %d, box %d x %d)", who, Hs, Ws, h, w);
    return check_range(who, lo, k);
}

// the three launches over checked arguments
template <class Surface>
int launch_axis_in(const char* kernel, const Surface& in, int N, int H, int W, const int32_t* boxes_yx, int y0, int x0, int Hin, int Win, int swap_rb,
                   const ResizeTables& t, float* dst, int Hout, int Wout, const Affine3& af, const Mat34& to_rgb, void* stream) {
    const int strips = spk::ceil_div(Hout, STRIP);
    const long long total = (long long)N * strips * Wout;
    hipLaunchKernelGGL(frames_nv12_to_f32_kernel<Surface>, grid_for(total), dim3(256), 0, (hipStream_t)stream, in, (const int*)boxes_yx, y0, x0, H, W,
                       Hin, Win, swap_rb, t, dst, Hout, Wout, strips, total, af, to_rgb);
    return spk::check_launch(kernel);
}

template <class Surface>
int launch_axis_paste(const char* kernel, const float* src, int N, int Hs, int Ws, const Surface& out, int H, int W, int h, int w, int y0, int x0,
                      const int32_t* boxes_yx, const ResizeTables& t, const float* a_y, const float* a_x, float lo, float k, const Mat34& from_rgb,
                      void* stream) {
    const int blocks_y = h / 2 + 1, blocks_x = w / 2 + 1;
    const long long total = (long long)N * blocks_y * blocks_x;
    hipLaunchKernelGGL((frames_paste_nv12_kernel<Surface, true>), grid_for(total), dim3(256), 0, (hipStream_t)stream, src, Hs, Ws, out, H, W, h, w, y0,
                       x0, (const int*)boxes_yx, t, a_y, a_x, lo, k, blocks_y, blocks_x, total, from_rgb);
    return spk::check_launch(kernel);
}

template <class Surface>
int launch_axis_whole(const char* kernel, const float* src, int N, int H, int W, const Surface& out, float lo, float k, const Mat34& from_rgb,
                      void* stream) {
    const int blocks_y = H / 2, blocks_x = W / 2;            // the origin is (0, 0): the blocks of the frame, none empty
    const long long total = (long long)N * blocks_y * blocks_x;
    hipLaunchKernelGGL((frames_paste_nv12_kernel<Surface, false>), grid_for(total), dim3(256), 0, (hipStream_t)stream, src, H, W, out, H, W, H, W, 0, 0,
                       (const int*)nullptr, ResizeTables{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1}, (const float*)nullptr,
                       (const float*)nullptr, lo, k, blocks_y, blocks_x, total, from_rgb);
    return spk::check_launch(kernel);
}

}  // namespace spk::frame
