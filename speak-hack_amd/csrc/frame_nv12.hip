// The video-frame edge in NV12 form: what a hardware decoder / encoder holds in device memory -- a full-resolution Y plane and a
// half-resolution interleaved UV plane, each with its own row pitch -- in and out of the network without a packed-RGB detour.
//   frames_nv12_to_f32: crop (origin by value or per frame from a device array) + antialiased bilinear resize of the three
//   component fields + YUV -> RGB + normalise -> CHW, one pass, no scratch;
//   frames_paste_nv12: resize to the box + quantise + RGB -> YUV + feather-blend into the surface the box came from, one pass,
//   one thread per chroma block (2 x 2 luma pixels); frames_f32_to_nv12 is its whole-frame case without tables.
// Definitions (siting, colour matrices, the order of every operation) are in include/spk.h.  The resize tables are those of
// csrc/frame_io.hip (spk_resize_table, spk_feather_table): this file holds no filter arithmetic and links without that one; what
// the two share is in csrc/frame_common.hpp, and what this file shares with the aligned NV12 edge (csrc/frame_sim_nv12.hip) --
// the colour maps, affine_row, the surface checks -- in csrc/frame_nv12_common.hpp.
#include "frame_nv12_common.hpp"

namespace {

using namespace spk::frame;

// ---- in ----
// A thread owns output column ox of one STRIP-row strip of one frame, as frames_u8_to_f32_kernel does, and carries the three
// component fields Y, U, V of the box through the separable sum in fp64 (same tables, same order of additions); the colour matrix,
// the clamp and the normalisation follow the resize (both are linear, so they commute up to the clamp: see include/spk.h).  Per
// input row the luma window is byte loads (a box column has no alignment); the chroma window is 16-bit loads of packed (U, V)
// pairs, a pair serving the two luma columns above it, and its horizontal sums are formed once per chroma row: a chroma row
// serves two luma rows.  The origin is clamped so that the Hin x Win box lies inside the H x W frame and every window is clamped
// into the box, so neither a tracker's origin nor a foreign table can send a load out of bounds.
__global__ __launch_bounds__(256) void frames_nv12_to_f32_kernel(const uint8_t* __restrict__ yp, long long y_image_stride, long long y_row_stride,
                                                                 const uint8_t* __restrict__ uvp, long long uv_image_stride,
                                                                 long long uv_row_stride, const int* __restrict__ boxes_yx, int y0, int x0,
                                                                 int H, int W, int Hin, int Win, int swap_rb, ResizeTables t,
                                                                 float* __restrict__ dst, int Hout, int Wout, int strips, long long total,
                                                                 Affine3 af, Mat34 to_rgb) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const Strip s = strip_prologue(idx, t, Hin, Win, Hout, Wout, strips);
        double acc[STRIP][3];
#pragma unroll
        for (int k = 0; k < STRIP; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
        const Origin o = box_origin(boxes_yx, s.n, y0, x0);
        const int Y0 = min(max(o.y, 0), H - Hin), X0 = min(max(o.x, 0), W - Win);
        const int Xs = X0 + s.fx;                                // frame column of the window's first tap
        const uint8_t* luma = yp + s.n * y_image_stride + Xs;
        const uint8_t* chroma = uvp + s.n * uv_image_stride;
        const float* wx = t.w_x + (long long)s.ox * t.taps_x;
        double hu = 0.0, hv = 0.0;
        for (int iy = s.row_lo; iy < s.row_hi; ++iy) {
            const int Yf = Y0 + iy;
            if (iy == s.row_lo || !(Yf & 1)) {                   // a new chroma row: its sums serve this luma row and the next
                const uint8_t* c = chroma + (long long)(Yf >> 1) * uv_row_stride;
                unsigned pair = 0;
                hu = hv = 0.0;
                for (int j = 0; j < s.cx; ++j) {
                    const int X = Xs + j;
                    if (j == 0 || !(X & 1)) pair = *reinterpret_cast<const uint16_t*>(c + (X & ~1));
                    const double w = (double)wx[j];
                    hu = fma(w, (double)(pair & 0xffu), hu);
                    hv = fma(w, (double)(pair >> 8), hv);
                }
            }
            const uint8_t* p = luma + (long long)Yf * y_row_stride;
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
// A thread owns one chroma sample of one frame and the 2 x 2 luma pixels under it (x fastest: a wave writes 64 consecutive UV
// pairs and two runs of 128 consecutive Y bytes).  blocks_y x blocks_x = (h / 2 + 1) x (w / 2 + 1) blocks per frame cover a box of
// either parity (with device origins the host cannot know it); block (by, bx) is chroma sample (floor(Y0 / 2) + by,
// floor(X0 / 2) + bx).  H and W are even, so a block lies wholly inside or wholly outside the frame: a block outside is skipped
// before any load, and so is every pixel of a block that the box does not hold.  Per pixel: the fp64 resize of the fp32 source with
// the tables and sums of frames_paste_u8_kernel (RESIZE false: the source pixel itself, which is what identity tables give), the
// fp32 quantise chain without its rounding, RGB -> YUV in fp64, the luma byte blended and stored; the chroma terms are added up
// over the block's pixels in row-major order and blended into the one UV pair the thread reads and writes (16 bits).  A thread
// reads no byte it does not write, so the surfaces may be pasted in place.
template <bool RESIZE>
__global__ __launch_bounds__(256) void frames_paste_nv12_kernel(const float* __restrict__ src, int Hs, int Ws, uint8_t* yp, long long y_image_stride,
                                                                long long y_row_stride, uint8_t* uvp, long long uv_image_stride,
                                                                long long uv_row_stride, int H, int W, int h, int w, int y0, int x0,
                                                                const int* __restrict__ boxes_yx, ResizeTables t,
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
        uint8_t* luma = yp + n * y_image_stride;
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
            uint8_t* py = luma + Yf * y_row_stride + Xf;
            *py = (uint8_t)(int)rint(fmin(fmax(fma(1.0 - m, (double)*py, m * e_y), 0.0), 255.0));
            const double qm = 0.25 * m;
            acc_u = fma(qm, e_u, acc_u);
            acc_v = fma(qm, e_v, acc_v);
            S += qm;
            any = true;
        }
        if (!any) continue;
        uint16_t* pc = reinterpret_cast<uint16_t*>(uvp + n * uv_image_stride + CY * uv_row_stride + CX * 2);
        const unsigned pair = *pc;
        const unsigned u = (unsigned)(int)rint(fmin(fmax(fma(1.0 - S, (double)(pair & 0xffu), acc_u), 0.0), 255.0));
        const unsigned v = (unsigned)(int)rint(fmin(fmax(fma(1.0 - S, (double)(pair >> 8), acc_v), 0.0), 255.0));
        *pc = (uint16_t)(u | v << 8);
    }
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
    SPK_REQUIRE(dst, "%s: null frame pointer", who);
    if (int rc = check_tables(who, t)) return rc;
    SPK_REQUIRE(Hin >= 1 && Win >= 1 && Hout >= 1 && Wout >= 1, "%s: box and output sizes must be >= 1 (%d x %d -> %d x %d)", who, Hin, Win, Hout,
                Wout);
    SPK_REQUIRE(H >= Hin && W >= Win, "%s: the %d x %d box does not fit the %d x %d frame", who, Hin, Win, H, W);
    Mat34 M;
    if (int rc = spk_yuv_coeffs(standard, full_range, M.m, nullptr)) return rc;
    const int strips = spk::ceil_div(Hout, STRIP);
    const long long total = (long long)N * strips * Wout;
    Affine3 af = {{scale0, scale1, scale2}, {shift0, shift1, shift2}};
    hipLaunchKernelGGL(frames_nv12_to_f32_kernel, grid_for(total), dim3(256), 0, (hipStream_t)stream, y, N > 1 ? (long long)y_image_stride : 0ll,
                       (long long)y_row_stride, uv, N > 1 ? (long long)uv_image_stride : 0ll, (long long)uv_row_stride, (const int*)boxes_yx, y0, x0,
                       H, W, Hin, Win, swap_rb, t, dst, Hout, Wout, strips, total, af, M);
    return spk::check_launch("frames_nv12_to_f32_kernel");
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
    if (int rc = check_tables(who, t)) return rc;
    SPK_REQUIRE((a_y == nullptr) == (a_x == nullptr), "%s: the feather tables are both given or both null", who);
    SPK_REQUIRE(Hs >= 1 && Ws >= 1 && h >= 1 && w >= 1, "%s: source and box sizes must be >= 1 (source %d x %d, box %d x %d)", who, Hs, Ws, h, w);
    if (int rc = check_range(who, lo, k)) return rc;
    Mat34 M;
    if (int rc = spk_yuv_coeffs(standard, full_range, nullptr, M.m)) return rc;
    const int blocks_y = h / 2 + 1, blocks_x = w / 2 + 1;
    const long long total = (long long)N * blocks_y * blocks_x;
    hipLaunchKernelGGL(frames_paste_nv12_kernel<true>, grid_for(total), dim3(256), 0, (hipStream_t)stream, src, Hs, Ws, y,
                       N > 1 ? (long long)y_image_stride : 0ll, (long long)y_row_stride, uv, N > 1 ? (long long)uv_image_stride : 0ll,
                       (long long)uv_row_stride, H, W, h, w, y0, x0, (const int*)boxes_yx, t, a_y, a_x, lo, k, blocks_y, blocks_x, total, M);
    return spk::check_launch("frames_paste_nv12_kernel");
}

int spk_frames_f32_to_nv12(const float* src, int N, int H, int W, uint8_t* y, int64_t y_image_stride, int64_t y_row_stride, uint8_t* uv,
                           int64_t uv_image_stride, int64_t uv_row_stride, int standard, int full_range, float lo, float k, void* stream) {
    SPK_REQUIRE(src, "frames_f32_to_nv12: null frame pointer");
    if (int rc = check_surface("frames_f32_to_nv12", y, y_image_stride, y_row_stride, uv, uv_image_stride, uv_row_stride, N, H, W, true)) return rc;
    if (int rc = check_range("frames_f32_to_nv12", lo, k)) return rc;
    Mat34 M;
    if (int rc = spk_yuv_coeffs(standard, full_range, nullptr, M.m)) return rc;
    const int blocks_y = H / 2, blocks_x = W / 2;            // the origin is (0, 0): the blocks of the frame, none empty
    const long long total = (long long)N * blocks_y * blocks_x;
    hipLaunchKernelGGL(frames_paste_nv12_kernel<false>, grid_for(total), dim3(256), 0, (hipStream_t)stream, src, H, W, y,
                       N > 1 ? (long long)y_image_stride : 0ll, (long long)y_row_stride, uv, N > 1 ? (long long)uv_image_stride : 0ll,
                       (long long)uv_row_stride, H, W, H, W, 0, 0, (const int*)nullptr, ResizeTables{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1},
                       (const float*)nullptr, (const float*)nullptr, lo, k, blocks_y, blocks_x, total, M);
    return spk::check_launch("frames_paste_nv12_kernel<whole frame>");
}

}  // extern "C"
