// The axis-aligned video-frame edge on RGB32 frames (include/spk.h has the definitions): what csrc/frame_io.hip does for packed
// 24-bit frames, for what a capture surface, an interop texture or a compositor holds -- uint8 [H][W][4], a pixel one aligned 32-bit
// word in rgba / bgra / argb / abgr order -- without a strip of the fourth byte into packed scratch frames and a scatter back.
//   frames_rgb32_to_f32:  the way in of frames_u8_to_f32 (the box is the frame, or per-frame device origins), a tap ONE 32-bit load;
//   frames_paste_rgb32:   its paste, a pasted pixel one 32-bit load and one 32-bit store that carries the fourth byte as loaded;
//   frames_f32_to_rgb32:  the way out through byte strides, the fourth byte filled with `alpha` or kept.
// csrc/frame_io.hip is left byte for byte as it was: the kernels here are written over the device functions it is written over
// (csrc/frame_common.hpp: strip_prologue, strip_accumulate, resize_point, quant_*, box_origin) and over load_pixel / Rgb32Taps of
// csrc/frame_rgb32_common.hpp, and form the fp64 sums from the same byte values in the same order: every result is bit for bit the
// packed sibling's on a copy of the colour bytes.  The fourth byte is never interpreted.  Links without any other file.
#include "frame_rgb32_common.hpp"

namespace {

using namespace spk::frame;

// ---- in ----
// frames_u8_to_f32_kernel with a pixel stride of 4: a thread owns output column ox of one STRIP-row strip of one frame; per input row
// the horizontal sums of the three colour bytes come from one aligned 32-bit load per tap (Rgb32Taps::tap: the byte values and the
// order of frames_u8_to_f32_kernel's three byte loads).  BOXES: the Hin x Win box of frame n starts at boxes_yx[n], clamped so that
// it stays inside the H x W frame.  The base and both strides are multiples of 4 (refused otherwise), so every tap is aligned.
template <bool BOXES>
__global__ __launch_bounds__(256) void frames_rgb32_to_f32_kernel(const uint8_t* __restrict__ src, long long image_stride, long long row_stride,
                                                                  const int* __restrict__ boxes_yx, int H, int W, int Hin, int Win, int swap_rb,
                                                                  int shift0, ResizeTables t, float* __restrict__ dst, int Hout, int Wout,
                                                                  int strips, long long total, Affine3 af) {
    const Rgb32Taps taps = {shift0};
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const Strip s = strip_prologue(idx, t, Hin, Win, Hout, Wout, strips);
        double acc[STRIP][3];
#pragma unroll
        for (int k = 0; k < STRIP; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
        const uint8_t* img = src + s.n * image_stride + (long long)s.fx * 4;
        if (BOXES) {
            const Origin o = box_origin(boxes_yx, s.n, 0, 0);
            const int y0 = min(max(o.y, 0), H - Hin), x0 = min(max(o.x, 0), W - Win);
            img += (long long)y0 * row_stride + (long long)x0 * 4;
        }
        const float* wx = t.w_x + (long long)s.ox * t.taps_x;
        for (int iy = s.row_lo; iy < s.row_hi; ++iy) {
            const uint8_t* p = img + (long long)iy * row_stride;
            double h0 = 0.0, h1 = 0.0, h2 = 0.0;
            for (int j = 0; j < s.cx; ++j) taps.tap(p, j, false, (double)wx[j], h0, h1, h2);
            strip_accumulate(acc, s, t, iy, h0, h1, h2);
        }
        const long long plane = (long long)Hout * Wout;
        float* out = dst + s.n * 3 * plane + s.ox;
#pragma unroll
        for (int k = 0; k < STRIP; ++k) {
            if (s.oy0 + k >= Hout) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int cd = swap_rb ? 2 - c : c;              // colour byte c lands in plane cd
                out[cd * plane + (long long)(s.oy0 + k) * Wout] = (float)fma((double)af.scale[cd], acc[k][c], (double)af.shift[cd]);
            }
        }
    }
}

// ---- paste ----
// frames_paste_u8_kernel with a pixel stride of 4: a thread owns one pixel (y, x) of the h x w box of one frame (x fastest: a wave
// writes 256 consecutive bytes of a frame row).  The resize, the quantise chain and the blend are that kernel's, on the three colour
// bytes of the word the thread loads once; the word it stores holds the three blended bytes and every other bit as loaded.  It reads
// no pixel but its own, so the frames may be pasted in place; a pixel outside the H x W frame is skipped before its load.
__global__ __launch_bounds__(256) void frames_paste_rgb32_kernel(const float* __restrict__ src, int Hs, int Ws, uint8_t* dst, long long image_stride,
                                                                 long long row_stride, int H, int W, int h, int w, int y0, int x0,
                                                                 const int* __restrict__ boxes_yx, int swap_rb, int shift0, ResizeTables t,
                                                                 const float* __restrict__ a_y, const float* __restrict__ a_x, float lo, float k,
                                                                 long long total) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % w);
        const int y = (int)((idx / w) % h);
        const long long n = idx / ((long long)w * h);
        const Origin o = box_origin(boxes_yx, n, y0, x0);
        const long long Y = (long long)o.y + y, X = (long long)o.x + x;
        if (Y < 0 || Y >= H || X < 0 || X >= W) continue;
        const long long plane = (long long)Hs * Ws;
        double v[3];
        resize_point(src + n * 3 * plane, plane, Hs, Ws, t, y, x, v[0], v[1], v[2]);
        const double m = a_y ? (double)a_y[y] * (double)a_x[x] : 1.0;
        uint32_t* out = reinterpret_cast<uint32_t*>(dst + n * image_stride + Y * row_stride + X * 4);
        const uint32_t px = *out;
        uint32_t res = px;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int sh = shift0 + 8 * (swap_rb ? 2 - c : c);
            const float q = quant_unrounded((float)v[c], lo, k);
            const double b = (double)((px >> sh) & 255u);
            const uint32_t r = (uint32_t)(int)rint(fmin(fmax(fma(m, (double)q - b, b), 0.0), 255.0));        // (the clamp: a foreign feather table)
            res = (res & ~(255u << sh)) | (r << sh);
        }
        *out = res;
    }
}

// ---- out ----
// A thread takes four consecutive pixels of one row of one frame (groups counted per row: a group never straddles a row pitch) and
// writes their four words whole: the three colour bytes quant_u8 gives, in the order of swap_rb behind shift0, and the fourth byte
// -- `alpha`, or with KEEP the fourth byte of the word that is there, loaded by the thread that stores the word (no byte store
// beside another thread's word).  VEC: three float4 loads (W % 4 == 0 and the source planes 16-byte aligned) and the four words as
// four dword accesses, which is all a destination that is only 4-byte aligned -- a region-of-interest view -- allows in C++; on gfx950
// a global_store_dwordx4 needs dword alignment only, and the compiler makes one of them (with KEEP one global_load_dwordx4 in front
// of it), so a 16-byte aligned destination needs no form of its own: written with one uint4 store it compiles to the same
// instructions.  Else: dword loads, dword stores and a row tail (W % 4 != 0 or an unaligned source).
template <bool VEC, bool KEEP>
__global__ __launch_bounds__(256) void frames_f32_to_rgb32_kernel(const float* __restrict__ src, uint8_t* dst, long long image_stride,
                                                                  long long row_stride, int H, int W, int groups, long long total, int swap_rb,
                                                                  int shift0, uint32_t fill, float lo, float k) {
    const uint32_t colour = 0xffffffu << shift0;                 // the bits of a word the three colour bytes take
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x0 = (int)(idx % groups) * 4;
        const int y = (int)((idx / groups) % H);
        const long long n = idx / ((long long)groups * H);
        const long long HW = (long long)H * W;
        const float* in = src + n * 3 * HW + (long long)y * W + x0;
        uint32_t* out = reinterpret_cast<uint32_t*>(dst + n * image_stride + (long long)y * row_stride) + x0;
        uint32_t word[4] = {0u, 0u, 0u, 0u};
        if (VEC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 v = *reinterpret_cast<const float4*>(in + c * HW);
                const int sh = shift0 + 8 * (swap_rb ? 2 - c : c);
                word[0] |= quant_u8(v.x, lo, k) << sh; word[1] |= quant_u8(v.y, lo, k) << sh;
                word[2] |= quant_u8(v.z, lo, k) << sh; word[3] |= quant_u8(v.w, lo, k) << sh;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int sh = shift0 + 8 * (swap_rb ? 2 - c : c);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (x0 + i < W) word[i] |= quant_u8(in[c * HW + i], lo, k) << sh;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (VEC || x0 + i < W) out[i] = word[i] | (KEEP ? out[i] & ~colour : fill);
    }
}

// spk_frames_rgb32_to_f32 and spk_frames_rgb32_to_f32_boxes: without boxes the box is the frame (H x W = Hin x Win)
int launch_rgb32_to_f32(const char* who, bool boxes, const uint8_t* src, int64_t image_stride, int64_t row_stride, int N, int H, int W,
                        const int32_t* boxes_yx, int Hin, int Win, int swap_rb, int alpha_first, const ResizeTables& t, float* dst, int Hout,
                        int Wout, const Affine3& af, void* stream) {
    SPK_REQUIRE(src && dst, "%s: null frame pointer", who);
    SPK_REQUIRE(!boxes || boxes_yx, "%s: null box origin array", who);
    if (int rc = check_tables(who, t)) return rc;
    SPK_REQUIRE(N >= 1 && Hin >= 1 && Win >= 1 && Hout >= 1 && Wout >= 1, "%s: N / H / W must be >= 1 (N %d, %d x %d -> %d x %d)", who, N, Hin,
                Win, Hout, Wout);
    SPK_REQUIRE(H >= Hin && W >= Win, "%s: the %d x %d box does not fit the %d x %d frame", who, Hin, Win, H, W);
    if (int rc = check_rgb32_frames(who, src, image_stride, row_stride, N, H, W, alpha_first, false)) return rc;
    const int strips = spk::ceil_div(Hout, STRIP);
    const long long total = (long long)N * strips * Wout;
    hipLaunchKernelGGL(boxes ? frames_rgb32_to_f32_kernel<true> : frames_rgb32_to_f32_kernel<false>, grid_for(total), dim3(256), 0,
                       (hipStream_t)stream, src, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, (const int*)boxes_yx, H, W, Hin, Win,
                       swap_rb, 8 * alpha_first, t, dst, Hout, Wout, strips, total, af);
    return spk::check_launch(boxes ? "frames_rgb32_to_f32_kernel<boxes>" : "frames_rgb32_to_f32_kernel");
}

template <bool VEC>
void launch_out(bool keep, dim3 grid, hipStream_t stream, const float* src, uint8_t* dst, long long image_stride, long long row_stride, int H, int W,
                int groups, long long total, int swap_rb, int shift0, uint32_t fill, float lo, float k) {
    if (keep)
        hipLaunchKernelGGL((frames_f32_to_rgb32_kernel<VEC, true>), grid, dim3(256), 0, stream, src, dst, image_stride, row_stride, H, W, groups,
                           total, swap_rb, shift0, fill, lo, k);
    else
        hipLaunchKernelGGL((frames_f32_to_rgb32_kernel<VEC, false>), grid, dim3(256), 0, stream, src, dst, image_stride, row_stride, H, W, groups,
                           total, swap_rb, shift0, fill, lo, k);
}

}  // namespace

extern "C" {

int spk_frames_rgb32_to_f32(const uint8_t* src, int64_t image_stride, int64_t row_stride, int N, int Hin, int Win, int swap_rb, int alpha_first,
                            const int32_t* first_y, const int32_t* count_y, const float* w_y, int taps_y, const int32_t* first_x,
                            const int32_t* count_x, const float* w_x, int taps_x, float* dst, int Hout, int Wout, float scale0, float scale1,
                            float scale2, float shift0, float shift1, float shift2, void* stream) {
    return launch_rgb32_to_f32("frames_rgb32_to_f32", false, src, image_stride, row_stride, N, Hin, Win, nullptr, Hin, Win, swap_rb, alpha_first,
                               {first_y, count_y, w_y, first_x, count_x, w_x, taps_y, taps_x}, dst, Hout, Wout,
                               {{scale0, scale1, scale2}, {shift0, shift1, shift2}}, stream);
}

int spk_frames_rgb32_to_f32_boxes(const uint8_t* src, int64_t image_stride, int64_t row_stride, int N, int H, int W, const int32_t* boxes_yx,
                                  int Hin, int Win, int swap_rb, int alpha_first, const int32_t* first_y, const int32_t* count_y, const float* w_y,
                                  int taps_y, const int32_t* first_x, const int32_t* count_x, const float* w_x, int taps_x, float* dst, int Hout,
                                  int Wout, float scale0, float scale1, float scale2, float shift0, float shift1, float shift2, void* stream) {
    return launch_rgb32_to_f32("frames_rgb32_to_f32_boxes", true, src, image_stride, row_stride, N, H, W, boxes_yx, Hin, Win, swap_rb, alpha_first,
                               {first_y, count_y, w_y, first_x, count_x, w_x, taps_y, taps_x}, dst, Hout, Wout,
                               {{scale0, scale1, scale2}, {shift0, shift1, shift2}}, stream);
}

int spk_frames_paste_rgb32(const float* src, int N, int Hs, int Ws, uint8_t* dst, int64_t image_stride, int64_t row_stride, int H, int W, int h,
                           int w, int y0, int x0, const int32_t* boxes_yx, int swap_rb, int alpha_first, const int32_t* first_y,
                           const int32_t* count_y, const float* w_y, int taps_y, const int32_t* first_x, const int32_t* count_x, const float* w_x,
                           int taps_x, const float* a_y, const float* a_x, float lo, float k, void* stream) {
    const char* who = "frames_paste_rgb32";
    const ResizeTables t = {first_y, count_y, w_y, first_x, count_x, w_x, taps_y, taps_x};
    SPK_REQUIRE(src && dst, "%s: null frame pointer", who);
    if (int rc = check_tables(who, t)) return rc;
    SPK_REQUIRE((a_y == nullptr) == (a_x == nullptr), "%s: the feather tables are both given or both null", who);
    SPK_REQUIRE(N >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1,
                "%s: N / H / W must be >= 1 (N %d, source %d x %d, box %d x %d, frame %d x %d)", who, N, Hs, Ws, h, w, H, W);
    if (int rc = check_rgb32_frames(who, dst, image_stride, row_stride, N, H, W, alpha_first, true)) return rc;
    if (int rc = check_range(who, lo, k)) return rc;
    const long long total = (long long)N * h * w;
    hipLaunchKernelGGL(frames_paste_rgb32_kernel, grid_for(total), dim3(256), 0, (hipStream_t)stream, src, Hs, Ws, dst,
                       N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, H, W, h, w, y0, x0, (const int*)boxes_yx, swap_rb,
                       8 * alpha_first, t, a_y, a_x, lo, k, total);
    return spk::check_launch("frames_paste_rgb32_kernel");
}

int spk_frames_f32_to_rgb32(const float* src, uint8_t* dst, int64_t image_stride, int64_t row_stride, int N, int H, int W, int swap_rb,
                            int alpha_first, int alpha, float lo, float k, void* stream) {
    const char* who = "frames_f32_to_rgb32";
    SPK_REQUIRE(src && dst, "%s: null frame pointer", who);
    SPK_REQUIRE(N >= 1 && H >= 1 && W >= 1, "%s: N / H / W must be >= 1 (N %d, %d x %d)", who, N, H, W);
    if (int rc = check_rgb32_frames(who, dst, image_stride, row_stride, N, H, W, alpha_first, true)) return rc;
    SPK_REQUIRE(alpha >= -1 && alpha <= 255, "%s: alpha must be 0 .. 255, or -1 to keep the fourth byte that is there (got %d)", who, alpha);
    if (int rc = check_range(who, lo, k)) return rc;
    const long long img = N > 1 ? (long long)image_stride : 0ll;
    const int groups = (int)(((long long)W + 3) / 4);
    const long long total = (long long)N * H * groups;
    const bool vec = W % 4 == 0 && (uintptr_t)src % 16 == 0;            // (then H W % 4 == 0: every plane and every row of it is 16-byte aligned)
    const int shift0 = 8 * alpha_first;
    const uint32_t fill = alpha < 0 ? 0u : (uint32_t)alpha << (alpha_first ? 0 : 24);
    const dim3 grid = grid_for(total);
    if (vec) launch_out<true>(alpha < 0, grid, (hipStream_t)stream, src, dst, img, row_stride, H, W, groups, total, swap_rb, shift0, fill, lo, k);
    else launch_out<false>(alpha < 0, grid, (hipStream_t)stream, src, dst, img, row_stride, H, W, groups, total, swap_rb, shift0, fill, lo, k);
    return spk::check_launch("frames_f32_to_rgb32_kernel");
}

}  // extern "C"
