// The video-frame edge of the inference path: uint8 HWC frames in, uint8 HWC frames out.
//
// inference.py:29-33,46-58 turns every frame into the network's input with PIL (Resize) + ToTensor + Normalize(0.5, 0.5) on
// the host, and inference.py:78-86 turns the result back into uint8 HWC for the video writer.  On the device that edge is a
// chain of eleven ATen launches per chunk and fp32 traffic over the host link; here it is two kernels:
//   frames_u8_to_f32: crop (pointer + strides) + antialiased bilinear resize + normalise + HWC -> CHW, one pass, no scratch;
//   frames_f32_to_u8: quantise + CHW -> HWC, one pass;
//   frames_paste_u8: the inverse of the crop -- resize to the box + quantise + feather-blend into the uint8 frame the box came
//   from + CHW -> HWC, one pass, the box origin per frame (by value, or from a device array a tracker wrote).
// The resize is separable and table driven: the taps of both axes come from the caller (spk_resize_table, built in fp64 on
// the host), so the kernel holds no filter arithmetic.
#include "frame_common.hpp"

#include <vector>

namespace {

using namespace spk::frame;

// ---- host: the triangle filter of F.interpolate(mode="bilinear", align_corners=False, antialias=True), one output sample ----
// window [first, first + count) and its normalised weights (zero weights at either end dropped); returns count
int table_row(int n_in, int n_out, int o, int* first, std::vector<double>& w) {
    const double s = (double)n_in / (double)n_out;
    const double support = s > 1.0 ? s : 1.0;
    const double centre = s * (o + 0.5);
    int lo = (int)(centre - support + 0.5), hi = (int)(centre + support + 0.5);
    lo = std::max(lo, 0);
    hi = std::min(hi, n_in);
    w.clear();
    double total = 0.0;
    for (int j = lo; j < hi; ++j) {
        const double v = std::max(0.0, 1.0 - std::fabs((j - centre + 0.5) / support));
        w.push_back(v);
        total += v;
    }
    for (double& v : w) v /= total;
    size_t a = 0, b = w.size();
    while (b - a > 1 && w[b - 1] == 0.0) --b;
    while (b - a > 1 && w[a] == 0.0) ++a;
    w.assign(w.begin() + a, w.begin() + b);
    *first = lo + (int)a;
    return (int)w.size();
}

// fp32 weights of one row: each rounded to nearest, then moved by whole ulps -- the largest weights first -- until the row
// sums to exactly 1, so that a constant frame stays that constant whatever the size (a partition of unity in the number
// format the kernel reads).  The residual of the roundings is a multiple of the smallest weight's ulp, so it always fits.
void round_row_f32(const double* w, int count, float* out) {
    double r = 1.0;
    std::vector<int> order(count);
    for (int j = 0; j < count; ++j) {
        out[j] = (float)w[j];
        r -= (double)out[j];
        order[j] = j;
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return out[a] > out[b]; });
    for (int idx = 0; idx < count && r != 0.0; ++idx) {
        float& v = out[order[idx]];
        if (!(v > 0.f)) continue;
        int e;
        std::frexp(v, &e);                                   // v = m * 2^e, m in [0.5, 1): ulp = 2^(e - 24)
        const double ulp = std::ldexp(1.0, e - 24);
        const double k = std::nearbyint(r / ulp);
        if (k == 0.0) continue;
        const float moved = (float)((double)v + k * ulp);
        if (!(moved > 0.f)) continue;
        r -= (double)moved - (double)v;
        v = moved;
    }
}

// ---- device ----
// A thread owns output column ox of one STRIP-row strip of one frame, all three channels.  It walks the input rows the strip's
// vertical windows cover once: the horizontal sum of a row from byte loads (one weight load serves the three channels), added
// into the accumulators of the output rows whose window holds the row.  Sums are kept in fp64 (full-rate FMA on this chip, and
// the kernel is bound by its byte loads): with rows that sum to exactly 1 a constant frame comes out as that constant, and the
// longest chain of one output is taps_x + taps_y additions.  No LDS, no scratch; horizontal work is redone only where the
// windows of neighbouring strips overlap.  BOXES: src is the frame origin and the Hin x Win box of frame n starts at
// boxes_yx[n] = (y0, x0), clamped so that the box stays inside the H x W frame (a tracker's box cannot send a load out of bounds).
template <bool BOXES>
__global__ __launch_bounds__(256) void frames_u8_to_f32_kernel(const uint8_t* __restrict__ src, long long image_stride, long long row_stride,
                                                               const int* __restrict__ boxes_yx, int H, int W, int Hin, int Win, int swap_rb,
                                                               ResizeTables t, float* __restrict__ dst, int Hout, int Wout, int strips,
                                                               long long total, Affine3 af) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const Strip s = strip_prologue(idx, t, Hin, Win, Hout, Wout, strips);
        double acc[STRIP][3];
#pragma unroll
        for (int k = 0; k < STRIP; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
        const uint8_t* img = src + s.n * image_stride + (long long)s.fx * 3;
        if (BOXES) {
            const Origin o = box_origin(boxes_yx, s.n, 0, 0);
            const int y0 = min(max(o.y, 0), H - Hin), x0 = min(max(o.x, 0), W - Win);
            img += (long long)y0 * row_stride + (long long)x0 * 3;
        }
        const float* wx = t.w_x + (long long)s.ox * t.taps_x;
        for (int iy = s.row_lo; iy < s.row_hi; ++iy) {
            const uint8_t* p = img + (long long)iy * row_stride;
            double h0 = 0.0, h1 = 0.0, h2 = 0.0;
            for (int j = 0; j < s.cx; ++j) {
                const double w = (double)wx[j];
                h0 = fma(w, (double)p[3 * j], h0);
                h1 = fma(w, (double)p[3 * j + 1], h1);
                h2 = fma(w, (double)p[3 * j + 2], h2);
            }
            strip_accumulate(acc, s, t, iy, h0, h1, h2);
        }
        const long long plane = (long long)Hout * Wout;
        float* out = dst + s.n * 3 * plane + s.ox;
#pragma unroll
        for (int k = 0; k < STRIP; ++k) {
            if (s.oy0 + k >= Hout) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int cd = swap_rb ? 2 - c : c;              // source channel c lands in plane cd
                out[cd * plane + (long long)(s.oy0 + k) * Wout] = (float)fma((double)af.scale[cd], acc[k][c], (double)af.shift[cd]);
            }
        }
    }
}

// A thread takes four pixels of a frame (pixels counted over the H*W plane).  MODE 2: three float4 loads, three dword stores
// (planes and output 4-byte / 16-byte aligned, H*W % 4 == 0); MODE 1: float4 loads, twelve byte stores (output base not
// 4-byte aligned); MODE 0: dword loads and byte stores with a tail (H*W % 4 != 0 or an unaligned input).
template <int MODE>
__global__ __launch_bounds__(256) void frames_f32_to_u8_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, long long HW,
                                                               long long groups, long long total, int swap_rb, float lo, float k) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long n = idx / groups, p0 = (idx % groups) * 4;
        const float* in = src + n * 3 * HW + p0;
        uint8_t* out = dst + (n * HW + p0) * 3;
        unsigned q[4][3];                                        // [pixel][output channel]
        if (MODE >= 1) {
            float4 v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = *reinterpret_cast<const float4*>(in + c * HW);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int cd = swap_rb ? 2 - c : c;
                q[0][cd] = quant_u8(v[c].x, lo, k); q[1][cd] = quant_u8(v[c].y, lo, k);
                q[2][cd] = quant_u8(v[c].z, lo, k); q[3][cd] = quant_u8(v[c].w, lo, k);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int cd = swap_rb ? 2 - c : c;
#pragma unroll
                for (int i = 0; i < 4; ++i) q[i][cd] = p0 + i < HW ? quant_u8(in[c * HW + i], lo, k) : 0u;
            }
        }
        if (MODE == 2) {
            uint32_t* o4 = reinterpret_cast<uint32_t*>(out);
            o4[0] = q[0][0] | q[0][1] << 8 | q[0][2] << 16 | q[1][0] << 24;
            o4[1] = q[1][1] | q[1][2] << 8 | q[2][0] << 16 | q[2][1] << 24;
            o4[2] = q[2][2] | q[3][0] << 8 | q[3][1] << 16 | q[3][2] << 24;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (MODE == 1 || p0 + i < HW) {
                    out[3 * i] = (uint8_t)q[i][0]; out[3 * i + 1] = (uint8_t)q[i][1]; out[3 * i + 2] = (uint8_t)q[i][2];
                }
        }
    }
}

// The inverse of the crop.  A thread owns one pixel (y, x) of the h x w box of one frame, all three channels (x fastest: a wave
// writes 192 consecutive bytes of a frame row).  It resizes the fp32 source to its pixel with the same tables and the same fp64
// sums as the input kernel (an enlarging box has at most 2 x 2 taps), quantises in the fp32 order of quant_u8 without the
// rounding, reads the background byte it is about to overwrite -- and no other, so the frames may be pasted in place --
// and stores rint(b + m (q - b)) in fp64 (one fused multiply-add), m = a_y[y] a_x[x] the feather (both tables null: m = 1).  The box origin is
// (y0, x0) or, with boxes_yx, frame n's pair of a device array; frame coordinates are formed in 64 bits and every pixel that
// falls outside the H x W frame is skipped, so no origin can send a store (or the load in front of it) out of bounds.  The
// frames are byte addressed at any offset (3 * X0 + row_stride * Y0 has no alignment), so loads and stores are bytes.
__global__ __launch_bounds__(256) void frames_paste_u8_kernel(const float* __restrict__ src, int Hs, int Ws, uint8_t* dst, long long image_stride,
                                                              long long row_stride, int H, int W, int h, int w, int y0, int x0,
                                                              const int* __restrict__ boxes_yx, int swap_rb, ResizeTables t,
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
        uint8_t* out = dst + n * image_stride + Y * row_stride + X * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int cd = swap_rb ? 2 - c : c;
            const float q = quant_unrounded((float)v[c], lo, k);
            const double b = (double)out[cd];
            out[cd] = (uint8_t)(int)rint(fmin(fmax(fma(m, (double)q - b, b), 0.0), 255.0));      // (the clamp: a foreign feather table)
        }
    }
}

// spk_frames_u8_to_f32 and spk_frames_u8_to_f32_boxes: without boxes the box is the frame (H x W = Hin x Win)
int launch_u8_to_f32(const char* who, bool boxes, const uint8_t* src, int64_t image_stride, int64_t row_stride, int N, int H, int W,
                     const int32_t* boxes_yx, int Hin, int Win, int swap_rb, const ResizeTables& t, float* dst, int Hout, int Wout,
                     const Affine3& af, void* stream) {
    SPK_REQUIRE(src && dst, "%s: null frame pointer", who);
    SPK_REQUIRE(!boxes || boxes_yx, "%s: null box origin array", who);
    if (int rc = check_tables(who, t)) return rc;
    SPK_REQUIRE(N >= 1 && Hin >= 1 && Win >= 1 && Hout >= 1 && Wout >= 1, "%s: N / H / W must be >= 1 (N %d, %d x %d -> %d x %d)", who, N, Hin,
                Win, Hout, Wout);
    SPK_REQUIRE(H >= Hin && W >= Win, "%s: the %d x %d box does not fit the %d x %d frame", who, Hin, Win, H, W);
    SPK_REQUIRE(row_stride >= 3ll * W, "%s: row stride %lld is smaller than 3 * W = %lld", who, (long long)row_stride, 3ll * W);
    SPK_REQUIRE(image_stride >= 0, "%s: negative image stride", who);
    const int strips = spk::ceil_div(Hout, STRIP);
    const long long total = (long long)N * strips * Wout;
    hipLaunchKernelGGL(boxes ? frames_u8_to_f32_kernel<true> : frames_u8_to_f32_kernel<false>, grid_for(total), dim3(256), 0, (hipStream_t)stream,
                       src, (long long)image_stride, (long long)row_stride, (const int*)boxes_yx, H, W, Hin, Win, swap_rb, t, dst, Hout, Wout,
                       strips, total, af);
    return spk::check_launch(boxes ? "frames_u8_to_f32_kernel<boxes>" : "frames_u8_to_f32_kernel");
}

}  // namespace

extern "C" {

int spk_resize_table_taps(int n_in, int n_out) {
    SPK_REQUIRE(n_in >= 1 && n_out >= 1, "resize_table_taps: sizes must be >= 1 (got %d -> %d)", n_in, n_out);
    std::vector<double> w;
    int taps = 0, first;
    for (int o = 0; o < n_out; ++o) taps = std::max(taps, table_row(n_in, n_out, o, &first, w));
    return taps;
}

int spk_resize_table(int n_in, int n_out, int taps, int32_t* first_host, int32_t* count_host, double* w_host, float* w_f32_host) {
    SPK_REQUIRE(n_in >= 1 && n_out >= 1, "resize_table: sizes must be >= 1 (got %d -> %d)", n_in, n_out);
    SPK_REQUIRE(first_host && count_host && (w_host || w_f32_host), "resize_table: null table pointer");
    SPK_REQUIRE(taps >= 1, "resize_table: taps must be >= 1 (got %d)", taps);
    std::vector<double> w;
    for (int o = 0; o < n_out; ++o) {
        int first;
        const int count = table_row(n_in, n_out, o, &first, w);
        SPK_REQUIRE(count <= taps, "resize_table: output %d needs %d taps, the table holds %d (spk_resize_table_taps)", o, count, taps);
        first_host[o] = first;
        count_host[o] = count;
        if (w_host) {
            for (int j = 0; j < taps; ++j) w_host[(size_t)o * taps + j] = j < count ? w[j] : 0.0;
        }
        if (w_f32_host) {
            float* row = w_f32_host + (size_t)o * taps;
            for (int j = count; j < taps; ++j) row[j] = 0.f;
            round_row_f32(w.data(), count, row);
        }
    }
    return SPK_OK;
}

int spk_frames_u8_to_f32(const uint8_t* src, int64_t image_stride, int64_t row_stride, int N, int Hin, int Win, int swap_rb,
                         const int32_t* first_y, const int32_t* count_y, const float* w_y, int taps_y, const int32_t* first_x,
                         const int32_t* count_x, const float* w_x, int taps_x, float* dst, int Hout, int Wout, float scale0,
                         float scale1, float scale2, float shift0, float shift1, float shift2, void* stream) {
    return launch_u8_to_f32("frames_u8_to_f32", false, src, image_stride, row_stride, N, Hin, Win, nullptr, Hin, Win, swap_rb,
                            {first_y, count_y, w_y, first_x, count_x, w_x, taps_y, taps_x}, dst, Hout, Wout,
                            {{scale0, scale1, scale2}, {shift0, shift1, shift2}}, stream);
}

int spk_frames_u8_to_f32_boxes(const uint8_t* src, int64_t image_stride, int64_t row_stride, int N, int H, int W, const int32_t* boxes_yx,
                               int Hin, int Win, int swap_rb, const int32_t* first_y, const int32_t* count_y, const float* w_y, int taps_y,
                               const int32_t* first_x, const int32_t* count_x, const float* w_x, int taps_x, float* dst, int Hout, int Wout,
                               float scale0, float scale1, float scale2, float shift0, float shift1, float shift2, void* stream) {
    return launch_u8_to_f32("frames_u8_to_f32_boxes", true, src, image_stride, row_stride, N, H, W, boxes_yx, Hin, Win, swap_rb,
                            {first_y, count_y, w_y, first_x, count_x, w_x, taps_y, taps_x}, dst, Hout, Wout,
                            {{scale0, scale1, scale2}, {shift0, shift1, shift2}}, stream);
}

int spk_frames_f32_to_u8(const float* src, uint8_t* dst, int N, int H, int W, int swap_rb, float lo, float k, void* stream) {
    SPK_REQUIRE(src && dst, "frames_f32_to_u8: null frame pointer");
    SPK_REQUIRE(N >= 1 && H >= 1 && W >= 1, "frames_f32_to_u8: N / H / W must be >= 1 (N %d, %d x %d)", N, H, W);
    if (int rc = check_range("frames_f32_to_u8", lo, k)) return rc;
    const long long HW = (long long)H * W, groups = (HW + 3) / 4, total = (long long)N * groups;
    const bool vec_in = HW % 4 == 0 && (uintptr_t)src % 16 == 0;
    const int mode = !vec_in ? 0 : (uintptr_t)dst % 4 == 0 ? 2 : 1;
    const dim3 grid = grid_for(total);
    if (mode == 2) hipLaunchKernelGGL(frames_f32_to_u8_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, HW, groups, total, swap_rb, lo, k);
    else if (mode == 1) hipLaunchKernelGGL(frames_f32_to_u8_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, HW, groups, total, swap_rb, lo, k);
    else hipLaunchKernelGGL(frames_f32_to_u8_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, HW, groups, total, swap_rb, lo, k);
    return spk::check_launch("frames_f32_to_u8_kernel");
}

int spk_feather_table(int n, double feather, float* a_host) {
    SPK_REQUIRE(n >= 1, "feather_table: n must be >= 1 (got %d)", n);
    SPK_REQUIRE(std::isfinite(feather) && feather >= 0.0, "feather_table: feather must be a finite number >= 0 (got %g)", feather);
    SPK_REQUIRE(a_host, "feather_table: null table pointer");
    for (int i = 0; i < n; ++i) a_host[i] = (float)std::min(1.0, (double)(std::min(i, n - 1 - i) + 1) / (feather + 1.0));
    return SPK_OK;
}

int spk_frames_paste_u8(const float* src, int N, int Hs, int Ws, uint8_t* dst, int64_t image_stride, int64_t row_stride, int H, int W,
                        int h, int w, int y0, int x0, const int32_t* boxes_yx, int swap_rb, const int32_t* first_y, const int32_t* count_y,
                        const float* w_y, int taps_y, const int32_t* first_x, const int32_t* count_x, const float* w_x, int taps_x,
                        const float* a_y, const float* a_x, float lo, float k, void* stream) {
    const char* who = "frames_paste_u8";
    const ResizeTables t = {first_y, count_y, w_y, first_x, count_x, w_x, taps_y, taps_x};
    SPK_REQUIRE(src && dst, "%s: null frame pointer", who);
    if (int rc = check_tables(who, t)) return rc;
    SPK_REQUIRE((a_y == nullptr) == (a_x == nullptr), "%s: the feather tables are both given or both null", who);
    SPK_REQUIRE(N >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1,
                "%s: N / H / W must be >= 1 (N %d, source %d x %d, box %d x %d, frame %d x %d)", who, N, Hs, Ws, h, w, H, W);
    SPK_REQUIRE(row_stride >= 3ll * W, "%s: row stride %lld is smaller than 3 * W = %lld", who, (long long)row_stride, 3ll * W);
    SPK_REQUIRE(N == 1 || image_stride >= (long long)(H - 1) * row_stride + 3ll * W,
                "%s: image stride %lld makes the frames overlap (%d rows of stride %lld)", who, (long long)image_stride, H, (long long)row_stride);
    if (int rc = check_range(who, lo, k)) return rc;
    const long long total = (long long)N * h * w;
    hipLaunchKernelGGL(frames_paste_u8_kernel, grid_for(total), dim3(256), 0, (hipStream_t)stream, src, Hs, Ws, dst,
                       N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, H, W, h, w, y0, x0, (const int*)boxes_yx, swap_rb, t, a_y, a_x,
                       lo, k, total);
    return spk::check_launch("frames_paste_u8_kernel");
}

}  // extern "C"
