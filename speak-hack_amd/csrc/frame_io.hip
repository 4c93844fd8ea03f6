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
#include "spk_common.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

constexpr int STRIP = 8;            // output rows a thread of the resize owns
constexpr int GRID_CAP = 2048;      // workgroups per launch; the rest of the work is a grid-stride trip

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
struct Affine3 { float scale[3], shift[3]; };

// A thread owns output column ox of one STRIP-row strip of one frame, all three channels.  It walks the input rows the strip's
// vertical windows cover once: the horizontal sum of a row from byte loads (one weight load serves the three channels), added
// into the accumulators of the output rows whose window holds the row.  Sums are kept in fp64 (full-rate FMA on this chip, and
// the kernel is bound by its byte loads): with rows that sum to exactly 1 a constant frame comes out as that constant, and the
// longest chain of one output is taps_x + taps_y additions.  No LDS, no scratch; horizontal work is redone only where the
// windows of neighbouring strips overlap.  BOXES: src is the frame origin and the Hin x Win box of frame n starts at
// boxes_yx[n] = (y0, x0), clamped so that the box stays inside the H x W frame (a tracker's box cannot send a load out of bounds).
template <bool BOXES>
__global__ __launch_bounds__(256) void frames_u8_to_f32_kernel(const uint8_t* __restrict__ src, long long image_stride, long long row_stride,
                                                               const int* __restrict__ boxes_yx, int H, int W,
                                                               int Hin, int Win, int swap_rb, const int* __restrict__ first_y,
                                                               const int* __restrict__ count_y, const float* __restrict__ w_y, int taps_y,
                                                               const int* __restrict__ first_x, const int* __restrict__ count_x,
                                                               const float* __restrict__ w_x, int taps_x, float* __restrict__ dst,
                                                               int Hout, int Wout, int strips, long long total, Affine3 af) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(idx % Wout);
        const int strip = (int)((idx / Wout) % strips);
        const long long n = idx / ((long long)Wout * strips);
        const int oy0 = strip * STRIP;
        // the tables are the caller's: clamp every window into the image so that no table can send a load out of bounds
        const int fx = min(max(first_x[ox], 0), Win - 1);
        const int cx = max(min(min(count_x[ox], taps_x), Win - fx), 0);
        int fy[STRIP], cy[STRIP];
        int row_lo = Hin, row_hi = 0;
#pragma unroll
        for (int k = 0; k < STRIP; ++k) {
            const int oy = min(oy0 + k, Hout - 1);
            fy[k] = min(max(first_y[oy], 0), Hin - 1);
            cy[k] = oy0 + k < Hout ? max(min(min(count_y[oy], taps_y), Hin - fy[k]), 0) : 0;
            if (cy[k] > 0) { row_lo = min(row_lo, fy[k]); row_hi = max(row_hi, fy[k] + cy[k]); }
        }
        double acc[STRIP][3];
#pragma unroll
        for (int k = 0; k < STRIP; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
        const uint8_t* img = src + n * image_stride + (long long)fx * 3;
        if (BOXES) {
            const int y0 = min(max(boxes_yx[2 * n], 0), H - Hin), x0 = min(max(boxes_yx[2 * n + 1], 0), W - Win);
            img += (long long)y0 * row_stride + (long long)x0 * 3;
        }
        const float* wx = w_x + (long long)ox * taps_x;
        for (int iy = row_lo; iy < row_hi; ++iy) {
            const uint8_t* p = img + (long long)iy * row_stride;
            double h0 = 0.0, h1 = 0.0, h2 = 0.0;
            for (int j = 0; j < cx; ++j) {
                const double w = (double)wx[j];
                h0 = fma(w, (double)p[3 * j], h0);
                h1 = fma(w, (double)p[3 * j + 1], h1);
                h2 = fma(w, (double)p[3 * j + 2], h2);
            }
#pragma unroll
            for (int k = 0; k < STRIP; ++k) {
                const int j = iy - fy[k];
                if ((unsigned)j < (unsigned)cy[k]) {
                    const double w = (double)w_y[(long long)(oy0 + k) * taps_y + j];
                    acc[k][0] = fma(w, h0, acc[k][0]);
                    acc[k][1] = fma(w, h1, acc[k][1]);
                    acc[k][2] = fma(w, h2, acc[k][2]);
                }
            }
        }
        const long long plane = (long long)Hout * Wout;
        float* out = dst + n * 3 * plane + ox;
#pragma unroll
        for (int k = 0; k < STRIP; ++k) {
            if (oy0 + k >= Hout) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int cd = swap_rb ? 2 - c : c;              // source channel c lands in plane cd
                out[cd * plane + (long long)(oy0 + k) * Wout] = (float)fma((double)af.scale[cd], acc[k][c], (double)af.shift[cd]);
            }
        }
    }
}

// q = rint(min(max((x - lo) * k, 0), 255)) in exactly this order of fp32 operations (a subtraction and a multiplication cannot
// contract into an FMA), the bits of torch's ((x - lo) * k).clamp(0, 255).round().to(torch.uint8), ties to even.  fmaxf returns
// its other operand for a NaN: NaN -> 0.
__device__ __forceinline__ unsigned quant_u8(float x, float lo, float k) {
    const float v = __fmul_rn(__fsub_rn(x, lo), k);
    return (unsigned)rintf(fminf(fmaxf(v, 0.f), 255.f));
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
                                                              const int* __restrict__ boxes_yx, int swap_rb, const int* __restrict__ first_y,
                                                              const int* __restrict__ count_y, const float* __restrict__ w_y, int taps_y,
                                                              const int* __restrict__ first_x, const int* __restrict__ count_x,
                                                              const float* __restrict__ w_x, int taps_x, const float* __restrict__ a_y,
                                                              const float* __restrict__ a_x, float lo, float k, long long total) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % w);
        const int y = (int)((idx / w) % h);
        const long long n = idx / ((long long)w * h);
        const long long Y = (long long)(boxes_yx ? boxes_yx[2 * n] : y0) + y, X = (long long)(boxes_yx ? boxes_yx[2 * n + 1] : x0) + x;
        if (Y < 0 || Y >= H || X < 0 || X >= W) continue;
        // the tables are the caller's: clamp every window into the source so that no table can send a load out of bounds
        const int fx = min(max(first_x[x], 0), Ws - 1), cx = max(min(min(count_x[x], taps_x), Ws - fx), 0);
        const int fy = min(max(first_y[y], 0), Hs - 1), cy = max(min(min(count_y[y], taps_y), Hs - fy), 0);
        const float* wx = w_x + (long long)x * taps_x;
        const float* wy = w_y + (long long)y * taps_y;
        const long long plane = (long long)Hs * Ws;
        const float* in = src + n * 3 * plane + (long long)fy * Ws + fx;
        double v0 = 0.0, v1 = 0.0, v2 = 0.0;
        for (int i = 0; i < cy; ++i) {
            const float* p = in + (long long)i * Ws;
            double h0 = 0.0, h1 = 0.0, h2 = 0.0;
            for (int j = 0; j < cx; ++j) {
                const double wj = (double)wx[j];
                h0 = fma(wj, (double)p[j], h0);
                h1 = fma(wj, (double)p[plane + j], h1);
                h2 = fma(wj, (double)p[2 * plane + j], h2);
            }
            const double wi = (double)wy[i];
            v0 = fma(wi, h0, v0);
            v1 = fma(wi, h1, v1);
            v2 = fma(wi, h2, v2);
        }
        const double m = a_y ? (double)a_y[y] * (double)a_x[x] : 1.0;
        uint8_t* out = dst + n * image_stride + Y * row_stride + X * 3;
        const double v[3] = {v0, v1, v2};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int cd = swap_rb ? 2 - c : c;
            const float q = fminf(fmaxf(__fmul_rn(__fsub_rn((float)v[c], lo), k), 0.f), 255.f);
            const double b = (double)out[cd];
            out[cd] = (uint8_t)(int)rint(fmin(fmax(fma(m, (double)q - b, b), 0.0), 255.0));      // (the clamp: a foreign feather table)
        }
    }
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
    SPK_REQUIRE(src && dst, "frames_u8_to_f32: null frame pointer");
    SPK_REQUIRE(first_y && count_y && w_y && first_x && count_x && w_x, "frames_u8_to_f32: null table pointer");
    SPK_REQUIRE(N >= 1 && Hin >= 1 && Win >= 1 && Hout >= 1 && Wout >= 1, "frames_u8_to_f32: N / H / W must be >= 1 (N %d, %d x %d -> %d x %d)",
                N, Hin, Win, Hout, Wout);
    SPK_REQUIRE(taps_y >= 1 && taps_x >= 1, "frames_u8_to_f32: tap count must be >= 1 (got %d, %d)", taps_y, taps_x);
    SPK_REQUIRE(row_stride >= 3ll * Win, "frames_u8_to_f32: row stride %lld is smaller than 3 * Win = %lld", (long long)row_stride,
                3ll * Win);
    SPK_REQUIRE(image_stride >= 0, "frames_u8_to_f32: negative image stride");
    const int strips = spk::ceil_div(Hout, STRIP);
    const long long total = (long long)N * strips * Wout;
    Affine3 af = {{scale0, scale1, scale2}, {shift0, shift1, shift2}};
    hipLaunchKernelGGL(frames_u8_to_f32_kernel<false>, dim3((unsigned)std::min((total + 255) / 256, (long long)GRID_CAP)), dim3(256), 0,
                       (hipStream_t)stream, src, (long long)image_stride, (long long)row_stride, (const int*)nullptr, Hin, Win, Hin, Win,
                       swap_rb, first_y, count_y, w_y, taps_y, first_x, count_x, w_x, taps_x, dst, Hout, Wout, strips, total, af);
    return spk::check_launch("frames_u8_to_f32_kernel");
}

int spk_frames_u8_to_f32_boxes(const uint8_t* src, int64_t image_stride, int64_t row_stride, int N, int H, int W, const int32_t* boxes_yx,
                               int Hin, int Win, int swap_rb, const int32_t* first_y, const int32_t* count_y, const float* w_y, int taps_y,
                               const int32_t* first_x, const int32_t* count_x, const float* w_x, int taps_x, float* dst, int Hout, int Wout,
                               float scale0, float scale1, float scale2, float shift0, float shift1, float shift2, void* stream) {
    SPK_REQUIRE(src && dst, "frames_u8_to_f32_boxes: null frame pointer");
    SPK_REQUIRE(boxes_yx, "frames_u8_to_f32_boxes: null box origin array");
    SPK_REQUIRE(first_y && count_y && w_y && first_x && count_x && w_x, "frames_u8_to_f32_boxes: null table pointer");
    SPK_REQUIRE(N >= 1 && Hin >= 1 && Win >= 1 && Hout >= 1 && Wout >= 1,
                "frames_u8_to_f32_boxes: N / H / W must be >= 1 (N %d, %d x %d -> %d x %d)", N, Hin, Win, Hout, Wout);
    SPK_REQUIRE(H >= Hin && W >= Win, "frames_u8_to_f32_boxes: the %d x %d box does not fit the %d x %d frame", Hin, Win, H, W);
    SPK_REQUIRE(taps_y >= 1 && taps_x >= 1, "frames_u8_to_f32_boxes: tap count must be >= 1 (got %d, %d)", taps_y, taps_x);
    SPK_REQUIRE(row_stride >= 3ll * W, "frames_u8_to_f32_boxes: row stride %lld is smaller than 3 * W = %lld", (long long)row_stride, 3ll * W);
    SPK_REQUIRE(image_stride >= 0, "frames_u8_to_f32_boxes: negative image stride");
    const int strips = spk::ceil_div(Hout, STRIP);
    const long long total = (long long)N * strips * Wout;
    Affine3 af = {{scale0, scale1, scale2}, {shift0, shift1, shift2}};
    hipLaunchKernelGGL(frames_u8_to_f32_kernel<true>, dim3((unsigned)std::min((total + 255) / 256, (long long)GRID_CAP)), dim3(256), 0,
                       (hipStream_t)stream, src, (long long)image_stride, (long long)row_stride, (const int*)boxes_yx, H, W, Hin, Win, swap_rb,
                       first_y, count_y, w_y, taps_y, first_x, count_x, w_x, taps_x, dst, Hout, Wout, strips, total, af);
    return spk::check_launch("frames_u8_to_f32_kernel<boxes>");
}

int spk_frames_f32_to_u8(const float* src, uint8_t* dst, int N, int H, int W, int swap_rb, float lo, float k, void* stream) {
    SPK_REQUIRE(src && dst, "frames_f32_to_u8: null frame pointer");
    SPK_REQUIRE(N >= 1 && H >= 1 && W >= 1, "frames_f32_to_u8: N / H / W must be >= 1 (N %d, %d x %d)", N, H, W);
    SPK_REQUIRE(std::isfinite(lo) && std::isfinite(k) && k > 0.f, "frames_f32_to_u8: the value range must be finite and increasing");
    const long long HW = (long long)H * W, groups = (HW + 3) / 4, total = (long long)N * groups;
    const bool vec_in = HW % 4 == 0 && (uintptr_t)src % 16 == 0;
    const int mode = !vec_in ? 0 : (uintptr_t)dst % 4 == 0 ? 2 : 1;
    const dim3 grid((unsigned)std::min((total + 255) / 256, (long long)GRID_CAP));
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
    SPK_REQUIRE(src && dst, "frames_paste_u8: null frame pointer");
    SPK_REQUIRE(first_y && count_y && w_y && first_x && count_x && w_x, "frames_paste_u8: null table pointer");
    SPK_REQUIRE((a_y == nullptr) == (a_x == nullptr), "frames_paste_u8: the feather tables are both given or both null");
    SPK_REQUIRE(N >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1,
                "frames_paste_u8: N / H / W must be >= 1 (N %d, source %d x %d, box %d x %d, frame %d x %d)", N, Hs, Ws, h, w, H, W);
    SPK_REQUIRE(taps_y >= 1 && taps_x >= 1, "frames_paste_u8: tap count must be >= 1 (got %d, %d)", taps_y, taps_x);
    SPK_REQUIRE(row_stride >= 3ll * W, "frames_paste_u8: row stride %lld is smaller than 3 * W = %lld", (long long)row_stride, 3ll * W);
    SPK_REQUIRE(N == 1 || image_stride >= (long long)(H - 1) * row_stride + 3ll * W,
                "frames_paste_u8: image stride %lld makes the frames overlap (%d rows of stride %lld)", (long long)image_stride, H,
                (long long)row_stride);
    SPK_REQUIRE(std::isfinite(lo) && std::isfinite(k) && k > 0.f, "frames_paste_u8: the value range must be finite and increasing");
    const long long total = (long long)N * h * w;
    hipLaunchKernelGGL(frames_paste_u8_kernel, dim3((unsigned)std::min((total + 255) / 256, (long long)GRID_CAP)), dim3(256), 0,
                       (hipStream_t)stream, src, Hs, Ws, dst, N > 1 ? (long long)image_stride : 0ll, (long long)row_stride, H, W, h, w, y0, x0,
                       (const int*)boxes_yx, swap_rb, first_y, count_y, w_y, taps_y, first_x, count_x, w_x, taps_x, a_y, a_x, lo, k, total);
    return spk::check_launch("frames_paste_u8_kernel");
}

}  // extern "C"
