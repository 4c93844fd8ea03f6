// What the RGB32 files share (csrc/frame_sim_rgb32.hip: aligned crops on N frames of one size behind a pointer and two byte strides;
// csrc/frame_table_rgb32.hip: every frame an entry of a device table of spk_frame_ref): how the four bytes of a pixel are read and
// written, and the checks every RGB32 frame argument gets.  An RGB32 frame is the packed frame with the same colour bytes behind a
// pixel stride of 4 and a fourth byte nobody interprets: the kernels are the templates the packed files instantiate, the sums are
// formed from the same byte values in the same order, so the two layouts agree to the bit.  A pixel is ONE aligned 32-bit load --
// and, in the paste, one 32-bit store that carries the fourth byte as it was loaded -- which is why a frame's base and every stride
// that leads to a pixel are multiples of 4: refused on the host, and judged by the kernel for an entry of a table.
#pragma once

#include "frame_blend_common.hpp"

namespace spk::frame {

// A pixel is a little-endian word: memory byte i is bits 8 i ... 8 i + 7.  shift0 = 8 alpha_first is where its first colour byte
// begins: word >> shift0 has the three colour bytes, in memory order, in its low 24 bits.
__device__ __forceinline__ uint32_t load_pixel(const uint8_t* row, int ix) { return reinterpret_cast<const uint32_t*>(row)[ix]; }

// The way in: one 32-bit load per tap; the three sums take the byte values RgbTaps takes, in its order.
struct Rgb32Taps {
    int shift0;
    __device__ __forceinline__ void tap(const uint8_t* p, int ix, bool, double w, double& a0, double& a1, double& a2) const {
        const uint32_t px = load_pixel(p, ix) >> shift0;
        a0 = fma(w, (double)(px & 255u), a0);
        a1 = fma(w, (double)((px >> 8) & 255u), a1);
        a2 = fma(w, (double)((px >> 16) & 255u), a2);
    }
    __device__ __forceinline__ void rgb(double m0, double m1, double m2, double (&val)[3]) const { val[0] = m0, val[1] = m1, val[2] = m2; }
};

// The background of a region pixel by network channel, of the pixel's word loaded once.
__device__ __forceinline__ void rgb32_background(const uint8_t* row, int X, int shift0, int swap_rb, double (&b)[3]) {
    const uint32_t px = load_pixel(row, X) >> shift0;
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = (double)((px >> (8 * (swap_rb ? 2 - c : c))) & 255u);
}

// What a Target of this format answers pixel() with, and the paste's blend_pixel for it: one load of the word that is about to be
// overwritten, the three channels through the arithmetic of the packed blend_pixel, one store with every other bit as loaded.
struct Rgb32Pixel { uint32_t* p; int shift0; };

__device__ __forceinline__ void blend_pixel(Rgb32Pixel out, int swap_rb, bool matched, const float (&g)[3], const float (&o)[3], const float (&q)[3],
                                            double mm) {
    const uint32_t px = *out.p;
    uint32_t res = px;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int sh = out.shift0 + 8 * (swap_rb ? 2 - c : c);
        const float qc = matched ? fminf(fmaxf(fmaf(g[c], q[c], o[c]), 0.f), 255.f) : q[c];
        const double b = (double)((px >> sh) & 255u);
        const uint32_t r = (uint32_t)(int)rint(fma(mm, (double)qc - b, b));     // m in [0, 1], q' and b in [0, 255]: so is the result
        res = (res & ~(255u << sh)) | (r << sh);
    }
    *out.p = res;
}

// ---- host ----
// where the colour is: alpha_first in {0, 1}; -> the shift a policy holds
inline int check_alpha_first(const char* who, int alpha_first) {
    SPK_REQUIRE(alpha_first == 0 || alpha_first == 1, "%s: alpha_first must be 0 (colour in bytes 0..2) or 1 (colour in bytes 1..3), got %d", who,
                alpha_first);
    return SPK_OK;
}

// the checks every strided RGB32 frame argument gets, the counterpart of the packed checks; 0: fine.  written: the frames of a
// paste (they may not overlap); else frames that are only read.
inline int check_rgb32_frames(const char* who, const void* frames, int64_t image_stride, int64_t row_stride, int N, int H, int W, int alpha_first,
                              bool written) {
    SPK_REQUIRE(row_stride >= 4ll * W, "%s: row stride %lld is smaller than 4 * W = %lld", who, (long long)row_stride, 4ll * W);
    SPK_REQUIRE(row_stride % 4 == 0, "%s: row stride %lld is not a multiple of 4 (a pixel is one aligned 32-bit access)", who, (long long)row_stride);
    if (written) {
        SPK_REQUIRE(N == 1 || image_stride >= (long long)(H - 1) * row_stride + 4ll * W,
                    "%s: image stride %lld makes the frames overlap (%d rows of stride %lld)", who, (long long)image_stride, H, (long long)row_stride);
    } else {
        SPK_REQUIRE(image_stride >= 0, "%s: negative image stride", who);
    }
    SPK_REQUIRE(N == 1 || image_stride % 4 == 0, "%s: image stride %lld is not a multiple of 4 (a pixel is one aligned 32-bit access)", who,
                (long long)image_stride);
    SPK_REQUIRE((uintptr_t)frames % 4 == 0, "%s: the frames must be aligned to 4 bytes (got %p)", who, frames);
    return check_alpha_first(who, alpha_first);
}

}  // namespace spk::frame
