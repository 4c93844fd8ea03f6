// What the aligned NV12 files share (csrc/frame_sim_nv12.hip: N surfaces of one size behind two pointers and four strides;
// csrc/frame_table_nv12.hip: every surface an entry of a device table) with the three-plane files (csrc/frame_sim_i420.hip,
// csrc/frame_table_i420.hip): the way out, a kernel over a format's Target, with its
// launch, and the two colour maps of a standard.  Written once, so that frame n of a table is bit for bit the strided launch at
// N = 1 on entry n: a file holds where the bytes of its surfaces are, and nothing else.
#pragma once

#include "frame_blend_common.hpp"
#include "frame_nv12_common.hpp"

namespace spk::frame {

struct Nv12Pair {                       // the pair of an NV12 target at p: U in the low byte
    __device__ __forceinline__ static void load(const uint8_t* p, unsigned& u, unsigned& v) {
        const unsigned pair = *reinterpret_cast<const uint16_t*>(p);
        u = pair & 0xffu, v = pair >> 8;
    }
    __device__ __forceinline__ static void store(uint8_t* p, unsigned u, unsigned v) { *reinterpret_cast<uint16_t*>(p) = (uint16_t)(u | v << 8); }
};

// The way out.  The decomposition of frames_paste_u8_sim_kernel over CHROMA BLOCKS: blockIdx.y walks the frames, the
// PASTE_WGS workgroups of blockIdx.x share the blocks (x_lo >> 1 ... x_hi >> 1) x (y_lo >> 1 ... y_hi >> 1) of a frame's bounding
// box, x fastest.  A thread owns one chroma sample and the 2 x 2 luma pixels under it, as frames_paste_nv12_kernel does, and
// visits them in row-major order; a pixel takes part when region_pixel holds it.  It reads only bytes it writes -- a luma byte per
// region pixel, the one UV pair of a block that has a region pixel -- so the surfaces may be pasted in place.
// Target: where the surfaces are.  out.frame(n, H, W) is surface n (csrc/frame_sim_common.hpp: its size and usable(), asked once
// per frame); out.luma(frame, n, X, Y) is where luma byte (Y, X) lives; out.load_chroma(frame, n, CX, CY, u, v) reads the (U, V) of
// chroma sample (CY, CX) and out.store_chroma(frame, n, CX, CY, u, v) writes it, as the layout holds it: an NV12 target with one
// 16-bit load and one 16-bit store of the pair (Nv12Pair), a three-plane target (csrc/frame_i420_common.hpp) with a byte
// load and a byte store per plane.  H and W are even, so a chroma block lies wholly inside its surface.
template <class Target>
__global__ __launch_bounds__(256) void frames_paste_nv12_sim_kernel(const float* __restrict__ src, int N, int Hs, int Ws, Target out, int H, int W,
                                                                    const float* __restrict__ sim, double feather, float lo, float k,
                                                                    const float* __restrict__ matte, int matte_frames,
                                                                    const float* __restrict__ colour, Mat34 from_rgb) {
    const long long plane = (long long)Hs * Ws;
    for (long long n = blockIdx.y; n < N; n += gridDim.y) {
        const Sim m = load_sim(sim, n);
        if (!m.valid) continue;
        const auto fr = out.frame(n, H, W);
        if (!fr.usable()) continue;
        const RegionBox box = region_box(m, Hs, Ws, fr.H, fr.W);
        if (box.x_lo > box.x_hi || box.y_lo > box.y_hi) continue;
        const int cx_lo = box.x_lo >> 1, cy_lo = box.y_lo >> 1;
        const long long bw = (box.x_hi >> 1) - cx_lo + 1, total = bw * ((box.y_hi >> 1) - cy_lo + 1);
        const PixelConsts pc = pixel_consts(m, feather);
        const float* img = src + n * 3 * plane;
        const float* mt = matte ? matte + (matte_frames > 1 ? n : 0) * plane : nullptr;
        float g[3], o[3];
        load_colour(colour, n, g, o);
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const int CX = cx_lo + (int)(idx % bw), CY = cy_lo + (int)(idx / bw);
            double acc_u = 0.0, acc_v = 0.0, S = 0.0;
            bool any = false;
#pragma unroll 1
            for (int d = 0; d < 4; ++d) {                        // row-major over the block
                const int Yf = 2 * CY + (d >> 1), Xf = 2 * CX + (d & 1);
                float q[3];
                double mm;
                if (!region_pixel(m, pc, Xf, Yf, img, plane, Hs, Ws, mt, lo, k, q, mm)) continue;
                if (colour) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) q[c] = fminf(fmaxf(fmaf(g[c], q[c], o[c]), 0.f), 255.f);
                }
                const double q0 = (double)q[0], q1 = (double)q[1], q2 = (double)q[2];
                const double e_y = affine_row(from_rgb, 0, q0, q1, q2), e_u = affine_row(from_rgb, 1, q0, q1, q2),
                             e_v = affine_row(from_rgb, 2, q0, q1, q2);
                uint8_t* py = out.luma(fr, n, Xf, Yf);
                *py = (uint8_t)(int)rint(fmin(fmax(fma(1.0 - mm, (double)*py, mm * e_y), 0.0), 255.0));
                const double qm = 0.25 * mm;
                acc_u = fma(qm, e_u, acc_u);
                acc_v = fma(qm, e_v, acc_v);
                S += qm;
                any = true;
            }
            if (!any) continue;
            unsigned bu, bv;
            out.load_chroma(fr, n, CX, CY, bu, bv);
            const unsigned u = (unsigned)(int)rint(fmin(fmax(fma(1.0 - S, (double)bu, acc_u), 0.0), 255.0));
            const unsigned v = (unsigned)(int)rint(fmin(fmax(fma(1.0 - S, (double)bv, acc_v), 0.0), 255.0));
            out.store_chroma(fr, n, CX, CY, u, v);
        }
    }
}

// ---- host ----
// (the two maps of a standard: colour_maps of csrc/frame_nv12_common.hpp)
// the launch of the paste into a target's surfaces over checked arguments (H, W: the launch's size, which a tabled target ignores)
template <class Target>
int launch_paste_nv12_sim(const char* kernel, const float* src, int N, int Hs, int Ws, const Target& out, int H, int W, const float* sim_dev,
                          double feather, float lo, float k, const float* matte_dev, int matte_frames, const float* colour_dev, const Mat34& from_rgb,
                          void* stream) {
    hipLaunchKernelGGL(frames_paste_nv12_sim_kernel<Target>, dim3(PASTE_WGS, (unsigned)std::min(N, 65535)), dim3(256), 0, (hipStream_t)stream, src, N,
                       Hs, Ws, out, H, W, sim_dev, feather, lo, k, matte_dev, matte_frames, colour_dev, from_rgb);
    return spk::check_launch(kernel);
}

}  // namespace spk::frame
