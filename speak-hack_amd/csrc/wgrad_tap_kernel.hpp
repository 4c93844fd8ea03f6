// wgrad_kernel<kh, kw, stride, mode, geo>: the weight gradient with one accumulator tile per tap, instantiated by wgrad_inst_tap3x3s1.hip
// (3x3 stride 1) and wgrad_inst_tap.hip (the other shapes).
#pragma once
#include "wgrad_mfma_f32.hpp"

namespace {

using namespace spkwg;

// GEO = 0: the pixel-tile shape (TW x TH x TB) comes from the arguments.  GEO = 1: fixed 16 x 4 x 1 -- the shape of every
// layer whose plane is at least 16 x 4.  With the shape known at compile time the LDS offsets of the 32 k-steps are
// immediates instead of ~100 hoisted address registers, the kernel fits 256 registers and TWO workgroups share a CU
// (one covers the other's staging phase; with runtime geometry the compiler needs 402 registers: one wave per SIMD,
// and the MFMA pipe idles through every store / barrier phase).
template <int KH, int KW, int S, int MODE, int GEO>
__global__ __launch_bounds__(256, GEO ? 2 : 1) void wgrad_kernel(const WgradArgs p) {
    using SH = WShape<KH, KW, S>;
    constexpr int TAPS = SH::TAPS, TP = SH::TP, CI_T = SH::CI_T, CO_T = SH::CO_T, PIX_T = SH::PIX_T, PAD = SH::PAD;
    constexpr bool AFF = MODE == WG_AFFINE_RELU;
    constexpr int KX = SH::KX, NG = CO_T * PIX_T / 256, NPT = SH::NPT, CPT = SH::CPT;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // first channel (within the block) this thread stages: NPT is a multiple of 64, so it is the same for a whole wave --
    // kept in an SGPR, the BatchNorm scale / shift of the staged channels are scalar loads (as per-lane loads they were
    // 2 * CPT vector loads per tile on the serial store phase)
    static_assert(NPT % 64 == 0, "a wave stages one channel slice");
    const int cb = (wave / (NPT / 64)) * CPT;
    const int half = lane >> 5, l32 = lane & 31;
    const int wco = wave & 1, wci = (wave >> 1) % SH::WCI, wpx = (wave >> 1) / SH::WCI;

    const int lgTW = GEO ? 4 : p.lgTW, lgTH = GEO ? 2 : p.lgTH, lgTB = GEO ? 0 : p.lgTB;
    const int TW = 1 << lgTW, TH = 1 << lgTH, TB = 1 << lgTB;
    const int PW = (TW - 1) * S + KW, PH = (TH - 1) * S + KH, PLANE = PH * PW;
    const int GPITCH = PIX_T + 1, XPITCH = (TB * PLANE) | 1;
    float* const g_s = smem;
    float* const x_s = smem + CO_T * GPITCH;

    const int co0 = blockIdx.x * CO_T;                  // in the gradient tensor (all groups)
    const int grp = co0 / p.Cout;
    const int co_end = (grp + 1) * p.Cout;
    const int cx0 = grp * p.gin;                        // the group's first channel in x
    const int ci_blocks = (p.Cin + CI_T - 1) / CI_T;
    const int ci0 = (blockIdx.y % ci_blocks) * CI_T;
    const int pass = blockIdx.y / ci_blocks;            // tap row for ROWPASS kernels, else 0
    const int tap0 = SH::ROWPASS ? pass * KW : 0;
    const int nci = min(CI_T, p.Cin - ci0);
    const size_t HW = (size_t)p.H * p.W, src_plane = (size_t)p.Hs * p.Ws;

    f32x16 acc[TP];
#pragma unroll
    for (int t = 0; t < TP; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // plane positions this thread stages for every channel of every tile (relative to the tile origin)
    int xs_rem[KX], xs_r[KX], xs_c[KX], xs_tb[KX];
#pragma unroll
    for (int k = 0; k < KX; ++k) {
        const int e = (tid % NPT) + NPT * k;
        xs_rem[k] = -1; xs_r[k] = 0; xs_c[k] = 0; xs_tb[k] = 0;
        if (e < TB * PLANE) {
            const int tb = e / PLANE, pidx = e - tb * PLANE;
            xs_rem[k] = e; xs_tb[k] = tb; xs_r[k] = pidx / PW; xs_c[k] = pidx - (pidx / PW) * PW;
        }
    }

    // prefetch registers: the next tile's global loads are in flight during the current tile's MFMAs
    float xg[KX * CPT], gg[NG];
    unsigned xok = 0;   // bit k: plane position k of the prefetched tile is inside the image
    unsigned gok = 0;   // bit i: gradient element i of the prefetched tile is inside the tensor

#define SPK_WG_PREFETCH(tile_)                                                                              \
    {                                                                                                       \
        int bx_ = (tile_);                                                                                  \
        const int tx_ = bx_ % p.tiles_x; bx_ /= p.tiles_x;                                                  \
        const int ty_ = bx_ % p.tiles_y;                                                                    \
        const int b0_ = (bx_ / p.tiles_y) << lgTB, y0_ = ty_ << lgTH, x0_ = tx_ << lgTW;                    \
        gok = 0;                                                                                            \
        _Pragma("unroll") for (int i = 0; i < NG; ++i) {                                                    \
            const int e = tid + 256 * i;                                                                    \
            const int co = e / PIX_T, pix = e % PIX_T;                                                      \
            const int px = pix & (TW - 1), py = (pix >> lgTW) & (TH - 1), tb = pix >> (lgTW + lgTH);        \
            const int b = b0_ + tb, yy = y0_ + py, xx = x0_ + px;                                           \
            const bool ok = tb < TB && b < p.B && yy < p.H && xx < p.W && co0 + co < co_end;                \
            const size_t off = ok ? ((size_t)b * p.Cy + co0 + co) * HW + (size_t)yy * p.W + xx : 0;         \
            gg[i] = p.g[off];          /* masked at store time: no wait on the load here */                \
            if (ok) gok |= 1u << i;                                                                         \
        }                                                                                                   \
        xok = 0;                                                                                            \
        _Pragma("unroll") for (int k = 0; k < KX; ++k) {                                                    \
            const int uy = y0_ * S + xs_r[k] - PAD, ux = x0_ * S + xs_c[k] - PAD, b = b0_ + xs_tb[k];       \
            const bool ok = xs_rem[k] >= 0 && uy >= 0 && uy < p.Hs && ux >= 0 && ux < p.Ws && b < p.B;      \
            if (ok) xok |= 1u << k;                                                                         \
            const float* src = p.x + ((size_t)(ok ? b : 0) * p.Cx + cx0 + ci0) * src_plane +                \
                               (ok ? (size_t)uy * p.Ws + ux : 0);                                           \
            _Pragma("unroll") for (int ci = 0; ci < CPT; ++ci)                                              \
                xg[k * CPT + ci] = src[(size_t)(cb + ci < nci ? cb + ci : 0) * src_plane];                  \
        }                                                                                                   \
    }

#define SPK_WG_STORE()                                                                                      \
    {                                                                                                       \
        _Pragma("unroll") for (int i = 0; i < NG; ++i) {                                                    \
            const int e = tid + 256 * i;                                                                    \
            g_s[(e / PIX_T) * GPITCH + (e % PIX_T)] = ((gok >> i) & 1u) ? gg[i] : 0.f;                      \
        }                                                                                                   \
        _Pragma("unroll") for (int k = 0; k < KX; ++k) {                                                    \
            if (xs_rem[k] >= 0) {                                                                           \
                const bool ok = (xok >> k) & 1u;                                                            \
                float* dst = x_s + xs_rem[k];                                                               \
                _Pragma("unroll") for (int ci = 0; ci < CPT; ++ci) {                                        \
                    float v = xg[k * CPT + ci];                                                             \
                    const int cc = cb + ci;                                                                 \
                    if (AFF) v = fmaxf(v * p.in_scale[cx0 + ci0 + (cc < nci ? cc : 0)] +                    \
                                       p.in_shift[cx0 + ci0 + (cc < nci ? cc : 0)], 0.f);                   \
                    dst[cc * XPITCH] = (ok && cc < nci) ? v : 0.f;                                          \
                }                                                                                           \
            }                                                                                               \
        }                                                                                                   \
    }

    int tile = blockIdx.z;
    if (tile < p.n_tiles) SPK_WG_PREFETCH(tile);
    for (; tile < p.n_tiles; tile += gridDim.z) {
        __syncthreads();          // previous tile fully consumed
        SPK_WG_STORE();
        __syncthreads();
        if (tile + (int)gridDim.z < p.n_tiles) SPK_WG_PREFETCH(tile + (int)gridDim.z);
        // ---- k-steps over this wave's pixel range: A read once per step, reused by every tap ----
        const float* ga = g_s + (wco * 32 + l32) * GPITCH;
        // B-fragment row of this lane: its input channel, or (PACK) its (kx, ci) pair: channel row + kx columns
        const float* xb = SH::PACK ? x_s + (l32 % nci) * XPITCH + min(l32 / nci, KW - 1)
                                   : x_s + (wci * 32 + l32) * XPITCH;
        constexpr int STEPS = PIX_T / 2 / SH::WPX;
        // Fragments are read one k-step ahead of the MFMAs that use them (two register sets, static indices after full
        // unrolling; sched_group_barrier pins the ds_read / MFMA interleave): with 144 accumulator registers the kernel
        // runs one wave per SIMD, so nothing else would hide the LDS latency.
        float fa[2], fb[2][TP];
#define SPK_WG_FRAG(st_, slot_)                                                                             \
    {                                                                                                       \
        const int pix = wpx * (PIX_T / SH::WPX) + 2 * (st_) + half;                                         \
        const int px = pix & (TW - 1), py = (pix >> lgTW) & (TH - 1);                                       \
        const int tb = min(pix >> (lgTW + lgTH), TB - 1);       /* idle pixel groups hold zeros in g_s */   \
        fa[slot_] = ga[pix];                                                                                \
        const float* xp = xb + tb * PLANE + (py * S) * PW + px * S;                                         \
        _Pragma("unroll") for (int t = 0; t < TP; ++t) {                                                    \
            const int tap = tap0 + t;                                                                       \
            const int ky = SH::PACK ? t : tap / KW, kx = SH::PACK ? 0 : tap % KW;   /* PACK: kx sits in the lane */ \
            fb[slot_][t] = xp[ky * PW + kx];                                                                \
        }                                                                                                   \
    }
        SPK_WG_FRAG(0, 0);
        wg_static_for<0, STEPS>([&](auto s_) {
            constexpr int st = decltype(s_)::value;
            if constexpr (st + 1 < STEPS) {
                SPK_WG_FRAG(st + 1, (st + 1) & 1);
                __builtin_amdgcn_sched_group_barrier(0x100, TP + 1, 0);
            }
#pragma unroll
            for (int t = 0; t < TP; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[st & 1], fb[st & 1][t], acc[t], 0, 0, 0);
            __builtin_amdgcn_sched_group_barrier(0x8, TP, 0);
        });
#undef SPK_WG_FRAG
    }
#undef SPK_WG_PREFETCH
#undef SPK_WG_STORE

    // ---- partial block -> slab [slab][co][tap][ci] (ci contiguous: 128-B stores per half wave) ----
    const int slab = blockIdx.z * SH::WPX + wpx;
    float* out = p.slabs + (size_t)slab * p.Cy * TAPS * p.Cin;
    // D column of this lane: an input channel, or (PACK) the (kx, ci) pair l32 = kx * nci + ci
    const int ci = SH::PACK ? l32 % nci : ci0 + wci * 32 + l32;
    const int kx_l = SH::PACK ? l32 / nci : 0;
    const bool col_ok = SH::PACK ? l32 < KW * nci : ci < p.Cin;
#pragma unroll
    for (int t = 0; t < TP; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + wco * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const int tap = SH::PACK ? t * KW + kx_l : tap0 + t;
            if (co < co_end && col_ok) out[((size_t)co * TAPS + tap) * p.Cin + ci] = acc[t][r];
        }
}

template <int KH, int KW, int S>
const void* tap_kernel(const WgradPlan& p) {
    if constexpr (KH == 3 && S == 1) {
        if (p.form == SPK_WGRAD_TAP_FIXED) return reinterpret_cast<const void*>(&wgrad_kernel<3, 3, 1, WG_AFFINE_RELU, 1>);
    }
    if constexpr (KH != 4) {               // (the 4x4 stride-2 form takes a plain input)
        if (p.mode == WG_AFFINE_RELU) return reinterpret_cast<const void*>(&wgrad_kernel<KH, KW, S, WG_AFFINE_RELU, 0>);
    }
    return reinterpret_cast<const void*>(&wgrad_kernel<KH, KW, S, WG_PLAIN, 0>);
}

}  // namespace
