// Weight gradient of a 1x1 conv as a GEMM: wgrad1x1_kernel (SPK_WGRAD_GEMM1X1) and its LDS-DMA twin (SPK_WGRAD_GEMM1X1_DMA).
#include "wgrad_mfma_f32.hpp"

using namespace spkwg;

namespace {

// ---- 1x1 weight gradient as a GEMM: dW[co][ci] = sum_{b,pix} g[b,co,pix] * in(x)[b,ci,pix*S] --------------------------------
// The tap-per-tile kernel above keeps ONE accumulator tile per wave for a 1x1 (32 MFMAs per 64-pixel tile against ~80 staged
// elements per thread: staging-bound, a third of the G step's weight-gradient time).  Here a workgroup owns a 128co x 128ci
// block, each of its 2x2 waves a 64x64 quarter (2x2 MFMA tiles sharing their fragments), and walks 32-pixel k-tiles:
// 64 MFMAs per wave against 8 float4 loads per thread, LDS double-buffered (one barrier per k-tile), fragments read one
// k-step ahead.  Pixels are the contraction: rows of G and X are contiguous in memory (16-byte loads, stride 1), and
// LDS rows have pitch 33 so that the 32 lanes of a fragment (32 channels, one pixel) hit 32 banks.

// MT x NT = MFMA tiles per wave along co / ci (1 or 2): the block is (64 MT) co x (64 NT) ci.  2 x 2 is the general form;
// the narrow forms serve the trunk's layer1 shapes (64 -> 256, 256 -> 64, 64 -> 64 at 64^2), where a 128-wide block would
// multiply half a block of zeros.
template <int S, int MODE, int MT, int NT>
__global__ __launch_bounds__(256) void wgrad1x1_kernel(const WgradArgs p, int tiles_per_split) {
    constexpr bool AFF = MODE == WG_AFFINE_RELU;
    constexpr int BM = 64 * MT, BN = 64 * NT;             // block rows of G / of X
    constexpr int RG = BM / 32, RX = BN / 32;             // staging rounds: row = tid/8 + 32 i
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const gs = smem;                               // [2][BM][33]
    float* const xs = smem + 2 * BM * G1_PITCH;           // [2][BN][33]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l32 = lane & 31;
    const int wm = wave & 1, wn = wave >> 1;

    const int co0 = blockIdx.x * BM;                      // in the gradient tensor (all groups)
    const int grp = co0 / p.Cout;
    const int co_end = (grp + 1) * p.Cout;
    const int ci0 = blockIdx.y * BN;                      // within the group
    const int cx0 = grp * p.gin + ci0;                    // first x channel of this block
    const size_t HW = (size_t)p.H * p.W, src_plane = (size_t)p.Hs * p.Ws;
    const int tpi = (int)(HW / G1_KT);                    // k-tiles per image (HW % 32 == 0: checked on the host)
    const int t_begin = blockIdx.z * tiles_per_split, t_end = min(p.n_tiles, t_begin + tiles_per_split);

    // staging roles: row = tid/8 + 32*i, pixels 4*(tid%8) .. +3 of the k-tile
    const int srow = tid >> 3, scol = (tid & 7) * 4;
    float4 gq[RG], xq[RX];
    float a_sc[RX], a_sh[RX];
    bool g_ok[RG], x_ok[RX];
#pragma unroll
    for (int i = 0; i < RG; ++i) g_ok[i] = co0 + srow + 32 * i < co_end;
#pragma unroll
    for (int i = 0; i < RX; ++i) {
        const int r = srow + 32 * i;
        x_ok[i] = ci0 + r < p.Cin;
        a_sc[i] = 1.f; a_sh[i] = 0.f;
        if (AFF && x_ok[i]) { a_sc[i] = p.in_scale[cx0 + r]; a_sh[i] = p.in_shift[cx0 + r]; }
    }

    // Vector-instruction diet (the f32 MFMA shares the SIMD's vector ALU, tools/mfma_valu_coexec.hip: the first version of this
    // loop spent 150 vector instructions per 64 MFMAs -- a uniform integer division, 64-bit address products per load, a zero
    // select per staged value):
    //   * a load is a SCALAR base (image / k-tile: advanced with scalar adds) + the lane's constant 32-bit offset (row, pixels);
    //   * rows past the group / past Cin are loaded from a valid row and NOT zeroed: they only reach accumulator rows / columns
    //     that the final store skips;
    //   * stride 2 gathers keep their per-lane pixel arithmetic (they are three launches of the trunk).
    unsigned g_lane[RG], x_lane[RX];                       // element offsets of (row, scol) from the k-tile's first pixel
#pragma unroll
    for (int i = 0; i < RG; ++i) g_lane[i] = (unsigned)((g_ok[i] ? co0 + srow + 32 * i : co0) * HW) + (unsigned)scol;
#pragma unroll
    for (int i = 0; i < RX; ++i) x_lane[i] = (unsigned)((x_ok[i] ? cx0 + srow + 32 * i : cx0) * src_plane) + (S == 1 ? (unsigned)scol : 0u);
    // (uniform) position of k-tile t: image b, first pixel q of the tile inside the image
    int tb = t_begin / tpi, tq = (t_begin - tb * tpi) * G1_KT;
#define SPK_G1_LOAD(tb_, tq_)                                                                                \
    {                                                                                                        \
        const float* gb_ = p.g + ((size_t)(tb_) * p.Cy * HW + (size_t)(tq_));                  /* uniform */  \
        _Pragma("unroll") for (int i = 0; i < RG; ++i) gq[i] = *reinterpret_cast<const float4*>(gb_ + g_lane[i]); \
        if (S == 1) {                                                                                        \
            const float* xb_ = p.x + ((size_t)(tb_) * p.Cx * src_plane + (size_t)(tq_));       /* uniform */  \
            _Pragma("unroll") for (int i = 0; i < RX; ++i) xq[i] = *reinterpret_cast<const float4*>(xb_ + x_lane[i]); \
        } else {                                                                                             \
            const float* xb_ = p.x + (size_t)(tb_) * p.Cx * src_plane;                                       \
            const int q0_ = (tq_) + scol;                                                                    \
            const int y_ = q0_ / p.W, x_ = q0_ - y_ * p.W;   /* 4 pixels of one row (W % 4 == 0) */           \
            _Pragma("unroll") for (int i = 0; i < RX; ++i) {                                                 \
                const float* xp = xb_ + x_lane[i] + (size_t)(y_ * S) * p.Ws + x_ * S;                        \
                xq[i] = make_float4(xp[0], xp[S], xp[2 * S], xp[3 * S]);                                     \
            }                                                                                                \
        }                                                                                                    \
    }
#define SPK_G1_STORE(buf_)                                                                                   \
    {                                                                                                        \
        float* gd = gs + (buf_) * BM * G1_PITCH;                                                             \
        float* xd = xs + (buf_) * BN * G1_PITCH;                                                             \
        _Pragma("unroll") for (int i = 0; i < RG; ++i) {                                                     \
            const int o = (srow + 32 * i) * G1_PITCH + scol;                                                 \
            gd[o] = gq[i].x; gd[o + 1] = gq[i].y; gd[o + 2] = gq[i].z; gd[o + 3] = gq[i].w;                  \
        }                                                                                                    \
        _Pragma("unroll") for (int i = 0; i < RX; ++i) {                                                     \
            const int o = (srow + 32 * i) * G1_PITCH + scol;                                                 \
            float4 xv = xq[i];                                                                               \
            if (AFF) {                                                                                       \
                xv.x = fmaxf(xv.x * a_sc[i] + a_sh[i], 0.f); xv.y = fmaxf(xv.y * a_sc[i] + a_sh[i], 0.f);    \
                xv.z = fmaxf(xv.z * a_sc[i] + a_sh[i], 0.f); xv.w = fmaxf(xv.w * a_sc[i] + a_sh[i], 0.f);    \
            }                                                                                                \
            xd[o] = xv.x; xd[o + 1] = xv.y; xd[o + 2] = xv.z; xd[o + 3] = xv.w;                              \
        }                                                                                                    \
    }

    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    if (t_begin < t_end) {
        SPK_G1_LOAD(tb, tq);
        SPK_G1_STORE(0);
    }
    __syncthreads();
    for (int t = t_begin; t < t_end; ++t) {
        const int buf = (t - t_begin) & 1;
        const bool more = t + 1 < t_end;
        tq += G1_KT;                                        // (uniform) the next k-tile: same image, or the next one's first
        if (tq >= (int)HW) { tq = 0; ++tb; }
        if (more) SPK_G1_LOAD(tb, tq);
        const volatile wg_lds_f32* ga = (const volatile wg_lds_f32*)(gs + buf * BM * G1_PITCH + (wm * 32 * MT + l32) * G1_PITCH + half);
        const volatile wg_lds_f32* xb = (const volatile wg_lds_f32*)(xs + buf * BN * G1_PITCH + (wn * 32 * NT + l32) * G1_PITCH + half);
        float fa[2][MT], fb[2][NT];
#define SPK_G1_FRAG(ks_, slot_)                                                                              \
    {                                                                                                        \
        _Pragma("unroll") for (int m = 0; m < MT; ++m) fa[slot_][m] = ga[m * 32 * G1_PITCH + 2 * (ks_)];     \
        _Pragma("unroll") for (int n = 0; n < NT; ++n) fb[slot_][n] = xb[n * 32 * G1_PITCH + 2 * (ks_)];     \
    }
        SPK_G1_FRAG(0, 0);
        wg_static_for<0, G1_KT / 2>([&](auto s_) {
            constexpr int ks = decltype(s_)::value;
            if constexpr (ks + 1 < G1_KT / 2) {
                SPK_G1_FRAG(ks + 1, (ks + 1) & 1);
                __builtin_amdgcn_sched_group_barrier(0x100, MT + NT, 0);
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[ks & 1][m], fb[ks & 1][n], acc[m][n], 0, 0, 0);
            __builtin_amdgcn_sched_group_barrier(0x8, MT * NT, 0);
        });
#undef SPK_G1_FRAG
        if (more) SPK_G1_STORE(buf ^ 1);
        __syncthreads();
    }
#undef SPK_G1_LOAD
#undef SPK_G1_STORE

    // partial block -> slab [slab][co][ci] (ci contiguous)
    float* out = p.slabs + (size_t)blockIdx.z * p.Cy * p.Cin;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int ci = ci0 + (wn * NT + n) * 32 + l32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + (wm * MT + m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (co < co_end && ci < p.Cin) out[(size_t)co * p.Cin + ci] = acc[m][n][r];
            }
        }
}

// ---- the same GEMM, stride 1, with EVERY operand by LDS-DMA ---------------------------------------------------------------------
// The register-staged kernel above pays, per 32-pixel k-tile and thread, 8 float4 loads, 32 ds_write_b32 and (folded BatchNorm) 32
// fma / max -- about 45 vector instructions per 64 MFMAs after its diet, and on gfx950 every one of them is matrix time (the f32
// MFMA and the vector ALU do not overlap); its LDS pitch of 33 also rules out wide fragment reads.  Here:
//   * a k-tile row (one channel, 32 pixels = 128 B = eight 16-byte chunks) goes global -> LDS by `global_load_lds_dwordx4`, 8 rows
//     per instruction (scalar base + one constant lane offset), rows at a pitch of exactly 128 B.  Lane i of the instruction fetches
//     chunk (i & 7) ^ f(row) of its row, f(row) = (row >> 1) & 7: the XOR swizzle costs nothing (a lane may fetch any address);
//   * a fragment read is ONE ds_read_b128 per MFMA tile and FOUR k-steps: lane (channel l32, half) takes pixels
//     8 jq + 4 half .. + 3 -- the pixel sum may run in any order as long as G and X use the same one -- and with the swizzle the
//     16 lanes of every ds_read_b128 lane group ({0-3,12-15,20-27} ...) fall on 16 distinct 16-byte slots: conflict-free;
//   * two ring slots, one bare barrier per k-tile, two workgroups per CU (64 KB each): one's DMA wait, barrier and slab
//     store hide behind the other's MFMAs; the loop's only vector instructions are the folded BatchNorm + ReLU of the X
//     fragments (2 per value and NT tiles; none for plain layers).
// Needs whole blocks (Cout % BM == 0, Cin % BN == 0), HW % 32 == 0 and 16-byte aligned tensors: dma_takes().
template <int MODE, int MT, int NT>
__global__ __launch_bounds__(256, 2) void wgrad1x1_dma_kernel(const WgradArgs p, int tiles_per_split) {
    constexpr bool AFF = MODE == WG_AFFINE_RELU;
    constexpr int BM = 64 * MT, BN = 64 * NT, KT = G1_KT;
    constexpr int SLOT_B = (BM + BN) * KT * 4;            // bytes per ring slot: rows [0, BM) of G, then [BM, BM + BN) of X
    constexpr int NJ = (BM + BN) / 32;                    // DMA instructions per wave and k-tile (8 rows each)
    static_assert(KT == 32 && 2 * SLOT_B <= 65536, "immediate LDS offsets reach 64 KB");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l32 = lane & 31;
    const int wm = wave & 1, wn = wave >> 1;

    const int co0 = blockIdx.x * BM;                      // in the gradient tensor (all groups)
    const int grp = co0 / p.Cout;
    const int ci0 = blockIdx.y * BN;                      // within the group
    const int cx0 = grp * p.gin + ci0;                    // first x channel of this block
    const size_t HW = (size_t)p.H * p.W;
    const int tpi = (int)(HW / KT);
    const int t_begin = blockIdx.z * tiles_per_split, t_end = min(p.n_tiles, t_begin + tiles_per_split);

    // DMA role of a lane: row lane / 8 of the instruction's 8 rows; LDS chunk lane % 8 of that row receives global chunk
    // (lane % 8) ^ f(row).  Instruction j = 4 jj + wave covers rows 8 j .. 8 j + 7, so f(row) = (4 (j & 1) + lane / 16) & 7 and
    // j & 1 = wave & 1: ONE constant lane offset per wave.
    // (a BYTE offset added to a byte pointer: base + zext(u32) is the scalar-base form of the load; scaled by 4 it is not)
    unsigned dma_lane = ((unsigned)((lane >> 3) * HW) + (unsigned)((((lane & 7) ^ (4 * (wave & 1) + (lane >> 4))) & 7) * 4)) * 4u;
    const float* const g_w = p.g + (size_t)(co0 + 8 * wave) * HW;
    const float* const x_w = p.x + (size_t)(cx0 + 8 * wave) * HW;
    auto dma_tile = [&](int tb_, int tq_, int slot_) {
        const float* gb = g_w + ((size_t)tb_ * p.Cy * HW + (size_t)tq_);            // uniform
        const float* xb = x_w + ((size_t)tb_ * p.Cx * HW + (size_t)tq_);
        char* dst = reinterpret_cast<char*>(smem) + slot_ * SLOT_B + wave * 1024;
        asm volatile("" : "+v"(dma_lane));                // keep (scalar base, 32-bit lane offset): no per-lane 64-bit pointers
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const float* src = jj * 32 < BM ? gb + (size_t)(jj * 32) * HW : xb + (size_t)(jj * 32 - BM) * HW;
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const char*>(src) + dma_lane, dst + jj * 4096, 16, 0, 0);
        }
    };

    // fragment byte addresses inside a slot, one per 8-pixel group jq (the XOR with the lane's f is not an immediate)
    const unsigned fl = (unsigned)(l32 >> 1) & 7u;
    unsigned a_addr[4], b_addr[4];
#pragma unroll
    for (int jq = 0; jq < 4; ++jq) {
        const unsigned posb = (((unsigned)(2 * jq + half)) ^ fl) * 16u;
        a_addr[jq] = (unsigned)(wm * 32 * MT + l32) * 128u + posb;
        b_addr[jq] = (unsigned)(BM + wn * 32 * NT + l32) * 128u + posb;
        asm volatile("" : "+v"(a_addr[jq]), "+v"(b_addr[jq]));      // eight registers, not a row + chunk add per read
    }
    float sc[NT], sh[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        sc[n] = 1.f; sh[n] = 0.f;
        if (AFF) { sc[n] = p.in_scale[cx0 + (wn * NT + n) * 32 + l32]; sh[n] = p.in_shift[cx0 + (wn * NT + n) * 32 + l32]; }
    }

    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    int tb = t_begin / tpi, tq = (t_begin - tb * tpi) * KT;    // (uniform) image and first pixel of the k-tile being fetched
    if (t_begin < t_end) dma_tile(tb, tq, 0);

    // one k-tile out of ring slot SLOT (compile-time: every LDS offset is an immediate)
    auto run_tile = [&](auto slot_c, bool more) {
        constexpr int SLOT = decltype(slot_c)::value;
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0x0070);               // vmcnt(0) lgkmcnt(0): this wave's rows of the k-tile have landed
        __builtin_amdgcn_s_barrier();                     // ... and everyone's; everyone is done reading the other slot
        __builtin_amdgcn_sched_barrier(0);
        tq += KT;
        if (tq >= (int)HW) { tq = 0; ++tb; }
        if (more) dma_tile(tb, tq, SLOT ^ 1);
        f32x4 fa[2][MT], fb[2][NT];
#define SPK_GD_FRAG(jq_, f_)                                                                                                   \
    {                                                                                                                          \
        _Pragma("unroll") for (int m = 0; m < MT; ++m)                                                                         \
            fa[f_][m] = *(const wg_lds_f32x4*)((wg_lds_u8*)smem + (a_addr[jq_] + (unsigned)(SLOT * SLOT_B + m * 4096)));      \
        _Pragma("unroll") for (int n = 0; n < NT; ++n)                                                                         \
            fb[f_][n] = *(const wg_lds_f32x4*)((wg_lds_u8*)smem + (b_addr[jq_] + (unsigned)(SLOT * SLOT_B + n * 4096)));      \
    }
        SPK_GD_FRAG(0, 0);
        __builtin_amdgcn_sched_barrier(0);
        wg_static_for<0, 4>([&](auto q_) {
            constexpr int jq = decltype(q_)::value;
            if constexpr (jq + 1 < 4) {
                SPK_GD_FRAG(jq + 1, (jq + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);          // the next group's reads first: 16 MFMAs of flight
                __builtin_amdgcn_s_waitcnt(0xC07F | ((MT + NT) << 8));      // lgkmcnt(MT + NT): this group's have landed, no more
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (AFF) {
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int i = 0; i < 4; ++i) fb[jq & 1][n][i] = fmaxf(__builtin_fmaf(fb[jq & 1][n][i], sc[n], sh[n]), 0.f);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int n = 0; n < NT; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[jq & 1][m][i], fb[jq & 1][n][i], acc[m][n], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        });
#undef SPK_GD_FRAG
    };
    for (int t = t_begin; t < t_end; t += 2) {
        run_tile(std::integral_constant<int, 0>{}, t + 1 < t_end);
        if (t + 1 < t_end) run_tile(std::integral_constant<int, 1>{}, t + 2 < t_end);
    }

    // partial block -> slab [slab][co][ci] (ci contiguous)
    float* out = p.slabs + (size_t)blockIdx.z * p.Cy * p.Cin;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int ci = ci0 + (wn * NT + n) * 32 + l32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + (wm * MT + m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                out[(size_t)co * p.Cin + ci] = acc[m][n][r];
            }
        }
}

template <int S, int MODE>
const void* g1_kernel(int MT, int NT) {
    if (MT == 2) return NT == 2 ? reinterpret_cast<const void*>(&wgrad1x1_kernel<S, MODE, 2, 2>) : reinterpret_cast<const void*>(&wgrad1x1_kernel<S, MODE, 2, 1>);
    return NT == 2 ? reinterpret_cast<const void*>(&wgrad1x1_kernel<S, MODE, 1, 2>) : reinterpret_cast<const void*>(&wgrad1x1_kernel<S, MODE, 1, 1>);
}
template <int MODE>
const void* dma_kernel(int MT, int NT) {
    if (MT == 2) return NT == 2 ? reinterpret_cast<const void*>(&wgrad1x1_dma_kernel<MODE, 2, 2>) : reinterpret_cast<const void*>(&wgrad1x1_dma_kernel<MODE, 2, 1>);
    return NT == 2 ? reinterpret_cast<const void*>(&wgrad1x1_dma_kernel<MODE, 1, 2>) : reinterpret_cast<const void*>(&wgrad1x1_dma_kernel<MODE, 1, 1>);
}

}  // namespace

int spkwg::launch_gemm1x1(const WgradPlan& p, hipStream_t stream) {
    const bool aff = p.mode == WG_AFFINE_RELU;
    const void* k = p.form == SPK_WGRAD_GEMM1X1_DMA ? (aff ? dma_kernel<WG_AFFINE_RELU>(p.MT, p.NT) : dma_kernel<WG_PLAIN>(p.MT, p.NT))
                  : p.stride == 1 ? (aff ? g1_kernel<1, WG_AFFINE_RELU>(p.MT, p.NT) : g1_kernel<1, WG_PLAIN>(p.MT, p.NT))
                                  : (aff ? g1_kernel<2, WG_AFFINE_RELU>(p.MT, p.NT) : g1_kernel<2, WG_PLAIN>(p.MT, p.NT));
    return launch_planned(k, "wgrad1x1_kernel", p, stream);
}
