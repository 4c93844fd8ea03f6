// The tile core of the double-buffered 3x3 weight-gradient kernels (wgrad3x3_pipe_kernel, wgrad3x3_up_kernel, wgrad3x3_wide_kernel,
// wgrad3x3_s2_kernel): block coordinates, accumulator clear, tile decode, the MFMA fragments, the 32 k-steps of a tile with the next
// tile's staging between the MFMAs, the first tile's serial staging, the persistent loop, the slab epilogue, and for wide and s2
// the roles of the 16-byte gradient pieces and the rule that spreads staging between the MFMAs.  Everything is inlined into the
// kernels; a kernel keeps its staging pieces.
//
// What is NOT here, and why: these kernels are scheduled by hand, and the compiler's schedule of their tile loop follows the order
// in which the source states things.  A shared piece was kept wherever the gfx950 code between a kernel's first and last MFMA stayed
// opcode for opcode what it was.  Observed exceptions, which stay written out in the kernel: in up, wg_frag3x3 (its fragment reads
// stay a local macro), the tile loop and wg_store_slab9, and the gradient roles (wg_grad_roles changes its span); in pipe,
// wg_persistent_tiles.  In wide, the loads and stores of the gradient pieces and the row-piece skeleton it has in common with s2
// changed the span when shared (as a struct, and the row test / row destination as functions), so both kernels state them.
// Kernels copy the block coordinates into locals and pass values, not the WgBlock, on: lambdas and helpers that take the struct
// itself changed the span of the 8 x 8 tile kernels.
#pragma once
#include "wgrad_mfma_f32.hpp"

namespace spkwg {

constexpr int WG_TAPS = 9, WG_STEPS = 32, WG_HS = WG_STEPS / 2;      // 64 pixels, two per k-step; loads before WG_HS, LDS stores from it

// ---- the block: CO_T output channels x CI_T input channels of one group, 4 waves ----
struct WgBlock {
    int tid, lane, wave, half, l32;
    int co0, co_end;        // first output channel; end of its group's channels
    int cx0, ci0, nci;      // first x channel of the group; first input channel (within the group); how many of CI_T exist
};

template <int CO_T, int CI_T>
__device__ __forceinline__ WgBlock wg_block(const WgradArgs& p) {
    WgBlock k;
    k.tid = threadIdx.x;
    k.lane = k.tid & 63;
    k.wave = __builtin_amdgcn_readfirstlane(k.tid >> 6);
    k.half = k.lane >> 5;
    k.l32 = k.lane & 31;
    k.co0 = blockIdx.x * CO_T;
    const int grp = k.co0 / p.Cout;
    k.co_end = (grp + 1) * p.Cout;
    k.cx0 = grp * p.gin;
    k.ci0 = blockIdx.y * CI_T;
    k.nci = min(CI_T, p.Cin - k.ci0);
    return k;
}

__device__ __forceinline__ void wg_zero(f32x16 (&acc)[WG_TAPS]) {
#pragma unroll
    for (int t = 0; t < WG_TAPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
}

// tile index -> image and first output pixel
struct WgTile { int b, y0, x0; };

template <int TW, int TH>
__device__ __forceinline__ WgTile wg_tile_origin(const WgradArgs& p, int tile) {
    const int tx = tile % p.tiles_x;
    const int q = tile / p.tiles_x;
    return {q / p.tiles_y, (q % p.tiles_y) * TH, tx * TW};
}

// ---- fragments of k-step ST (pixels 2 ST, 2 ST + 1 of the tile; S = the conv's stride): one gradient value and the 9 taps ----
template <int ST, int TW, int PW, int S>
__device__ __forceinline__ void wg_frag3x3(const volatile wg_lds_f32* ga, const volatile wg_lds_f32* xb, float& fa, float (&fb)[WG_TAPS]) {
    constexpr int px = (2 * ST) & (TW - 1), py = (2 * ST) / TW;
    fa = ga[2 * ST];
#pragma unroll
    for (int t = 0; t < WG_TAPS; ++t) fb[t] = xb[(S * py + t / 3) * PW + S * px + t % 3];
}

// LDS-typed pointers to this lane's operands in the tile buffer `cbuf` (images of shape SH): pixel 2 st + half of gradient row `row`,
// the same pixel's first tap in input channel `row`
template <class SH>
__device__ __forceinline__ const volatile wg_lds_f32* wg_grad_row(const float* cbuf, int row, int half) {
    return (const volatile wg_lds_f32*)(cbuf + row * SH::GPITCH + half);
}
template <class SH, int S>
__device__ __forceinline__ const volatile wg_lds_f32* wg_input_row(const float* cbuf, int row, int half) {
    return (const volatile wg_lds_f32*)(cbuf + SH::CO_T * SH::GPITCH + row * SH::XPITCH + S * half);
}

// the LDS reads of a k-step come first: the next step's fragments (and EXTRA reads of the kernel's own)
template <int ST, int EXTRA = 0>
__device__ __forceinline__ void wg_sched_frag_reads() {
    if constexpr (ST + 1 < WG_STEPS) __builtin_amdgcn_sched_group_barrier(0x100, WG_TAPS + 1 + EXTRA, 0);
}

// One tile's 32 k-steps out of the LDS buffer `cbuf` (images of shape SH): this lane's gradient row is `grow`, its input channel
// `xrow`.  Fragments are read one step ahead; stage(step) issues the step's share of the next tile's staging, sched(step) orders
// the step (wg_sched_frag_reads, then the MFMAs with the staging between them).
template <class SH, int S, class Stage, class Sched>
__device__ __forceinline__ void wg_run_tile(const volatile wg_lds_f32* ga, const volatile wg_lds_f32* xb, f32x16 (&acc)[WG_TAPS], Stage&& stage, Sched&& sched) {
    float fa[2], fb[2][WG_TAPS];
    wg_frag3x3<0, SH::TW, SH::PW, S>(ga, xb, fa[0], fb[0]);
    wg_static_for<0, WG_STEPS>([&](auto s_) {
        constexpr int st = decltype(s_)::value;
        // Nothing may be scheduled across the load / store boundary: left alone, the scheduler hoists the stores' VALU
        // halves (the zero-select of out-of-image pieces, the folded BatchNorm affine) up to the loads they consume -- and
        // every load is then followed by s_waitcnt vmcnt(0), a full memory latency with the MFMA pipe idle (one wave per SIMD).
        if constexpr (st == WG_HS) __builtin_amdgcn_sched_barrier(0);
        if constexpr (st + 1 < WG_STEPS) wg_frag3x3<st + 1, SH::TW, SH::PW, S>(ga, xb, fa[(st + 1) & 1], fb[(st + 1) & 1]);
        stage(s_);
#pragma unroll
        for (int t = 0; t < WG_TAPS; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[st & 1], fb[st & 1][t], acc[t], 0, 0, 0);
        sched(s_);
    });
}

// The persistent loop over the workgroup's tiles (blockIdx.z, + gridDim.z, ...): aim(next tile), run(buffer in use), barrier, flip.
// ONE loop body: after the last tile the staging still runs, with every piece masked off (it reads the tensors' first
// floats and fills the idle buffer with zeros).  With a second, staging-free copy of the tile for that case the
// accumulators cross the if / else merge in VGPRs: 144 v_accvgpr_write before and 144 v_accvgpr_read after EVERY tile's
// 288 MFMAs (and twice the code).
template <class Aim, class Run>
__device__ __forceinline__ void wg_persistent_tiles(const WgradArgs& p, Aim&& aim, Run&& run) {
    int cur = 0;
    for (int tile = blockIdx.z; tile < p.n_tiles; tile += gridDim.z) {
        aim(tile + (int)gridDim.z);
        run(cur);
        __syncthreads();                      // every wave is done with `cur`, and the other buffer is complete
        cur ^= 1;
    }
}

// first tile: staged the serial way (NL load pieces, NS store pieces) into buffer 0
template <int NL, int NS, class Aim, class Load, class Store>
__device__ __forceinline__ void wg_stage_first(const WgradArgs& p, float* buf, Aim&& aim, Load&& load_piece, Store&& store_piece) {
    const int tile = blockIdx.z;
    if (tile < p.n_tiles) {
        aim(tile);
        wg_static_for<0, NL>([&](auto j_) { load_piece(j_); });
        wg_static_for<0, NS>([&](auto s_) { store_piece(buf, s_); });
    }
    __syncthreads();
}

// ---- partial block -> slab [slab][co][tap][ci] (ci contiguous: 128-B stores per half wave); co_base: the wave's first row ----
__device__ __forceinline__ void wg_store_slab9(const WgradArgs& p, const f32x16 (&acc)[WG_TAPS], int co_base, int co_end, int ci, int half) {
    float* out = p.slabs + (size_t)blockIdx.z * p.Cy * WG_TAPS * p.Cin;
#pragma unroll
    for (int t = 0; t < WG_TAPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co_base + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (co < co_end && ci < p.Cin) out[((size_t)co * WG_TAPS + t) * p.Cin + ci] = acc[t][r];
        }
}

// ---- the gradient tile in 16-byte pieces (wide, s2), the roles: piece i = float4 gk of tile row grow of channel (tid >> 4) + 16 i ----
// g_ch[i]: its channel (rows past the group's last channel: clamped, never written out), g_off[i]: its offset from the tile's first
// pixel in channel 0 of the image, g_dst: its LDS offset (+ 16 i GPITCH + j)
template <class SH>
__device__ __forceinline__ void wg_grad_roles(const WgradArgs& p, int tid, int co0, int co_end, int& gk, int& grow, int (&g_ch)[SH::NG4], int (&g_off)[SH::NG4], int& g_dst) {
    gk = tid & (SH::TW / 4 - 1);
    grow = (tid / (SH::TW / 4)) & (SH::TH - 1);
#pragma unroll
    for (int i = 0; i < SH::NG4; ++i) {
        g_ch[i] = min(co0 + (tid >> 4) + 16 * i, co_end - 1);
        g_off[i] = (g_ch[i] * p.H + grow) * p.W + 4 * gk;
    }
    g_dst = (tid >> 4) * SH::GPITCH + grow * SH::TW + 4 * gk;
}

// pieces of a step that issues at most `per` of `n`, `done` being issued already
constexpr int wg_share(int n, int per, int done) { return done + per <= n ? per : (done < n ? n - done : 0); }

// One tile out of buffer `cur` (wide, s2) while the next is staged into the other: SH::PL load pieces behind each of the k-steps
// before WG_HS, SH::PS store pieces behind each of the others, one access behind every TAPS / (np + 1) MFMAs (pieces beyond the
// MFMA count share the last slot).
template <class SH, int S, class Load, class Store>
__device__ __forceinline__ void wg_run_tile_spread(float* smem, int cur, int grow, int xrow, int half, f32x16 (&acc)[WG_TAPS], Load&& load_piece, Store&& store_piece) {
    static_assert(SH::STEPS == WG_STEPS && SH::HS == WG_HS, "the staging shares are stated for 32 k-steps");
    const float* cbuf = smem + cur * SH::BUF;
    float* nbuf = smem + (cur ^ 1) * SH::BUF;
    wg_run_tile<SH, S>(wg_grad_row<SH>(cbuf, grow, half), wg_input_row<SH, S>(cbuf, xrow, half), acc,
        [&](auto s_) {
            constexpr int st = decltype(s_)::value;
            if constexpr (st < WG_HS) {
                wg_static_for<SH::PL * st, SH::PL * st + wg_share(SH::NL, SH::PL, SH::PL * st)>([&](auto j_) { load_piece(j_); });
            } else {
                constexpr int s0 = SH::PS * (st - WG_HS);
                wg_static_for<s0, s0 + wg_share(SH::NS, SH::PS, s0)>([&](auto q_) { store_piece(nbuf, q_); });
            }
        },
        [&](auto s_) {
            constexpr int st = decltype(s_)::value;
            constexpr bool loads = st < WG_HS;
            constexpr int np = loads ? wg_share(SH::NL, SH::PL, SH::PL * st) : wg_share(SH::NS, SH::PS, SH::PS * (st - WG_HS));
            constexpr int per = WG_TAPS / (np + 1) > 0 ? WG_TAPS / (np + 1) : 1;
            constexpr int groups = np < WG_TAPS ? np : WG_TAPS - 1;
            wg_sched_frag_reads<st>();
            wg_static_for<0, groups>([&](auto k_) {
                constexpr int cnt = (decltype(k_)::value + 1 == groups) ? np - (groups - 1) : 1;
                __builtin_amdgcn_sched_group_barrier(0x8, per, 0);
                __builtin_amdgcn_sched_group_barrier(loads ? 0x20 : 0x200, cnt, 0);
            });
            __builtin_amdgcn_sched_group_barrier(0x8, WG_TAPS - per * groups, 0);
        });
}

}  // namespace spkwg
