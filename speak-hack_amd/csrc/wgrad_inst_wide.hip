// Weight gradient, 3x3 stride 1 with 16-byte global loads: wgrad3x3_wide_kernel (SPK_WGRAD_WIDE16, SPK_WGRAD_WIDE8).
#include "wgrad_mfma_f32.hpp"

using namespace spkwg;

namespace {

// ---- 3x3 stride-1 weight gradient with 16-byte global loads ---------------------------------------------------------------
// The kernels above are bound by the ISSUE of their loads, not by the MFMA pipe (profiles/r01_k_wgrad_phases.txt: 48 dword
// loads per thread and tile, ~1 000 line requests against 18.4K cycles of MFMA).  Here rows are loaded 16 bytes per lane: a
// gradient row of the tile is TW / 4 aligned float4, an input row the same plus the two halo columns as single dwords --
// 13 (TW = 16) load instructions per thread and tile of 288 MFMAs where the dword form issues 48.  (A second accumulator tile
// set per wave -- 128co x 64ci blocks, 1.5x the FLOPs per staged byte -- was built and dropped: MFMA accumulators live in the
// 256 AGPRs only, two 9-tap sets need 288.)
// Staging roles make everything but the tile origin a launch constant: piece i of the input tile is a plane ROW of 64
// channels, so its global offset is a per-thread base plus a wave-uniform term, its LDS address an immediate offset and its
// row test a scalar compare.  Same 64co x 64ci block, LDS images (odd row pitch), per-element accumulation order and slab
// layout as wgrad3x3_pipe_kernel: results are bitwise equal to its for equal pixel splits.
// Needs W % 4 == 0, W >= 8 and 16-byte aligned tensors (host-checked: wide_takes).

// TW = 16: 16 x 4 pixel tiles (18 x 6 plane); TW = 8: 8 x 8 tiles (10 x 10 plane) for the 8^2 layers, one tile per image.
template <int TW_, int MODE>
__global__ __launch_bounds__(256, 1) void wgrad3x3_wide_kernel(const WgradArgs p) {
    using SH = WideShapeT<TW_>;
    constexpr int TAPS = 9, CO_T = SH::CO_T, CI_T = SH::CI_T, TW = SH::TW, TH = SH::TH, PW = SH::PW, PH = SH::PH;
    constexpr int GPITCH = SH::GPITCH, XPITCH = SH::XPITCH, BUF = SH::BUF;
    constexpr int NG4 = SH::NG4, NXK = SH::NXK, RS = SH::RS, NX4 = SH::NX4, NXH = SH::NXH, NL = SH::NL, NS = SH::NS;
    constexpr int STEPS = SH::STEPS, HS = SH::HS, PL = SH::PL, PS = SH::PS;
    constexpr bool AFF = MODE == WG_AFFINE_RELU, BSC = MODE == WG_BATCH_SCALE;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l32 = lane & 31;
    const int wco = wave & 1, wci = wave >> 1;

    const int co0 = blockIdx.x * CO_T;
    const int grp = co0 / p.Cout;
    const int co_end = (grp + 1) * p.Cout;
    const int cx0 = grp * p.gin;
    const int ci0 = blockIdx.y * CI_T;
    const int nci = min(CI_T, p.Cin - ci0);

    // ---- staging roles (launch constants; only the tile origin moves) ----
    // gradient piece i: float4 gk of tile row grow of channel (tid >> 4) + 16 i
    const int gk = tid & (TW / 4 - 1), grow = (tid / (TW / 4)) & (TH - 1);
    int g_off[NG4], g_ch[NG4];
#pragma unroll
    for (int i = 0; i < NG4; ++i) {
        g_ch[i] = min(co0 + (tid >> 4) + 16 * i, co_end - 1);                                      // rows past the last channel: clamped (never written out)
        g_off[i] = (g_ch[i] * p.H + grow) * p.W + 4 * gk;
    }
    float g_sc[NG4];                                                                              // BSC: d'[b, g_ch[i]] of the tile being staged
#pragma unroll
    for (int i = 0; i < NG4; ++i) g_sc[i] = 1.f;
    const int g_dst = (tid >> 4) * GPITCH + grow * TW + 4 * gk;                                   // + 16 i GPITCH + j
    // input piece i: float4 xk of plane row RS i + xr of channel xc
    const int xk = tid & (NXK - 1), xc = (tid / NXK) & (CI_T - 1), xr = tid / (NXK * CI_T);
    const int x_chan = cx0 + ci0 + min(xc, nci - 1);
    const int x_base = (x_chan * p.Hs + xr - 1) * p.Ws + 4 * xk;                                  // + RS i Ws
    const int x_dst = CO_T * GPITCH + xc * XPITCH + xr * PW + 1 + 4 * xk;                         // + RS i PW + j
    float x_sc = 1.f, x_sh = 0.f;
    if (AFF) { x_sc = p.in_scale[x_chan]; x_sh = p.in_shift[x_chan]; }
    // halo piece i: column -1 / TW (hs) of plane row 2 i + hr of channel hc
    const int hs = tid & 1, hc = (tid >> 1) & (CI_T - 1), hr = tid >> 7;
    const int h_chan = cx0 + ci0 + min(hc, nci - 1);
    const int h_base = (h_chan * p.Hs + hr - 1) * p.Ws + (hs ? TW : -1);                          // + 2 i Ws
    const int h_dst = CO_T * GPITCH + hc * XPITCH + hr * PW + (hs ? TW + 1 : 0);                  // + 2 i PW
    float h_sc = 1.f, h_sh = 0.f;
    if (AFF) { h_sc = p.in_scale[h_chan]; h_sh = p.in_shift[h_chan]; }

    f32x16 acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // prefetch registers and, for the tile being staged: its base pointers, origin row and which of this thread's columns exist
    f32x4 gq[NG4], xq[NX4];
    float hq[NXH];
    const float* gbase = p.g;
    const float* xbase = p.x;
    int ty0 = 0;
    bool g_ok = false, xcol_ok = false, hcol_ok = false;
    auto aim = [&](int tile) {
        const int tx = tile % p.tiles_x;
        const int q = tile / p.tiles_x;
        const int ty = q % p.tiles_y, b = q / p.tiles_y;
        const int y0 = ty * TH, x0 = tx * TW;
        ty0 = y0;
        gbase = p.g + ((size_t)b * p.Cy * p.H + y0) * p.W + x0;
        xbase = p.x + ((size_t)b * p.Cx * p.Hs + y0) * p.Ws + x0;
        const bool live = tile < p.n_tiles;
        g_ok = live && y0 + grow < p.H && x0 + 4 * gk < p.W;
        xcol_ok = live && x0 + 4 * xk < p.Ws;
        hcol_ok = live && (unsigned)(x0 + (hs ? TW : -1)) < (unsigned)p.Ws;
        if constexpr (BSC) {                     // the staged tile's image decides the modulation / demodulation factors
            const int bb = live ? b : 0;
            x_sc = p.in_scale[(size_t)bb * p.Cx + x_chan];
            h_sc = p.in_scale[(size_t)bb * p.Cx + h_chan];
#pragma unroll
            for (int i = 0; i < NG4; ++i) g_sc[i] = p.g_scale[(size_t)bb * p.Cy + g_ch[i]];
        }
    };
    // plane row r of the tile being staged lies inside the image (and inside the plane: the last piece of a two-row role)
    auto row_ok = [&](int r) { return r < PH && (unsigned)(ty0 + r - 1) < (unsigned)p.Hs; };
    auto load_piece = [&](auto j_) {
        constexpr int j = decltype(j_)::value;
        if constexpr (j < NG4) {
            gq[j] = *reinterpret_cast<const f32x4*>(g_ok ? gbase + g_off[j] : p.g);
        } else if constexpr (j < NG4 + NX4) {
            constexpr int i = j - NG4;
            const bool ok = xcol_ok && row_ok(RS * i + xr);
            xq[i] = *reinterpret_cast<const f32x4*>(ok ? xbase + (x_base + RS * i * p.Ws) : p.x);
        } else if constexpr (j < NL) {
            constexpr int i = j - NG4 - NX4;
            const bool ok = hcol_ok && row_ok(2 * i + hr);
            hq[i] = *(ok ? xbase + (h_base + 2 * i * p.Ws) : p.x);
        }
    };
    auto store_piece = [&](float* buf, auto s_) {
        constexpr int s = decltype(s_)::value;
        if constexpr (s < 4 * NG4) {
            constexpr int i = s / 4, j = s % 4;
            buf[g_dst + 16 * i * GPITCH + j] = g_ok ? (BSC ? gq[i][j] * g_sc[i] : gq[i][j]) : 0.f;   // only the PIXEL axis (the contraction) needs zeros
        } else if constexpr (s < 4 * NG4 + 4 * NX4) {
            constexpr int i = (s - 4 * NG4) / 4, j = (s - 4 * NG4) % 4;
            float v = xq[i][j];
            if (AFF) v = fmaxf(v * x_sc + x_sh, 0.f);
            if (BSC) v *= x_sc;
            // (a two-row role's last piece: plane row PH does not exist -- those lanes hit the dump slot, no branch)
            const int dst = (RS * i + RS - 1 < PH || RS * i + xr < PH) ? x_dst + RS * i * PW + j : BUF - 1;
            buf[dst] = (xcol_ok && row_ok(RS * i + xr)) ? v : 0.f;
        } else if constexpr (s < NS) {
            constexpr int i = s - 4 * NG4 - 4 * NX4;
            float v = hq[i];
            if (AFF) v = fmaxf(v * h_sc + h_sh, 0.f);
            if (BSC) v *= h_sc;
            const int dst = (2 * i + 1 < PH || 2 * i + hr < PH) ? h_dst + 2 * i * PW : BUF - 1;
            buf[dst] = (hcol_ok && row_ok(2 * i + hr)) ? v : 0.f;
        }
    };

    int tile = blockIdx.z;
    int cur = 0;
    if (tile < p.n_tiles) {                  // first tile: staged the serial way
        aim(tile);
        wg_static_for<0, NL>([&](auto j_) { load_piece(j_); });
        wg_static_for<0, NS>([&](auto s_) { store_piece(smem, s_); });
    }
    __syncthreads();

    // one tile's 32 k-steps out of buffer `cur`; the next tile is staged into the other buffer on the way (its loads behind the
    // first half of the k-steps, its LDS stores behind the second half)
    auto run_tile = [&]() {
        const float* cbuf = smem + cur * BUF;
        float* nbuf = smem + (cur ^ 1) * BUF;
        const volatile wg_lds_f32* ga = (const volatile wg_lds_f32*)(cbuf + (wco * 32 + l32) * GPITCH + half);
        const volatile wg_lds_f32* xb = (const volatile wg_lds_f32*)(cbuf + CO_T * GPITCH + (wci * 32 + l32) * XPITCH + half);
        float fa[2], fb[2][TAPS];
#define SPK_WW_FRAG(st_, slot_)                                                                               \
    {                                                                                                         \
        constexpr int px_ = (2 * (st_)) & (TW - 1), py_ = (2 * (st_)) / TW;                                   \
        fa[slot_] = ga[2 * (st_)];                                                                            \
        _Pragma("unroll") for (int t = 0; t < TAPS; ++t)                                                      \
            fb[slot_][t] = xb[(py_ + t / 3) * PW + px_ + t % 3];                                              \
    }
        SPK_WW_FRAG(0, 0);
        wg_static_for<0, STEPS>([&](auto s_) {
            constexpr int st = decltype(s_)::value;
            // Nothing may be scheduled across the load / store boundary: left alone, the scheduler hoists the stores' VALU
            // halves (the zero-select of out-of-image pieces, the folded BatchNorm affine) up to the loads they consume -- and
            // every load is then followed by s_waitcnt vmcnt(0), a full memory latency with the MFMA pipe idle (one wave per SIMD).
            if constexpr (st == HS) __builtin_amdgcn_sched_barrier(0);
            if constexpr (st + 1 < STEPS) SPK_WW_FRAG(st + 1, (st + 1) & 1);
            constexpr int nl = st < HS ? ((PL * st + PL <= NL) ? PL : (PL * st < NL ? NL - PL * st : 0)) : 0;
            constexpr int s0 = PS * (st - HS);
            constexpr int ns = st >= HS ? ((s0 + PS <= NS) ? PS : (s0 < NS ? NS - s0 : 0)) : 0;
            if constexpr (nl > 0) wg_static_for<PL * st, PL * st + nl>([&](auto j_) { load_piece(j_); });
            if constexpr (ns > 0) wg_static_for<s0, s0 + ns>([&](auto q_) { store_piece(nbuf, q_); });
#pragma unroll
            for (int t = 0; t < TAPS; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[st & 1], fb[st & 1][t], acc[t], 0, 0, 0);
            // order: next step's fragments first, then the MFMAs with the staging accesses spread between them
            if constexpr (st + 1 < STEPS) __builtin_amdgcn_sched_group_barrier(0x100, SH::NFRAG, 0);
            constexpr int np = nl > 0 ? nl : ns;
            if constexpr (np > 0) {
                constexpr int per = TAPS / (np + 1);
                wg_static_for<0, np>([&](auto k_) {
                    __builtin_amdgcn_sched_group_barrier(0x8, per, 0);
                    __builtin_amdgcn_sched_group_barrier(nl > 0 ? 0x20 : 0x200, 1, 0);
                });
                __builtin_amdgcn_sched_group_barrier(0x8, TAPS - per * np, 0);
            } else {
                __builtin_amdgcn_sched_group_barrier(0x8, TAPS, 0);
            }
        });
#undef SPK_WW_FRAG
    };

    // ONE loop body: after the last tile the staging still runs, with every piece masked off (it reads the tensors' first
    // floats and fills the idle buffer with zeros).  With a second, staging-free copy of the tile for that case the
    // accumulators cross the if / else merge in VGPRs: 144 v_accvgpr_write before and 144 v_accvgpr_read after EVERY tile's
    // 288 MFMAs (and twice the code).
    for (; tile < p.n_tiles; tile += gridDim.z) {
        aim(tile + (int)gridDim.z);
        run_tile();
        __syncthreads();                      // every wave is done with `cur`, and the other buffer is complete
        cur ^= 1;
    }

    // ---- partial block -> slab [slab][co][tap][ci] (ci contiguous: 128-B stores per half wave) ----
    float* out = p.slabs + (size_t)blockIdx.z * p.Cy * TAPS * p.Cin;
    const int ci = ci0 + wci * 32 + l32;
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + wco * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (co < co_end && ci < p.Cin) out[((size_t)co * TAPS + t) * p.Cin + ci] = acc[t][r];
        }
}

}  // namespace

template <int TW>
static const void* wide_kernel(int mode) {
    if (mode == WG_AFFINE_RELU) return reinterpret_cast<const void*>(&wgrad3x3_wide_kernel<TW, WG_AFFINE_RELU>);
    if (mode == WG_BATCH_SCALE) return reinterpret_cast<const void*>(&wgrad3x3_wide_kernel<TW, WG_BATCH_SCALE>);
    return reinterpret_cast<const void*>(&wgrad3x3_wide_kernel<TW, WG_PLAIN>);
}

int spkwg::launch_wide(const WgradPlan& p, hipStream_t stream) {
    return launch_planned(p.form == SPK_WGRAD_WIDE16 ? wide_kernel<16>(p.mode) : wide_kernel<8>(p.mode), "wgrad3x3_wide_kernel", p, stream);
}
