// Weight gradient, 3x3 stride 1 with 16-byte global loads: wgrad3x3_wide_kernel (SPK_WGRAD_WIDE16, SPK_WGRAD_WIDE8).
#include "wgrad_tile3x3.hpp"

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
    constexpr int CO_T = SH::CO_T, CI_T = SH::CI_T, TW = SH::TW, TH = SH::TH, PW = SH::PW, PH = SH::PH, GPITCH = SH::GPITCH, XPITCH = SH::XPITCH;
    constexpr int NG4 = SH::NG4, NXK = SH::NXK, RS = SH::RS, NX4 = SH::NX4, NXH = SH::NXH, NL = SH::NL, NS = SH::NS;
    constexpr bool AFF = MODE == WG_AFFINE_RELU, BSC = MODE == WG_BATCH_SCALE;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const WgBlock bk = wg_block<CO_T, CI_T>(p);
    const int tid = bk.tid, half = bk.half, l32 = bk.l32, wco = bk.wave & 1, wci = bk.wave >> 1;
    const int co0 = bk.co0, co_end = bk.co_end, cx0 = bk.cx0, ci0 = bk.ci0, nci = bk.nci;

    // ---- staging roles (launch constants; only the tile origin moves) ----
    int gk, grow, g_ch[NG4], g_off[NG4], g_dst;                                                   // gradient pieces: wg_grad_roles
    wg_grad_roles<SH>(p, tid, co0, co_end, gk, grow, g_ch, g_off, g_dst);
    float g_sc[NG4];                                                                              // BSC: d'[b, g_ch[i]] of the tile being staged
#pragma unroll
    for (int i = 0; i < NG4; ++i) g_sc[i] = 1.f;
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

    f32x16 acc[WG_TAPS];
    wg_zero(acc);

    // prefetch registers and, for the tile being staged: its base pointers, origin row and which of this thread's columns exist
    f32x4 gq[NG4], xq[NX4];
    float hq[NXH];
    const float* gbase = p.g;
    const float* xbase = p.x;
    int ty0 = 0;
    bool g_ok = false, xcol_ok = false, hcol_ok = false;
    auto aim = [&](int tile) {
        const WgTile o = wg_tile_origin<TW, TH>(p, tile);
        ty0 = o.y0;
        gbase = p.g + ((size_t)o.b * p.Cy * p.H + o.y0) * p.W + o.x0;
        xbase = p.x + ((size_t)o.b * p.Cx * p.Hs + o.y0) * p.Ws + o.x0;
        const bool live = tile < p.n_tiles;
        g_ok = live && o.y0 + grow < p.H && o.x0 + 4 * gk < p.W;
        xcol_ok = live && o.x0 + 4 * xk < p.Ws;
        hcol_ok = live && (unsigned)(o.x0 + (hs ? TW : -1)) < (unsigned)p.Ws;
        if constexpr (BSC) {                     // the staged tile's image decides the modulation / demodulation factors
            const int bb = live ? o.b : 0;
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
            const int dst = (RS * i + RS - 1 < PH || RS * i + xr < PH) ? x_dst + RS * i * PW + j : SH::BUF - 1;
            buf[dst] = (xcol_ok && row_ok(RS * i + xr)) ? v : 0.f;
        } else if constexpr (s < NS) {
            constexpr int i = s - 4 * NG4 - 4 * NX4;
            float v = hq[i];
            if (AFF) v = fmaxf(v * h_sc + h_sh, 0.f);
            if (BSC) v *= h_sc;
            const int dst = (2 * i + 1 < PH || 2 * i + hr < PH) ? h_dst + 2 * i * PW : SH::BUF - 1;
            buf[dst] = (hcol_ok && row_ok(2 * i + hr)) ? v : 0.f;
        }
    };

    wg_stage_first<NL, NS>(p, smem, aim, load_piece, store_piece);
    wg_persistent_tiles(p, aim, [&](int cur) {
        wg_run_tile_spread<SH, 1>(smem, cur, wco * 32 + l32, wci * 32 + l32, half, acc, load_piece, store_piece);
    });
    wg_store_slab9(p, acc, co0 + wco * 32, co_end, ci0 + wci * 32 + l32, half);
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
