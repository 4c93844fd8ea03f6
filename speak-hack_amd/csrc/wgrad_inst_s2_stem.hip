// Weight gradient, 3x3 stride 2 (SPK_WGRAD_S2_16, SPK_WGRAD_S2_8) and the 7x7 stride-2 stem (SPK_WGRAD_STEM).
#include "wgrad_tile3x3.hpp"

using namespace spkwg;

namespace {

// ---- 3x3 STRIDE-2 weight gradient (the trunk's downsampling convs, the discriminator's conv2 of every block) -----------
// dW[co][ci][ky][kx] = sum g[b,co,y,x] * in(x)[b,ci,2y+ky-1,2x+kx-1].  A stride-2 conv reads 4.6 input values per output pixel
// and channel where a stride-1 one reads 1.7, so the generic kernel above (64co x 32ci block, 64 dword gathers + 16 loads per
// thread for 144 MFMAs per wave, staged serially) spends its time issuing loads: 33-42 TFLOP/s on the trunk, 65 on the
// discriminator.  Here the input tile serves FOUR co tiles: block = 128co x 32ci, wave w owns co rows [32w, 32w+32) and all 64
// pixels of the tile (288 MFMAs per wave and tile), the (2 TH + 1) x (2 TW + 1) input plane is loaded as 16-byte row
// segments (columns 2 x0 .. 2 x0 + 2 TW - 1 are aligned; the left halo column is one dword per row), and -- as in
// wgrad3x3_wide_kernel -- the LDS tile is double-buffered with the next tile's loads behind k-steps 0-15 and its LDS stores
// behind k-steps 16-31: 19 load + 70 store instructions per thread against 288 MFMAs.
// TW = 16 (16 x 4 output pixels, 9 x 33 plane) or 8 (8 x 8, 17 x 17: the 8^2 outputs).  Needs W % 4 == 0, W >= TW / 2,
// Hin = 2 H, Win = 2 W, 16-byte aligned tensors (host-checked: s2_takes).

template <int TW_, int MODE>
__global__ __launch_bounds__(256) void wgrad3x3_s2_kernel(const WgradArgs p) {
    using SH = S2Shape<TW_>;
    constexpr int CO_T = SH::CO_T, CI_T = SH::CI_T, TW = SH::TW, TH = SH::TH, PW = SH::PW, PH = SH::PH, GPITCH = SH::GPITCH, XPITCH = SH::XPITCH;
    constexpr int NG4 = SH::NG4, NXK = SH::NXK, RS = SH::RS, NX4 = SH::NX4, NXH = SH::NXH, NL = SH::NL, NS = SH::NS;
    constexpr bool AFF = MODE == WG_AFFINE_RELU;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const WgBlock bk = wg_block<CO_T, CI_T>(p);
    const int tid = bk.tid, wave = bk.wave, half = bk.half, l32 = bk.l32;
    const int co0 = bk.co0, co_end = bk.co_end, cx0 = bk.cx0, ci0 = bk.ci0, nci = bk.nci;

    // ---- staging roles (launch constants; only the tile origin moves) ----
    int gk, grow, g_ch[NG4], g_off[NG4], g_dst;                                                    // gradient pieces: wg_grad_roles
    wg_grad_roles<SH>(p, tid, co0, co_end, gk, grow, g_ch, g_off, g_dst);
    // input piece i: float4 xk of plane row RS i + xr of channel xc
    const int xk = tid & (NXK - 1), xc = (tid / NXK) & (CI_T - 1), xr = tid / (NXK * CI_T);
    const int x_chan = cx0 + ci0 + min(xc, nci - 1);
    const int x_base = (x_chan * p.Hs + xr - 1) * p.Ws + 4 * xk;                                   // + RS i Ws
    const int x_dst = CO_T * GPITCH + xc * XPITCH + xr * PW + 1 + 4 * xk;                          // + RS i PW + j
    float x_sc = 1.f, x_sh = 0.f;
    if (AFF) { x_sc = p.in_scale[x_chan]; x_sh = p.in_shift[x_chan]; }
    // halo piece i: plane column 0 of plane row hr + 8 i of channel hc
    const int hc = tid & (CI_T - 1), hr = tid >> 5;
    const int h_chan = cx0 + ci0 + min(hc, nci - 1);
    const int h_base = (h_chan * p.Hs + hr - 1) * p.Ws - 1;                                        // + 8 i Ws
    const int h_dst = CO_T * GPITCH + hc * XPITCH + hr * PW;                                       // + 8 i PW
    float h_sc = 1.f, h_sh = 0.f;
    if (AFF) { h_sc = p.in_scale[h_chan]; h_sh = p.in_shift[h_chan]; }

    f32x16 acc[WG_TAPS];
    wg_zero(acc);

    f32x4 gq[NG4], xq[NX4];
    float hq[NXH];
    const float* gbase = p.g;
    const float* xbase = p.x;
    int sy0 = 0;                       // first input row of the tile being staged (2 y0)
    bool g_ok = false, xcol_ok = false, hcol_ok = false;
    auto aim = [&](int tile) {
        const WgTile o = wg_tile_origin<TW, TH>(p, tile);
        sy0 = 2 * o.y0;
        gbase = p.g + ((size_t)o.b * p.Cy * p.H + o.y0) * p.W + o.x0;
        xbase = p.x + ((size_t)o.b * p.Cx * p.Hs + 2 * o.y0) * p.Ws + 2 * o.x0;
        const bool live = tile < p.n_tiles;
        g_ok = live && o.y0 + grow < p.H && o.x0 + 4 * gk < p.W;
        xcol_ok = live && 2 * o.x0 + 4 * xk < p.Ws;
        hcol_ok = live && o.x0 > 0;
    };
    // plane row r of the tile being staged lies inside the image (and inside the plane: the last piece of a two-row role)
    auto row_ok = [&](int r) { return r < PH && (unsigned)(sy0 + r - 1) < (unsigned)p.Hs; };
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
            const bool ok = hcol_ok && row_ok(hr + 8 * i);
            hq[i] = *(ok ? xbase + (h_base + 8 * i * p.Ws) : p.x);
        }
    };
    auto store_piece = [&](float* buf, auto s_) {
        constexpr int s = decltype(s_)::value;
        if constexpr (s < 4 * NG4) {
            constexpr int i = s / 4, j = s % 4;
            buf[g_dst + 16 * i * GPITCH + j] = g_ok ? gq[i][j] : 0.f;         // only the PIXEL axis (the contraction) needs zeros
        } else if constexpr (s < 4 * NG4 + 4 * NX4) {
            constexpr int i = (s - 4 * NG4) / 4, j = (s - 4 * NG4) % 4;
            float v = xq[i][j];
            if (AFF) v = fmaxf(v * x_sc + x_sh, 0.f);
            // (a two-row role's last piece: plane row PH does not exist -- those lanes hit the dump slot, no branch)
            const int dst = (RS * i + RS - 1 < PH || RS * i + xr < PH) ? x_dst + RS * i * PW + j : SH::BUF - 1;
            buf[dst] = (xcol_ok && row_ok(RS * i + xr)) ? v : 0.f;
        } else if constexpr (s < NS) {
            constexpr int i = s - 4 * NG4 - 4 * NX4;
            float v = hq[i];
            if (AFF) v = fmaxf(v * h_sc + h_sh, 0.f);
            const int dst = (8 * i + 7 < PH || hr + 8 * i < PH) ? h_dst + 8 * i * PW : SH::BUF - 1;
            buf[dst] = (hcol_ok && row_ok(hr + 8 * i)) ? v : 0.f;
        }
    };

    wg_stage_first<NL, NS>(p, smem, aim, load_piece, store_piece);
    // wave w owns co rows [32 w, 32 w + 32) and all 32 input channels
    wg_persistent_tiles(p, aim, [&](int cur) {
        wg_run_tile_spread<SH, 2>(smem, cur, wave * 32 + l32, l32, half, acc, load_piece, store_piece);
    });
    wg_store_slab9(p, acc, co0 + wave * 32, co_end, ci0 + l32, half);
}

// ---- the stem's weight gradient: 7x7 stride 2, Cin = 3, Cout = 64 per group --------------------------------------------------
// dW[co][k] = sum_{b, oy, ox} g[b, co, oy, ox] * x[b, ci, 2 oy + ky - 3, 2 ox + kx - 3], k = (ci, ky, kx): a GEMM of 64 x 147 outputs over
// B H W pixels.  The generic tap kernel runs it with 49 taps of a padded 4-channel chunk (46 TFLOP/s, 0.32 ms of a G step).  Here,
// as in conv7x7_stem.hip: a 4 x 32 output tile's input patch (13 rows x 69 columns x 3 channels) in LDS with its columns split by
// parity, the tile's gradients [64 co][128 px] beside it; MFMA 32x32x2 with A = gradients (lane = channel, half = one of two adjacent
// pixels) and B = patch values (lane = k: a per-lane constant offset (ci, ky, kx) + the pixel as an immediate); every wave owns one
// row of the tile and ALL 2 x 5 accumulator tiles (64 co x 160 k, 160 registers), workgroups are persistent over tiles, the four
// waves' sums meet in LDS at the end and leave as one slab per workgroup ([co][147], the layout of dW itself).
__global__ __launch_bounds__(256, 2) void wgrad_stem_kernel(const WgradArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l32 = lane & 31;
    const int grp = blockIdx.y;
    const float* gb = p.g + (size_t)grp * 64 * p.H * p.W;             // + b Cy H W
    const float* xb = p.x + (size_t)grp * p.gin * p.Hs * p.Ws;       // + b Cx Hs Ws

    // staging roles: gradients -- float4 f = tid + 256 i of the tile's [64 co][4 rows][8 float4]; patch -- as conv7x7_stem.hip
    float4 gq[8];
    float pa[SW_TPW], pb[SW_TPW];
    const int g_co = tid >> 5, g_row = (tid >> 3) & 3, g_c4 = tid & 7;                     // + 8 i channels
    const unsigned g_dst = (unsigned)(g_co * SW_GP + g_row * SW_TW + 4 * g_c4) * 4u;      // + 8 i SW_GP floats
    const unsigned p_dst_a = (unsigned)(SW_G_FL + wave * SW_PROW + (lane & 1) * SW_PH + (lane >> 1)) * 4u;
    const unsigned p_dst_b = p_dst_a + 32 * 4;
    auto load_tile = [&](int t) {
        const bool live = t < p.n_tiles;
        const int tt = live ? t : 0;
        const int tx = tt % p.tiles_x, q = tt / p.tiles_x;
        const int ty = q % p.tiles_y, b = q / p.tiles_y;
        const int oy0 = ty * SW_TH, ox0 = tx * SW_TW;
        const float* gt = gb + (size_t)b * p.Cy * p.H * p.W;
        const bool g_ok = live && oy0 + g_row < p.H && ox0 + 4 * g_c4 < p.W;            // (W % 4 == 0: host-checked)
        const unsigned g_off = (unsigned)((min(oy0 + g_row, p.H - 1)) * p.W + min(ox0 + 4 * g_c4, p.W - 4)) * 4u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(gt + (size_t)(g_co + 8 * i) * p.H * p.W) + g_off);
            gq[i] = g_ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);      // zero gradients outside: the pixel sum ignores them
        }
        const float* xt = xb + (size_t)b * p.Cx * p.Hs * p.Ws;
        const int ix_a = 2 * ox0 - 3 + lane, ix_b = ix_a + 64;
        const bool ok_a = (unsigned)ix_a < (unsigned)p.Ws, ok_b = lane < SW_PC - 64 && (unsigned)ix_b < (unsigned)p.Ws;
        const unsigned off_a = (unsigned)min(max(ix_a, 0), p.Ws - 1) * 4u, off_b = (unsigned)min(max(ix_b, 0), p.Ws - 1) * 4u;
#pragma unroll
        for (int j = 0; j < SW_TPW; ++j) {
            const int qq = min(wave + 4 * j, SW_TASKS - 1);                  // (uniform)
            const int ci = qq / SW_PR, r = qq - ci * SW_PR;
            const int iy = 2 * oy0 - 3 + r;
            const bool row_ok = (unsigned)iy < (unsigned)p.Hs;
            const char* row = reinterpret_cast<const char*>(xt + ((size_t)ci * p.Hs + min(max(iy, 0), p.Hs - 1)) * p.Ws);
            const float a = *reinterpret_cast<const float*>(row + off_a);
            const float c = *reinterpret_cast<const float*>(row + off_b);
            pa[j] = (row_ok && ok_a) ? a : 0.f;
            pb[j] = (row_ok && ok_b) ? c : 0.f;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            volatile wg_lds_f32* d = (volatile wg_lds_f32*)((wg_lds_u8*)smem + (g_dst + (unsigned)(8 * i * SW_GP * 4)));
            d[0] = gq[i].x; d[1] = gq[i].y; d[2] = gq[i].z; d[3] = gq[i].w;
        }
#pragma unroll
        for (int j = 0; j < SW_TPW; ++j) {
            if (wave + 4 * j < SW_TASKS) {                                   // (uniform)
                *(volatile wg_lds_f32*)((wg_lds_u8*)smem + (p_dst_a + (unsigned)(j * 4 * SW_PROW * 4))) = pa[j];
                if (lane < SW_PC - 64) *(volatile wg_lds_f32*)((wg_lds_u8*)smem + (p_dst_b + (unsigned)(j * 4 * SW_PROW * 4))) = pb[j];
            }
        }
    };

    // fragment addresses (bytes): A -- channel m 32 + l32, pixel row = wave, pixels 2 s + half; B -- k = 32 j + l32 (clamped: columns
    // >= 147 are never written out), the same pixels
    unsigned a_addr = (unsigned)(l32 * SW_GP + wave * SW_TW + half) * 4u;
    unsigned b_addr[SW_NT];
#pragma unroll
    for (int j = 0; j < SW_NT; ++j) {
        const int k = min(32 * j + l32, SW_K - 1);
        const int ci = k / 49, ky = (k % 49) / 7, kx = k % 7;
        b_addr[j] = (unsigned)(SW_G_FL + ((ci * SW_PR + 2 * wave + ky) * 2 + (kx & 1)) * SW_PH + (kx >> 1) + half) * 4u;
        asm volatile("" : "+v"(b_addr[j]));
    }
    asm volatile("" : "+v"(a_addr));

    f32x16 acc[2][SW_NT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < SW_NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.f;

    int tile = blockIdx.x;
    load_tile(tile);
    store_tile();
    __syncthreads();
    for (; tile < p.n_tiles; tile += gridDim.x) {
        load_tile(tile + (int)gridDim.x);                   // the next tile's loads fly behind this tile's MFMAs
        float fa[2][2], fb[2][SW_NT];
#define SPK_SW_FRAG(s_, f_)                                                                                                   \
    {                                                                                                                         \
        fa[f_][0] = *(const volatile wg_lds_f32*)((wg_lds_u8*)smem + (a_addr + (unsigned)(2 * (s_) * 4)));                    \
        fa[f_][1] = *(const volatile wg_lds_f32*)((wg_lds_u8*)smem + (a_addr + (unsigned)((32 * SW_GP + 2 * (s_)) * 4)));     \
        _Pragma("unroll") for (int j = 0; j < SW_NT; ++j)                                                                     \
            fb[f_][j] = *(const volatile wg_lds_f32*)((wg_lds_u8*)smem + (b_addr[j] + (unsigned)(2 * (s_) * 4)));             \
    }
        SPK_SW_FRAG(0, 0);
        __builtin_amdgcn_sched_barrier(0);
        wg_static_for<0, SW_TW / 2>([&](auto s_) {
            constexpr int st = decltype(s_)::value;
            if constexpr (st + 1 < SW_TW / 2) {
                SPK_SW_FRAG(st + 1, (st + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int j = 0; j < SW_NT; ++j)
#pragma unroll
                for (int m = 0; m < 2; ++m)
                    acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[st & 1][m], fb[st & 1][j], acc[m][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        });
#undef SPK_SW_FRAG
        __syncthreads();                                    // every wave is done reading the tile
        store_tile();
        __syncthreads();
    }

    // ---- the four waves' sums, one n-tile at a time through LDS, -> slab [slab][co_all][147] ----
    float* out = p.slabs + ((size_t)blockIdx.x * p.Cy + (size_t)grp * 64) * SW_K;
#pragma unroll
    for (int j = 0; j < SW_NT; ++j) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) smem[((wave * 2 + m) * 16 + r) * 64 + lane] = acc[m][j][r];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int idx = tid + 256 * e;                  // (m, r, lane) of 2 x 16 x 64
            const int ln = idx & 63, r = (idx >> 6) & 15, m = idx >> 10;
            const float v = (smem[idx] + smem[2048 + idx]) + (smem[4096 + idx] + smem[6144 + idx]);
            const int co = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5), k = 32 * j + (ln & 31);
            if (k < SW_K) out[co * SW_K + k] = v;
        }
        __syncthreads();
    }
}

}  // namespace

template <int TW>
static const void* s2_kernel(int mode) {
    return mode == WG_AFFINE_RELU ? reinterpret_cast<const void*>(&wgrad3x3_s2_kernel<TW, WG_AFFINE_RELU>)
                                  : reinterpret_cast<const void*>(&wgrad3x3_s2_kernel<TW, WG_PLAIN>);
}

int spkwg::launch_s2_stem(const WgradPlan& p, hipStream_t stream) {
    if (p.form == SPK_WGRAD_STEM) return launch_planned(reinterpret_cast<const void*>(&wgrad_stem_kernel), "wgrad_stem_kernel", p, stream);
    return launch_planned(p.form == SPK_WGRAD_S2_16 ? s2_kernel<16>(p.mode) : s2_kernel<8>(p.mode), "wgrad3x3_s2_kernel", p, stream);
}
