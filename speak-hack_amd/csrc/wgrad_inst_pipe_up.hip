// Weight gradient, 3x3 stride 1 on 16 x 4 tiles: the pipelined form (SPK_WGRAD_PIPE) and the upsample-folded form (SPK_WGRAD_UP).
#include "wgrad_tile3x3.hpp"

using namespace spkwg;

namespace {

// ---- 3x3 stride-1 weight gradient, staging interleaved with the MFMAs ------------------------------------------------
// Same block (64co x 64ci x 9 taps, 4 waves, 16x4-pixel tiles) and the same arithmetic order as wgrad_kernel<3,3,1>, but
// the LDS tile is double-buffered and the next tile's staging rides in the shadow of this tile's MFMAs: k-steps 0-15
// issue its 48 global loads per thread (3 per step), k-steps 16-31 store them to the other buffer (3 per step), and one
// barrier ends the tile.  In the serial form a tile cost 18.6K cycles of MFMA + 8.6K of load issue, LDS stores and two
// barriers (profiles/r01_m_core_clock_under_load.txt).  The tile shape is a compile-time constant, so every LDS offset is
// an immediate and a staging piece is a clamp, a load or store and a select -- the per-piece index arithmetic is what
// made an earlier pipelined attempt slower than the serial kernel.
__global__ __launch_bounds__(256) void wgrad3x3_pipe_kernel(const WgradArgs p) {
    using SH = WideShapeT<16>;                 // the tile images of the wide form at TW = 16 (idle lanes: its dump slot)
    constexpr int TAPS = WG_TAPS, CI_T = SH::CI_T, CO_T = SH::CO_T, TW = SH::TW, PW = SH::PW, PLANE = SH::PLANE;
    constexpr int GPITCH = SH::GPITCH, XPITCH = SH::XPITCH, BUF = SH::BUF;
    constexpr int NGL = 16, NXL = 32, PPS = (NGL + NXL) / WG_HS;                     // 3 staging pieces per k-step
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const WgBlock bk = wg_block<CO_T, CI_T>(p);
    const int tid = bk.tid, wave = bk.wave, half = bk.half, l32 = bk.l32, wco = wave & 1, wci = wave >> 1;
    const int co0 = bk.co0, co_end = bk.co_end, cx0 = bk.cx0, ci0 = bk.ci0, nci = bk.nci;
    const size_t HW = (size_t)p.H * p.W, src_plane = (size_t)p.Hs * p.Ws;

    // staging roles.  Gradient tile: thread -> pixel tid % 64, output channels tid / 64 + 4 i.  Input tile: thread -> plane
    // position tid % 128 (108 of them exist), channels 32 (tid / 128) + i (a wave-uniform slice).
    const int gpix = tid & 63, gpx = gpix & (TW - 1), gpy = gpix >> 4, gco = wave;
    const int xpos = tid & 127, cbw = (wave >> 1) * NXL;
    const bool xpos_ok = xpos < PLANE;
    const int xr = xpos / PW, xc = xpos - xr * PW;
    const int g_dst = gco * GPITCH + gpix;                                      // + 4 i GPITCH
    const int x_dst = xpos_ok ? CO_T * GPITCH + cbw * XPITCH + xpos : BUF - 1;  // + i XPITCH (idle lanes: the dump slot)
    const int x_dst_step = xpos_ok ? XPITCH : 0;

    f32x16 acc[TAPS];
    wg_zero(acc);

    float gg[NGL], xg[NXL];
    bool g_ok = false, x_ok = false;          // the tile being staged: this thread's pixel / plane position is inside the image
    const float* g_ptr = p.g;                 // ... and the address of its element in channel 0 of the block
    const float* x_ptr = p.x;

    // tile -> pointers and validity of this thread's elements (elements outside the image read the tensor's first float)
    auto aim = [&](int tile) {
        const WgTile o = wg_tile_origin<TW, 4>(p, tile);
        const int b = o.b, yy = o.y0 + gpy, xx = o.x0 + gpx;
        const bool live = tile < p.n_tiles;
        g_ok = live && yy < p.H && xx < p.W;
        g_ptr = p.g + (g_ok ? (size_t)b * p.Cy * HW + (size_t)yy * p.W + xx : 0);
        const int uy = o.y0 + xr - 1, ux = o.x0 + xc - 1;
        x_ok = live && xpos_ok && uy >= 0 && uy < p.Hs && ux >= 0 && ux < p.Ws;
        x_ptr = p.x + (x_ok ? ((size_t)b * p.Cx + cx0 + ci0) * src_plane + (size_t)uy * p.Ws + ux : 0);
    };
    // staging pieces (j static): 0..15 the gradient element j, 16..47 the input channel j - 16
    auto load_piece = [&](auto j_) {
        constexpr int j = decltype(j_)::value;
        if constexpr (j < NGL) {
            const int c = min(co0 + gco + 4 * j, co_end - 1);      // rows past the group's last channel: clamped (see the store)
            gg[j] = g_ptr[g_ok ? (size_t)c * HW : 0];
        } else {
            const int c = min(cbw + (j - NGL), nci - 1);
            xg[j - NGL] = x_ptr[x_ok ? (size_t)c * src_plane : 0];
        }
    };
    auto store_piece = [&](float* buf, auto j_) {
        constexpr int j = decltype(j_)::value;
        if constexpr (j < NGL) {
            // only the PIXEL axis (the contraction) needs zeros; rows of channels past the block's last one hold the
            // clamped row's values and feed accumulator rows / columns the epilogue never writes (a uniform test here
            // would also split the loop body into branches)
            buf[g_dst + 4 * j * GPITCH] = g_ok ? gg[j] : 0.f;
        } else {
            buf[x_dst + (j - NGL) * x_dst_step] = x_ok ? xg[j - NGL] : 0.f;
        }
    };

    wg_stage_first<NGL + NXL, NGL + NXL>(p, smem, aim, load_piece, store_piece);
    int tile = blockIdx.z;
    int cur = 0;

    // one tile's 32 k-steps out of buffer `cur`; the next tile is staged into the other buffer on the way: three pieces per k-step,
    // one staging access behind every third MFMA
    auto run_tile = [&]() {
        const float* cbuf = smem + cur * BUF;
        float* nbuf = smem + (cur ^ 1) * BUF;
        wg_run_tile<SH, 1>(wg_grad_row<SH>(cbuf, wco * 32 + l32, half), wg_input_row<SH, 1>(cbuf, wci * 32 + l32, half), acc,
            [&](auto s_) {
                constexpr int st = decltype(s_)::value;
                if constexpr (st < WG_HS) wg_static_for<PPS * st, PPS * st + PPS>([&](auto j_) { load_piece(j_); });
                else wg_static_for<PPS * (st - WG_HS), PPS * (st - WG_HS) + PPS>([&](auto j_) { store_piece(nbuf, j_); });
            },
            [&](auto s_) {
                constexpr int st = decltype(s_)::value;
                wg_sched_frag_reads<st>();
#pragma unroll
                for (int k = 0; k < PPS; ++k) {
                    __builtin_amdgcn_sched_group_barrier(0x8, WG_TAPS / PPS, 0);
                    __builtin_amdgcn_sched_group_barrier(st < WG_HS ? 0x20 : 0x200, 1, 0);
                }
            });
    };

    // the loop of wg_persistent_tiles (one body, see there), written out: through the helper this kernel's tile loop is scheduled
    // differently
    for (; tile < p.n_tiles; tile += gridDim.z) {
        aim(tile + (int)gridDim.z);
        run_tile();
        __syncthreads();                      // every wave is done with `cur`, and the other buffer is complete
        cur ^= 1;
    }

    // ---- partial block -> slab [slab][co][tap][ci] (ci contiguous: 128-B stores per half wave) ----
    wg_store_slab9(p, acc, co0 + wco * 32, co_end, ci0 + wci * 32 + l32, half);
}

// ---- 3x3 stride-1 weight gradient of a conv that reads the BILINEAR x2 UPSAMPLING of x (styleganv1.py:624-625) ---------
// dW[co][ci][tap] = sum g[b,co,y,x] * up(x)[b,ci,y+ky-1,x+kx-1] without up(x) ever existing in HBM (round 1 materialised it:
// 268 MB written and read back at [8,128,256,256]).  Same block, tile, LDS images and arithmetic order as
// wgrad3x3_wide_kernel<1,1>; what differs is where the 18 x 6 input plane comes from: the tile's low-resolution SOURCE patch
// (4 x 10 pixels per channel, 2.7x fewer bytes than the plane) is loaded with 16-byte row loads two tiles ahead into a small
// fp32 LDS buffer, and the plane of the NEXT tile is interpolated LDS -> LDS while this tile's MFMAs run -- one element per
// thread and k-step, its tap offsets and weights wave-uniform scalars (a wave owns a quarter of the plane's positions, a lane
// one channel).  An earlier attempt formed the four bilinear taps with global gathers inside the staging and lost 2x to the
// materialised form: those 4 loads per element could not be prefetched; LDS reads need no prefetch.

// MODE = WG_BATCH_SCALE: the StyleGAN2 variant's x2 layers -- the upsampling is upfirdn2d(up = 2, [1,3,3,1]), i.e. the SAME parity
// taps (.25 / .75) over a ZERO-bordered source (the bilinear form replicates the edge), the source is x * s[b,ci] and the
// gradient g * d'[b,co]: all three differences live in the staging (zeros instead of clamped loads, two multiplies).
template <int MODE>
__global__ __launch_bounds__(256) void wgrad3x3_up_kernel(const WgradArgs p) {
    constexpr bool BSC = MODE == WG_BATCH_SCALE;
    using SH = WideShapeT<16>;
    constexpr int TAPS = 9, CO_T = 64, CI_T = 64, PW = SH::PW, PLANE = SH::PLANE, GPITCH = SH::GPITCH, XPITCH = SH::XPITCH, BUF = SH::BUF;
    constexpr int NG4 = 4, STEPS = 32, HS = 16, EPT = CI_T * PLANE / 256;       // 27 plane elements per thread
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const sbuf = smem + 2 * BUF;                  // two source-patch buffers behind the two tile buffers

    const WgBlock bk = wg_block<CO_T, CI_T>(p);
    const int tid = bk.tid, lane = bk.lane, wave = bk.wave, half = bk.half, l32 = bk.l32, wco = wave & 1, wci = wave >> 1;
    const int co0 = bk.co0, co_end = bk.co_end, cx0 = bk.cx0, ci0 = bk.ci0, nci = bk.nci;

    // ---- staging roles ----
    const int gk = tid & 3, grow = (tid >> 2) & 3;
    int g_off[NG4], g_ch[NG4];
    float g_sc[NG4];
#pragma unroll
    for (int i = 0; i < NG4; ++i) {
        g_ch[i] = min(co0 + (tid >> 4) + 16 * i, co_end - 1);
        g_off[i] = (g_ch[i] * p.H + grow) * p.W + 4 * gk;
        g_sc[i] = 1.f;
    }
    const int g_dst = (tid >> 4) * GPITCH + grow * 16 + 4 * gk;
    // source patch: piece i in {0, 1} = source row rh + 2 i of channel sc: float4 sk (columns x0/2 + 4 sk ..) and the halo column
    // x0/2 - 1 (sk = 0) / x0/2 + 8 (sk = 1)
    const int sk = tid & 1, sc = (tid >> 1) & 63, rh = tid >> 7;
    const int s_ch = cx0 + ci0 + min(sc, nci - 1);
    const int s_chan = s_ch * p.Hs;
    const int s_dst4 = sc * US_PITCH + rh * US_PW + 1 + 4 * sk;      // + 2 i US_PW + j
    const int s_dsth = sc * US_PITCH + rh * US_PW + (sk ? 9 : 0);    // + 2 i US_PW

    f32x16 acc[TAPS];
    wg_zero(acc);

    // per-tile state: (g) the gradient tile being staged; (s) the source patch being staged; (i) the tile being interpolated
    f32x4 gq[NG4], sq[2];
    float sh[2];
    const float* gbase = p.g;
    const float* sbase = p.x;
    bool g_ok = false;
    int s_y0 = 0, i_y0 = 0, i_x0 = 0;
    auto aim_g = [&](int tile) {
        const WgTile o = wg_tile_origin<16, 4>(p, tile);
        const int b = o.b, y0 = o.y0, x0 = o.x0;
        gbase = p.g + ((size_t)b * p.Cy * p.H + y0) * p.W + x0;
        g_ok = tile < p.n_tiles && y0 + grow < p.H && x0 + 4 * gk < p.W;
        if constexpr (BSC) {
            const int bb = tile < p.n_tiles ? b : 0;
#pragma unroll
            for (int i = 0; i < NG4; ++i) g_sc[i] = p.g_scale[(size_t)bb * p.Cy + g_ch[i]];
        }
    };
    // The source patch is REPLICATE-padded (rows / columns outside the image take the nearest edge pixel: loads with clamped
    // coordinates): torch's bilinear clamps its second tap at the border, which is the plain parity weights (.75, .25) applied
    // to a replicated neighbour -- so every plane element is interpolated with position-independent weights and no branch; what
    // remains of the border is the conv's ZERO padding of the x2 image, a per-tile row / column mask.
    int s_x0 = 0;
    bool s4_out = false;
    float s_sc = 1.f;                                                 // BSC: s[b, channel] of the patch being staged
    auto aim_s = [&](int tile) {
        const WgTile o = wg_tile_origin<16, 4>(p, tile);
        const int b = o.b, y0 = o.y0, x0 = o.x0;
        s_y0 = (y0 >> 1) - 1;                                         // first source row of the patch (may be -1)
        s_x0 = x0 >> 1;
        sbase = p.x + ((size_t)b * p.Cx * p.Hs) * p.Ws;
        s4_out = s_x0 + 4 * sk >= p.Ws;                                // this thread's vector lies right of the image: replicate
        if constexpr (BSC) s_sc = p.in_scale[(size_t)b * p.Cx + s_ch];  // (aim_s is only ever called with a live tile)
    };
    unsigned i_rows = 0, i_cols = 0;                                  // plane rows / columns inside the x2 image (bit r / bit c)
    auto aim_i = [&](int tile) {
        const WgTile o = wg_tile_origin<16, 4>(p, tile);
        i_y0 = o.y0; i_x0 = o.x0;
        i_rows = 0; i_cols = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r) i_rows |= ((unsigned)(i_y0 - 1 + r) < (unsigned)p.H ? 1u : 0u) << r;
#pragma unroll
        for (int c = 0; c < PW; ++c) i_cols |= ((unsigned)(i_x0 - 1 + c) < (unsigned)p.W ? 1u : 0u) << c;
    };
    auto s_row = [&](int i) { return min(max(s_y0 + rh + 2 * i, 0), p.Hs - 1); };
    auto load_g = [&](auto j_) { constexpr int j = decltype(j_)::value; gq[j] = *reinterpret_cast<const f32x4*>(g_ok ? gbase + g_off[j] : p.g); };
    auto store_g = [&](float* buf, auto s_) {
        constexpr int s = decltype(s_)::value, i = s / 4, j = s % 4;
        buf[g_dst + 16 * i * GPITCH + j] = g_ok ? (BSC ? gq[i][j] * g_sc[i] : gq[i][j]) : 0.f;
    };
    auto load_s = [&](auto j_) {              // j: 0, 1 = float4 of piece j; 2, 3 = halo of piece j - 2
        constexpr int j = decltype(j_)::value, i = j & 1;
        const float* row = sbase + (size_t)(s_chan + s_row(i)) * p.Ws;
        if constexpr (j < 2) sq[i] = *reinterpret_cast<const f32x4*>(row + min(s_x0 + 4 * sk, p.Ws - 4));     // Ws % 4 == 0
        else sh[i] = row[min(max(s_x0 + (sk ? 8 : -1), 0), p.Ws - 1)];
    };
    auto store_s = [&](float* sb, auto s_) {  // s: 0..7 = element s % 4 of float4 piece s / 4; 8, 9 = halo of piece s - 8
        constexpr int s = decltype(s_)::value;
        if constexpr (s < 8) {
            constexpr int i = s / 4, j = s % 4;
            if constexpr (BSC) {     // zero border: a source row / vector outside the image contributes nothing
                const bool in = (unsigned)(s_y0 + rh + 2 * i) < (unsigned)p.Hs && !s4_out;
                sb[s_dst4 + 2 * i * US_PW + j] = in ? sq[i][j] * s_sc : 0.f;
            } else {
                sb[s_dst4 + 2 * i * US_PW + j] = s4_out ? sq[i][3] : sq[i][j];     // (the clamped load fetched the image's last vector)
            }
        } else {
            constexpr int i = s - 8;
            if constexpr (BSC) {
                const bool in = (unsigned)(s_y0 + rh + 2 * i) < (unsigned)p.Hs && (unsigned)(s_x0 + (sk ? 8 : -1)) < (unsigned)p.Ws;
                sb[s_dsth + 2 * i * US_PW] = in ? sh[i] * s_sc : 0.f;
            } else {
                sb[s_dsth + 2 * i * US_PW] = sh[i];
            }
        }
    };
    // plane element e = wave * 27 + i of channel `lane` (a wave owns a quarter of the 108 positions): everything but the
    // channel is wave-uniform, so the tap offsets and weights live in scalar registers
    const float* const s_lane_base = sbuf + lane * US_PITCH;          // this lane's channel in source buffer 0
    // an element's four source taps are READ one k-step before they are combined and written (as the MFMA fragments are): with
    // read, combine and write in one step every wave waited ~200 cycles on its own LDS reads 27 times a tile
    float iq[4];
    auto interp_read = [&](int sbo, int i) {                           // sbo: float offset of the source buffer (0 / US_FLOATS)
        const int e = wave * EPT + i;                                  // uniform
        const int r = (e * 3641) >> 16, c = e - r * PW;                 // e / 18 for e < 108
        // x2 pixel (y0 - 1 + r, x0 - 1 + c), y0 and x0 even: first tap at patch (r >> 1, c >> 1)
        const float* q = s_lane_base + sbo + (r >> 1) * US_PW + (c >> 1);
        iq[0] = q[0]; iq[1] = q[1]; iq[2] = q[US_PW]; iq[3] = q[US_PW + 1];
    };
    auto interp_write = [&](float* buf, int i) {
        const int e = wave * EPT + i;
        const int r = (e * 3641) >> 16, c = e - r * PW;
        const float ly1 = (r & 1) ? 0.75f : 0.25f, lx1 = (c & 1) ? 0.75f : 0.25f;    // second-tap weight .25 on even r / c
        const float t = (1.f - ly1) * ((1.f - lx1) * iq[0] + lx1 * iq[1]) + ly1 * ((1.f - lx1) * iq[2] + lx1 * iq[3]);
        const bool inside = ((i_rows >> r) & (i_cols >> c) & 1u) != 0;  // uniform
        buf[CO_T * GPITCH + lane * XPITCH + e] = inside ? t : 0.f;
    };
    auto interp = [&](float* buf, int sbo, int i) { interp_read(sbo, i); interp_write(buf, i); };
    const int stride = (int)gridDim.z;
    int tile = blockIdx.z;
    int cur = 0, par = 0;                      // tile buffer in use; source buffer holding the patch of tile `tile + stride`... see below
    // ---- prologue: S(k = 0) -> sbuf[0], S(k = 1) -> sbuf[1], G(0) -> buf 0; barrier; plane(0) by interpolation; barrier ----
    if (tile < p.n_tiles) {
        aim_s(tile);
        wg_static_for<0, 4>([&](auto j_) { load_s(j_); });
        wg_static_for<0, 10>([&](auto s_) { store_s(sbuf, s_); });
        if (tile + stride < p.n_tiles) {
            aim_s(tile + stride);
            wg_static_for<0, 4>([&](auto j_) { load_s(j_); });
            wg_static_for<0, 10>([&](auto s_) { store_s(sbuf + US_FLOATS, s_); });
        }
        aim_g(tile);
        wg_static_for<0, NG4>([&](auto j_) { load_g(j_); });
        wg_static_for<0, 4 * NG4>([&](auto s_) { store_g(smem, s_); });
        __syncthreads();
        aim_i(tile);
        for (int i = 0; i < EPT; ++i) interp(smem, 0, i);
    }
    __syncthreads();

    // iteration k computes tile k out of buf[cur]; meanwhile G(k+1) is loaded / stored into the other tile buffer, the plane of
    // tile k+1 is interpolated into it from sbuf[(k+1) & 1], and the source patch of tile k+2 is loaded and stored into
    // sbuf[k & 1] (whose previous content, the patch of tile k, was last read during iteration k - 1).
    // Fragment reads, tile loop and epilogue are those of wgrad_tile3x3.hpp WRITTEN OUT: wg_frag3x3, wg_run_tile /
    // wg_persistent_tiles and wg_store_slab9 each moved instructions inside this kernel's tile loop.
    auto run_tile = [&]() {
        const float* cbuf = smem + cur * BUF;
        float* nbuf = smem + (cur ^ 1) * BUF;
        const int s_next = (par ^ 1) * US_FLOATS;                      // patch of tile k+1 (float offset behind sbuf)
        float* s_fill = sbuf + par * US_FLOATS;                       // patch of tile k+2 goes here
        const volatile wg_lds_f32* ga = (const volatile wg_lds_f32*)(cbuf + (wco * 32 + l32) * GPITCH + half);
        const volatile wg_lds_f32* xb = (const volatile wg_lds_f32*)(cbuf + CO_T * GPITCH + (wci * 32 + l32) * XPITCH + half);
        float fa[2], fb[2][TAPS];
#define SPK_WU_FRAG(st_, slot_)                                                                               \
    {                                                                                                         \
        constexpr int px_ = (2 * (st_)) & 15, py_ = (2 * (st_)) >> 4;                                         \
        fa[slot_] = ga[2 * (st_)];                                                                            \
        _Pragma("unroll") for (int t = 0; t < TAPS; ++t) fb[slot_][t] = xb[(py_ + t / 3) * PW + px_ + t % 3];  \
    }
        SPK_WU_FRAG(0, 0);
        wg_static_for<0, STEPS>([&](auto s_) {
            constexpr int st = decltype(s_)::value;
            if constexpr (st == HS) __builtin_amdgcn_sched_barrier(0);               // see wg_run_tile
            if constexpr (st + 1 < STEPS) SPK_WU_FRAG(st + 1, (st + 1) & 1);
            if constexpr (st < NG4) load_g(std::integral_constant<int, st>{});
            if constexpr (st >= NG4 && st < NG4 + 4) load_s(std::integral_constant<int, st - NG4>{});
            if constexpr (st >= 1 && st <= EPT) interp_write(nbuf, st - 1);
            if constexpr (st < EPT) interp_read(s_next, st);
            if constexpr (st >= HS) store_g(nbuf, std::integral_constant<int, st - HS>{});
            if constexpr (st >= HS && st < HS + 10) store_s(s_fill, std::integral_constant<int, st - HS>{});
#pragma unroll
            for (int t = 0; t < TAPS; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[st & 1], fb[st & 1][t], acc[t], 0, 0, 0);
            // order: the LDS reads (next step's fragments, the next element's taps) first, then the MFMAs with the rest of the
            // step's staging (loads, LDS stores, the interpolation arithmetic) spread between them in three parts
            if constexpr (st + 1 < STEPS) __builtin_amdgcn_sched_group_barrier(0x100, TAPS + 1 + (st < EPT ? 4 : 0), 0);
            __builtin_amdgcn_sched_group_barrier(0x8, 3, 0);
            __builtin_amdgcn_sched_group_barrier(0x2 | 0x4 | 0x20 | 0x200, 8, 0);
            __builtin_amdgcn_sched_group_barrier(0x8, 3, 0);
            __builtin_amdgcn_sched_group_barrier(0x2 | 0x4 | 0x20 | 0x200, 8, 0);
            __builtin_amdgcn_sched_group_barrier(0x8, 3, 0);
        });
#undef SPK_WU_FRAG
    };

    for (; tile < p.n_tiles; tile += stride) {
        // one loop body (see wg_persistent_tiles): past the last tile the gradient pieces are masked off, the patch of the
        // last tile is fetched again and the idle buffers are filled with values nobody reads
        aim_g(tile + stride);
        aim_i(tile + stride);
        aim_s(min(tile + 2 * stride, p.n_tiles - 1));
        run_tile();
        __syncthreads();
        cur ^= 1;
        par ^= 1;
    }

    // ---- partial block -> slab [slab][co][tap][ci] ----
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

int spkwg::launch_pipe_up(const WgradPlan& p, hipStream_t stream) {
    if (p.form == SPK_WGRAD_PIPE) return launch_planned(reinterpret_cast<const void*>(&wgrad3x3_pipe_kernel), "wgrad3x3_pipe_kernel", p, stream);
    const void* k = p.mode == WG_BATCH_SCALE ? reinterpret_cast<const void*>(&wgrad3x3_up_kernel<WG_BATCH_SCALE>)
                                             : reinterpret_cast<const void*>(&wgrad3x3_up_kernel<WG_PLAIN>);
    return launch_planned(k, "wgrad3x3_up_kernel", p, stream);
}
