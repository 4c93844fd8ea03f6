// Weight gradient of the 2-D convolution on the gfx950 f32 MFMA pipe:
//     dW[co][ci][ky][kx] = sum_{b,y,x} g[b,co,y,x] * xin[b,ci,y*S+ky-P,x*S+kx-P]
// as the GEMM  D[co][(tap,ci)] = sum_pix G[co][pix] * X[ci][pix (+) tap]  with the pixel axis as K.
//   A fragment (v_mfma_f32_32x32x2_f32): lane l holds G[co = l&31][pix = l>>5]   (LDS row pitch odd)
//   B fragment, one per tap:             lane l holds X[ci = l&31][pix (+) tap]   (LDS row pitch odd)
//   D: col = lane&31 = ci, row = output channel; one 32x32 accumulator tile PER TAP per wave, so
//   the A fragment is read once per k-step and reused by all taps.
// A workgroup owns a 64co x CI_T block of dW and walks a strided share of the pixel tiles
// (64 pixels each, with halo, xin formed exactly as the forward pass forms it: plain, bilinear x2
// upsampled, or BatchNorm-affine+ReLU).  Partial blocks go to a slab per (pixel split, wave pixel
// half) in a ci-contiguous layout (coalesced stores); wgrad_reduce_kernel sums the slabs in a fixed
// order (bitwise reproducible, no float atomics) and transposes to [Cout][Cin][kh][kw].
//
// replaces: the weight-gradient half of F.conv2d's backward for every conv on the path
// (styleganv1.py:625,630 conv1/conv2; the torchvision trunk convs of model.py:60-62).
//
// This unit: the slab reducers, the planner (descriptor -> WgradPlan, every requirement and form decision, no HIP call) and the
// C entry points.  The kernels: one family per wgrad_inst_*.hip, launched from the plan.
#include "wgrad_mfma_f32.hpp"

#include <algorithm>
#include <cstdlib>

using namespace spkwg;

namespace {

// dW[co][ci][tap] (+)= scale * sum_slab slabs[slab][co][tap][ci]   (fixed order)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ dw,
                                                          int n_slabs, int Cout_all, int Cin, int taps, float scale,
                                                          int accumulate, int fold) {
    // fold > 1: output channel co also takes the slabs' channels co + Cout, co + 2 Cout, ... (the same conv on other images)
    const int Cout = Cout_all / fold;
    const size_t total = (size_t)Cout * Cin * taps, slab_stride = (size_t)Cout_all * Cin * taps;
    // walk the slabs in THEIR order ([co][tap][ci]: coalesced reads of n_slabs x total floats) and scatter the
    // (n_slabs times smaller) result into [co][ci][tap]
    for (size_t src = (size_t)blockIdx.x * blockDim.x + threadIdx.x; src < total; src += (size_t)gridDim.x * blockDim.x) {
        const int ci = (int)(src % Cin);
        const int tap = (int)((src / Cin) % taps);
        const int co = (int)(src / ((size_t)Cin * taps));
        // four interleaved partial sums (slab s goes to sum s % 4): still one fixed order, but four loads in flight
        float v = 0.f;
        for (int f = 0; f < fold; ++f) {
            const float* sl = slabs + (size_t)f * total + src;
            float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
            int s = 0;
            for (; s + 4 <= n_slabs; s += 4) {
                const float a0 = sl[(size_t)s * slab_stride], a1 = sl[(size_t)(s + 1) * slab_stride];
                const float a2 = sl[(size_t)(s + 2) * slab_stride], a3 = sl[(size_t)(s + 3) * slab_stride];
                v0 += a0; v1 += a1; v2 += a2; v3 += a3;
            }
            for (; s < n_slabs; ++s) v0 += sl[(size_t)s * slab_stride];
            v += (v0 + v1) + (v2 + v3);
        }
        v *= scale;
        const size_t idx = ((size_t)co * Cin + ci) * taps + tap;
        dw[idx] = accumulate ? dw[idx] + v : v;
    }
}

// The same sum, four input channels per thread (Cin % 4 == 0): 16-byte loads and EIGHT slabs in flight per thread.  The
// dword form above waits for every round of four loads before it issues the next -- with 16-42 slabs that is 4-10 memory
// latencies in a row, 2.3 TB/s on slabs that mostly still sit in the memory-side cache; this one runs at 13 -> ~7 us per
// trunk / decoder layer, ~65 (G step) to ~100 (D step) times per training step.  Same summation order as the dword form.
__global__ __launch_bounds__(256) void wgrad_reduce_vec_kernel(const float* __restrict__ slabs, float* __restrict__ dw,
                                                              int n_slabs, int Cout_all, int Cin, int taps, float scale,
                                                              int accumulate, int fold) {
    const int Cout = Cout_all / fold;
    const size_t total = (size_t)Cout * Cin * taps, slab_stride = (size_t)Cout_all * Cin * taps;
    const int cin4 = Cin >> 2;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total / 4; q += (size_t)gridDim.x * blockDim.x) {
        const int ci = (int)(q % cin4) * 4;
        const int tap = (int)((q / cin4) % taps);
        const int co = (int)(q / ((size_t)cin4 * taps));
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        for (int f = 0; f < fold; ++f) {
            const float* sl = slabs + (size_t)f * total + 4 * q;
            f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0, v2 = v0, v3 = v0;
            int s = 0;
            for (; s + 8 <= n_slabs; s += 8) {
                f32x4 a[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] = *reinterpret_cast<const f32x4*>(sl + (size_t)(s + j) * slab_stride);
                v0 += a[0]; v1 += a[1]; v2 += a[2]; v3 += a[3];
                v0 += a[4]; v1 += a[5]; v2 += a[6]; v3 += a[7];
            }
            if (s + 4 <= n_slabs) {
                f32x4 a[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = *reinterpret_cast<const f32x4*>(sl + (size_t)(s + j) * slab_stride);
                v0 += a[0]; v1 += a[1]; v2 += a[2]; v3 += a[3];
                s += 4;
            }
            for (; s < n_slabs; ++s) v0 += *reinterpret_cast<const f32x4*>(sl + (size_t)s * slab_stride);
            v += (v0 + v1) + (v2 + v3);
        }
        v *= scale;
        const size_t idx = ((size_t)co * Cin + ci) * taps + tap;
        if (taps == 1) {
            f32x4* o = reinterpret_cast<f32x4*>(dw + idx);
            *o = accumulate ? *o + v : v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) dw[idx + (size_t)j * taps] = accumulate ? dw[idx + (size_t)j * taps] + v[j] : v[j];
        }
    }
}

// MANY slabs of a SMALL gradient (the one-round grids of the Winograd weight gradient: 256 slabs of a 64 x 64 x 9 block, 37.7 MB for
// 36 workgroups of the kernel above -- 256 dependent rounds each): 16 threads share an output element group, thread (e, l) sums the
// slabs l, l + 16, ... (all of them in flight), the 16 partial sums meet in LDS and are added in lane order -- a fixed order, so the
// result stays bitwise reproducible (it is NOT the order of the kernels above: a layer always takes the same one of the two).
constexpr int RD_SL = 16, RD_EL = 16;
__global__ __launch_bounds__(256) void wgrad_reduce_deep_kernel(const float* __restrict__ slabs, float* __restrict__ dw, int n_slabs,
                                                               int Cout_all, int Cin, int taps, float scale, int accumulate, int fold) {
    __shared__ f32x4 part[RD_SL][RD_EL];
    const int Cout = Cout_all / fold;
    const size_t total = (size_t)Cout * Cin * taps, slab_stride = (size_t)Cout_all * Cin * taps;
    const int cin4 = Cin >> 2;
    const int e = threadIdx.x & (RD_EL - 1), l = threadIdx.x / RD_EL;
    for (size_t q0 = (size_t)blockIdx.x * RD_EL; q0 < total / 4; q0 += (size_t)gridDim.x * RD_EL) {      // (uniform trip count: barriers inside)
        const size_t q = q0 + e;
        const bool live = q < total / 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (live)
            for (int f = 0; f < fold; ++f) {
                const float* sl = slabs + (size_t)f * total + 4 * q;
                f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
                int s_ = l;
                for (; s_ + 7 * RD_SL < n_slabs; s_ += 8 * RD_SL) {
                    f32x4 a[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) a[j] = *reinterpret_cast<const f32x4*>(sl + (size_t)(s_ + j * RD_SL) * slab_stride);
#pragma unroll
                    for (int j = 0; j < 8; j += 2) { v0 += a[j]; v1 += a[j + 1]; }
                }
                for (; s_ < n_slabs; s_ += RD_SL) v0 += *reinterpret_cast<const f32x4*>(sl + (size_t)s_ * slab_stride);
                v += v0 + v1;
            }
        part[l][e] = v;
        __syncthreads();
        if (l == 0 && live) {
            f32x4 t = part[0][e];
#pragma unroll
            for (int j = 1; j < RD_SL; ++j) t += part[j][e];
            t *= scale;
            const int ci = (int)(q % cin4) * 4;
            const int tap = (int)((q / cin4) % taps);
            const int co = (int)(q / ((size_t)cin4 * taps));
            const size_t idx = ((size_t)co * Cin + ci) * taps + tap;
            if (taps == 1) {
                f32x4* o = reinterpret_cast<f32x4*>(dw + idx);
                *o = accumulate ? *o + t : t;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) dw[idx + (size_t)j * taps] = accumulate ? dw[idx + (size_t)j * taps] + t[j] : t[j];
            }
        }
        __syncthreads();
    }
}

// slabs -> dW on `stream`, after the kernel that wrote them
int launch_wgrad_reduce(hipStream_t stream, const float* slabs, float* dw, int n_slabs, int Cout_all, int Cin, int taps, float scale,
                        int accumulate, int fold) {
    const size_t slab_floats = (size_t)Cout_all * Cin * taps;
    const int reducer = pick_reducer(slabs, dw, n_slabs, slab_floats, Cin, fold);
    if (reducer == 2) {
        const unsigned blocks = (unsigned)std::min<size_t>((slab_floats / fold / 4 + RD_EL - 1) / RD_EL, 4096);
        hipLaunchKernelGGL(wgrad_reduce_deep_kernel, dim3(std::max(blocks, 1u)), dim3(256), 0, stream, slabs, dw, n_slabs, Cout_all, Cin,
                           taps, scale, accumulate, fold);
    } else if (reducer == 1) {
        const unsigned blocks = (unsigned)std::min<size_t>((slab_floats / fold / 4 + 255) / 256, 4096);
        hipLaunchKernelGGL(wgrad_reduce_vec_kernel, dim3(std::max(blocks, 1u)), dim3(256), 0, stream, slabs, dw, n_slabs, Cout_all, Cin,
                           taps, scale, accumulate, fold);
    } else {
        const unsigned blocks = (unsigned)std::min<size_t>((slab_floats + 255) / 256, 2048);
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, stream, slabs, dw, n_slabs, Cout_all, Cin, taps, scale,
                           accumulate, fold);
    }
    return spk::check_launch("wgrad_reduce_kernel");
}

// ---- the planner: descriptor -> WgradPlan, no HIP call ------------------------------------------------------------------------------
// The on/off switches of the forms (DESIGN's A/B figures were taken with them), read once.
struct Switches { bool wide, pipe, fixed, s2, stem, dma; };
bool env_on(const char* name) { const char* e = getenv(name); return !e || atoi(e) != 0; }
const Switches& switches() {
    static const Switches s = {env_on("SPK_WGRAD_WIDE"), env_on("SPK_WGRAD_PIPE"), env_on("SPK_WGRAD_FIXED"),
                               env_on("SPK_WGRAD_S2"),   env_on("SPK_WGRAD_STEM"), env_on("SPK_WGRAD1X1_DMA")};
    return s;
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
int groups_of(const spk_wgrad_desc* d) { return d->groups > 1 ? d->groups : 1; }

// pixel splits: the wanted count, or as many as bring `blocks` channel blocks to `target` workgroups; never more than tiles
int pick_splits(int want, int target, int blocks, int n_tiles) {
    const int sp = want > 0 ? want : std::max(1, target / blocks);
    return std::max(1, std::min(sp, n_tiles));
}

// The geometry of each form from the shape alone (Cout_all = groups * Cout): the tile, grid, LDS and slab fields of a plan.
// plan_wgrad completes it from the descriptor; spk_conv2d_wgrad_workspace_bytes asks for ws_slabs.
template <int KH, int KW, int S>
WgradPlan tap_geom(int B, int Cin, int Cout_all, int H, int W, int want_splits) {
    using SH = WShape<KH, KW, S>;
    WgradPlan g{};
    g.TW = std::min(32, spk::pow2_ceil(W));
    if (SH::CS > 1 && H >= 4) g.TW = std::min(g.TW, 16);     // 16x4 tiles: 108 staged positions (<= 128) instead of 136
    g.TH = std::min(SH::PIX_T / g.TW, spk::pow2_ceil(H));
    g.TB = SH::PIX_T / (g.TW * g.TH);
    // keep the staged input tile within LDS: shrink the image group first, then the rows
    auto lds = [&]() {
        const size_t plane = (size_t)((g.TH - 1) * S + KH) * ((g.TW - 1) * S + KW);
        return (SH::CO_T * (SH::PIX_T + 1) + SH::CI_T * ((g.TB * plane) | 1)) * sizeof(float);
    };
    auto plane_elems = [&]() { return g.TB * ((g.TH - 1) * S + KH) * ((g.TW - 1) * S + KW); };
    while ((lds() > 100 * 1024 || plane_elems() > SH::NPT * SH::KX) && g.TB > 1) g.TB >>= 1;   // idle pixel groups
    while (plane_elems() > SH::NPT * SH::KX && g.TH > 1) g.TH >>= 1;
    g.lds_bytes = lds();
    g.args.tiles_x = spk::ceil_div(W, g.TW);
    g.args.tiles_y = spk::ceil_div(H, g.TH);
    g.n_tiles = g.args.tiles_x * g.args.tiles_y * spk::ceil_div(B, g.TB);
    g.grid = dim3((unsigned)spk::ceil_div(Cout_all, SH::CO_T), (unsigned)(spk::ceil_div(Cin, SH::CI_T) * (SH::ROWPASS ? KH : 1)));
    g.splits = pick_splits(want_splits, 512, (int)(g.grid.x * g.grid.y), g.n_tiles);     // 2 rounds of one workgroup per CU
    g.tiles_per_split = spk::ceil_div(g.n_tiles, g.splits);
    g.n_slabs = g.ws_slabs = g.splits * SH::WPX;
    g.grid.z = (unsigned)g.splits;
    return g;
}
WgradPlan tap_geom(int kh, int stride, int B, int Cin, int Cout_all, int H, int W, int want_splits) {
    if (kh == 1) return stride == 1 ? tap_geom<1, 1, 1>(B, Cin, Cout_all, H, W, want_splits) : tap_geom<1, 1, 2>(B, Cin, Cout_all, H, W, want_splits);
    if (kh == 3) return stride == 1 ? tap_geom<3, 3, 1>(B, Cin, Cout_all, H, W, want_splits) : tap_geom<3, 3, 2>(B, Cin, Cout_all, H, W, want_splits);
    return kh == 4 ? tap_geom<4, 4, 2>(B, Cin, Cout_all, H, W, want_splits) : tap_geom<7, 7, 2>(B, Cin, Cout_all, H, W, want_splits);
}

// the 3x3 forms on tw x (64 / tw) pixel tiles with co_t x ci_t blocks, one workgroup per CU: wide (and up) 64 x 64, s2 128 x 32
WgradPlan tile_geom(int tw, int co_t, int ci_t, size_t lds_bytes, int B, int Cin, int Cout_all, int H, int W, int want_splits) {
    WgradPlan g{};
    g.TW = tw; g.TH = 64 / tw; g.TB = 1;
    g.lds_bytes = lds_bytes;
    g.args.tiles_x = spk::ceil_div(W, g.TW);
    g.args.tiles_y = spk::ceil_div(H, g.TH);
    g.n_tiles = g.args.tiles_x * g.args.tiles_y * B;
    g.grid = dim3((unsigned)spk::ceil_div(Cout_all, co_t), (unsigned)spk::ceil_div(Cin, ci_t));
    g.splits = pick_splits(want_splits, 256, (int)(g.grid.x * g.grid.y), g.n_tiles);
    g.tiles_per_split = spk::ceil_div(g.n_tiles, g.splits);
    g.n_slabs = g.ws_slabs = g.splits;
    g.grid.z = (unsigned)g.splits;
    return g;
}
bool wide_shape(int H, int W) { return W >= 8 && W % 4 == 0 && H >= 4; }
WgradPlan wide_geom(int B, int Cin, int Cout_all, int H, int W, int want_splits) {
    return W >= 16 ? tile_geom(16, 64, 64, 2 * WideShapeT<16>::BUF * sizeof(float), B, Cin, Cout_all, H, W, want_splits)
                   : tile_geom(8, 64, 64, 2 * WideShapeT<8>::BUF * sizeof(float), B, Cin, Cout_all, H, W, want_splits);
}
// (the upsample-folded form: the wide form's 16 x 4 tile and split rule, two source-patch buffers behind the two tile buffers)
bool up_shape(int H, int W) { return W >= 16 && W % 8 == 0 && H >= 4 && H % 2 == 0; }
WgradPlan up_geom(int B, int Cin, int Cout_all, int H, int W, int want_splits) {
    return tile_geom(16, 64, 64, (2 * WideShapeT<16>::BUF + 2 * US_FLOATS) * sizeof(float), B, Cin, Cout_all, H, W, want_splits);
}
bool s2_shape(int H, int W) { return W >= 8 && W % 4 == 0 && H >= 2; }
WgradPlan s2_geom(int B, int Cin, int Cout_all, int H, int W, int want_splits) {
    return W >= 16 ? tile_geom(16, 128, 32, 2 * S2Shape<16>::BUF * sizeof(float), B, Cin, Cout_all, H, W, want_splits)
                   : tile_geom(8, 128, 32, 2 * S2Shape<8>::BUF * sizeof(float), B, Cin, Cout_all, H, W, want_splits);
}

// the 1x1 GEMM forms: (64 mt) co x (64 nt) ci blocks over 32-pixel k-tiles, at least 4 k-tiles per workgroup
bool g1_shape(int H, int W) { return ((long long)H * W) % G1_KT == 0 && W % 4 == 0; }
int g1_mt(int G, int Cout) { return (Cout % 128 == 0 || (G == 1 && Cout > 64)) ? 2 : 1; }
int g1_nt(int Cin) { return Cin > 64 ? 2 : 1; }
WgradPlan g1_geom(int mt, int nt, int B, int Cin, int Cout_all, int H, int W, int want_splits) {
    WgradPlan g{};
    g.MT = mt; g.NT = nt;
    g.lds_bytes = 2 * (size_t)(64 * mt + 64 * nt) * G1_PITCH * sizeof(float);       // (the LDS-DMA twin: G1_KT for G1_PITCH)
    g.n_tiles = (int)((long long)B * H * W / G1_KT);
    g.grid = dim3((unsigned)spk::ceil_div(Cout_all, 64 * mt), (unsigned)spk::ceil_div(Cin, 64 * nt));
    const int sp = pick_splits(want_splits, 512, (int)(g.grid.x * g.grid.y), std::max(1, g.n_tiles / 4));
    g.tiles_per_split = spk::ceil_div(g.n_tiles, sp);
    g.splits = spk::ceil_div(g.n_tiles, g.tiles_per_split);
    g.n_slabs = g.ws_slabs = g.splits;
    g.grid.z = (unsigned)g.splits;
    return g;
}

// the stem form: G groups of 3 -> 64 channels, 32 x 4 tiles, one slab per persistent workgroup
bool stem_shape(int Cin, int Cout_all, int W) { return Cin == 3 && Cout_all % 64 == 0 && W % 4 == 0; }
WgradPlan stem_geom(int B, int G, int H, int W, int want_splits) {
    WgradPlan g{};
    g.TW = SW_TW; g.TH = SW_TH; g.TB = 1;
    g.lds_bytes = SW_LDS_FL * sizeof(float);
    g.args.tiles_x = spk::ceil_div(W, SW_TW);
    g.args.tiles_y = spk::ceil_div(H, SW_TH);
    const long long tiles = (long long)B * g.args.tiles_x * g.args.tiles_y;
    g.n_tiles = (int)tiles;
    g.ws_slabs = want_splits > 0 ? std::min(want_splits, 512) : pick_splits(0, 512, G, (int)std::min(tiles, 512ll));
    g.n_slabs = g.splits = std::min(g.ws_slabs, g.n_tiles);
    g.tiles_per_split = spk::ceil_div(g.n_tiles, g.splits);
    g.grid = dim3((unsigned)g.splits, (unsigned)G);
    return g;
}

// which form takes a descriptor
bool planes_fit_31_bits(const spk_wgrad_desc* d) {      // an image's planes of g and of x are addressed with 32-bit offsets
    const int G = groups_of(d);
    return (long long)G * d->Cout * d->H * d->W < (1ll << 31) && ((long long)d->group_in_stride * (G - 1) + d->Cin) * d->Hin * d->Win < (1ll << 31);
}
bool wide_takes(const spk_wgrad_desc* d) {
    return switches().wide && d->kh == 3 && d->kw == 3 && d->stride == 1 && wide_shape(d->H, d->W) && aligned16(d->g) && aligned16(d->x) &&
           planes_fit_31_bits(d) && (groups_of(d) == 1 || d->Cout % 64 == 0);
}
// the upsample-folded form: x is the LOW-resolution tensor [B, Cin, H/2, W/2]
bool up_takes(const spk_wgrad_desc* d) {
    return d->kh == 3 && d->kw == 3 && d->stride == 1 && up_shape(d->H, d->W) && aligned16(d->g) && aligned16(d->x) && planes_fit_31_bits(d) &&
           (groups_of(d) == 1 || d->Cout % 64 == 0);
}
// the stride-2 form: 128co x 32ci blocks, 16x4 or 8x8 output-pixel tiles
bool s2_takes(const spk_wgrad_desc* d) {
    return switches().s2 && d->kh == 3 && d->kw == 3 && d->stride == 2 && s2_shape(d->H, d->W) && d->Hin == 2 * d->H && d->Win == 2 * d->W &&
           aligned16(d->g) && aligned16(d->x) && d->Cout >= 96 && (groups_of(d) == 1 || d->Cout % 128 == 0) && planes_fit_31_bits(d);
}
// whether the GEMM form takes this 1x1 problem (else the tap kernel does)
bool g1_takes(const spk_wgrad_desc* d) { return d->kh == 1 && g1_shape(d->H, d->W) && (groups_of(d) == 1 || d->Cout % 64 == 0); }
// whether its LDS-DMA twin takes a stride-1 problem of block shape (bm, bn)
bool dma_takes(const spk_wgrad_desc* d, int bm, int bn) {
    const long long HW = (long long)d->H * d->W;
    return switches().dma && d->stride == 1 && d->Cout % bm == 0 && d->Cin % bn == 0 && HW % G1_KT == 0 && HW * 8 * 4 < (1ll << 31) &&
           aligned16(d->g) && aligned16(d->x) && d->Hin == d->H && d->Win == d->W;
}
bool stem_takes(const spk_wgrad_desc* d) {
    const int G = groups_of(d);
    return switches().stem && d->kh == 7 && d->kw == 7 && d->stride == 2 && d->Cout == 64 && stem_shape(d->Cin, d->Cout, d->W) && aligned16(d->g) &&
           (d->flags & ~0u) == 0 && (long long)G * 64 * d->H * d->W < (1ll << 29) && (long long)3 * G * d->Hin * d->Win < (1ll << 29) &&
           (G == 1 || d->group_in_stride == 0 || d->group_in_stride >= 3);
}

// geometry -> plan: the workspace check, the kernel's arguments and the reduce (slabs [G Cout][taps][red_cin])
int complete_plan(const spk_wgrad_desc* d, int form, int mode, int red_cin, int taps, WgradPlan& p) {
    const int G = groups_of(d);
    p.form = form; p.mode = mode; p.kh = d->kh; p.kw = d->kw; p.stride = d->stride;
    p.slab_floats = (size_t)G * d->Cout * red_cin * taps;
    const size_t need = p.ws_slabs * p.slab_floats * sizeof(float);
    SPK_REQUIRE(d->workspace && (size_t)d->workspace_bytes >= need, "wgrad: needs a %zu-byte workspace (see spk_conv2d_wgrad_workspace_bytes)", need);
    WgradArgs& a = p.args;
    a.g = d->g; a.x = d->x; a.in_scale = d->in_scale; a.in_shift = d->in_shift; a.g_scale = d->g_scale; a.slabs = static_cast<float*>(d->workspace);
    a.B = d->B; a.Cin = d->Cin; a.Cout = d->Cout; a.H = d->H; a.W = d->W; a.Hs = d->Hin; a.Ws = d->Win;
    a.gin = G > 1 ? d->group_in_stride : d->Cin;
    a.Cx = a.gin * (G - 1) + d->Cin;
    a.Cy = G * d->Cout;
    a.lgTW = spk::ilog2(p.TW); a.lgTH = spk::ilog2(p.TH); a.lgTB = spk::ilog2(p.TB);
    a.n_tiles = p.n_tiles;
    p.fold = d->fold > 1 ? d->fold : 1; p.taps = taps; p.red_cout = G * d->Cout; p.red_cin = red_cin;
    p.scale = d->scale; p.accumulate = d->accumulate ? 1 : 0; p.dw = d->dw;
    p.reducer = pick_reducer(a.slabs, p.dw, p.n_slabs, p.slab_floats, red_cin, p.fold);
    return SPK_OK;
}

template <int KH, int KW, int S>
int plan_tap(const spk_wgrad_desc* d, int mode, WgradPlan& p) {
    using SH = WShape<KH, KW, S>;
    const int G = groups_of(d);
    SPK_REQUIRE(!SH::PACK || KW * d->Cin <= 32, "wgrad: the %dx%d kernel packs (kx, ci) into 32 lanes: Cin <= %d", KH, KW, 32 / KW);
    SPK_REQUIRE(G == 1 || d->Cout % SH::CO_T == 0, "wgrad: grouped launches need Cout (per group) to be a multiple of %d", SH::CO_T);
    p = tap_geom<KH, KW, S>(d->B, d->Cin, G * d->Cout, d->H, d->W, d->splits);
    SPK_REQUIRE(p.lds_bytes <= 160 * 1024, "wgrad: input tile does not fit LDS");
    // On the 16 x 4 x 1 tile a 3x3 stride-1 layer leaves the runtime geometry: BatchNorm-folded for the compile-time tile shape
    // (two workgroups per CU; measured, profiles/r01_k_wgrad_phases.txt: +8% on the trunk's layers, whose store phase carries
    // the affine; -4% on the decoder's plain layers), plain for the form whose staging is interleaved with the MFMAs
    const bool tile16x4 = KH == 3 && S == 1 && p.TW == 16 && p.TH == 4 && p.TB == 1;
    int form = SPK_WGRAD_TAP;
    if (tile16x4 && mode == WG_AFFINE_RELU && switches().fixed) form = SPK_WGRAD_TAP_FIXED;
    if (tile16x4 && mode == WG_PLAIN && switches().pipe) {
        form = SPK_WGRAD_PIPE;
        p.lds_bytes = 2 * WP_BUF * sizeof(float);
    }
    return complete_plan(d, form, mode, d->Cin, SH::TAPS, p);
}
int plan_tap(const spk_wgrad_desc* d, int mode, WgradPlan& p) {
    if (d->kh == 1) return d->stride == 1 ? plan_tap<1, 1, 1>(d, mode, p) : plan_tap<1, 1, 2>(d, mode, p);
    if (d->kh == 3) return d->stride == 1 ? plan_tap<3, 3, 1>(d, mode, p) : plan_tap<3, 3, 2>(d, mode, p);
    return d->kh == 4 ? plan_tap<4, 4, 2>(d, mode, p) : plan_tap<7, 7, 2>(d, mode, p);
}

int plan_wide(const spk_wgrad_desc* d, int mode, WgradPlan& p) {
    p = wide_geom(d->B, d->Cin, groups_of(d) * d->Cout, d->H, d->W, d->splits);
    return complete_plan(d, p.TW == 16 ? SPK_WGRAD_WIDE16 : SPK_WGRAD_WIDE8, mode, d->Cin, 9, p);
}
int plan_up(const spk_wgrad_desc* d, int mode, WgradPlan& p) {
    p = up_geom(d->B, d->Cin, groups_of(d) * d->Cout, d->H, d->W, d->splits);
    return complete_plan(d, SPK_WGRAD_UP, mode, d->Cin, 9, p);
}
int plan_s2(const spk_wgrad_desc* d, int mode, WgradPlan& p) {
    p = s2_geom(d->B, d->Cin, groups_of(d) * d->Cout, d->H, d->W, d->splits);
    return complete_plan(d, p.TW == 16 ? SPK_WGRAD_S2_16 : SPK_WGRAD_S2_8, mode, d->Cin, 9, p);
}
int plan_g1(const spk_wgrad_desc* d, int mode, WgradPlan& p) {
    const int G = groups_of(d), mt = g1_mt(G, d->Cout), nt = g1_nt(d->Cin);
    p = g1_geom(mt, nt, d->B, d->Cin, G * d->Cout, d->H, d->W, d->splits);
    const bool dma = dma_takes(d, 64 * mt, 64 * nt);
    if (dma) p.lds_bytes = 2 * (size_t)(64 * mt + 64 * nt) * G1_KT * sizeof(float);
    const int rc = complete_plan(d, dma ? SPK_WGRAD_GEMM1X1_DMA : SPK_WGRAD_GEMM1X1, mode, d->Cin, 1, p);
    if (rc != SPK_OK) return rc;
    SPK_REQUIRE((long long)p.args.Cy * d->H * d->W < (1ll << 31) && (long long)p.args.Cx * d->Hin * d->Win < (1ll << 31),
                "wgrad 1x1 GEMM form: an image's planes are addressed with 32-bit offsets");
    // a co block must not straddle two groups
    SPK_REQUIRE(G == 1 || d->Cout % (64 * mt) == 0, "wgrad 1x1 GEMM form: grouped launches need Cout %% %d == 0 (use the tap kernel)", 64 * mt);
    return SPK_OK;
}
int plan_stem(const spk_wgrad_desc* d, WgradPlan& p) {
    p = stem_geom(d->B, groups_of(d), d->H, d->W, d->splits);
    return complete_plan(d, SPK_WGRAD_STEM, WG_PLAIN, SW_K, 1, p);      // slabs [G 64][147]: the layout of dW itself
}

bool wg_supported(int kh, int kw, int stride) {
    if (kh == 4 && kw == 4) return stride == 2;
    return kh == kw && (kh == 1 || kh == 3 || kh == 7) && (stride == 1 || stride == 2) && !(kh == 7 && stride == 1);
}

// every requirement and every form decision of spk_conv2d_wgrad (the Winograd route has its own: plan_wino)
int plan_wgrad(const spk_wgrad_desc* d, WgradPlan& p) {
    SPK_REQUIRE(d->B > 0 && d->Cin > 0 && d->Cout > 0 && d->H > 0 && d->W > 0 && d->Hin > 0 && d->Win > 0, "wgrad: bad shape");
    SPK_REQUIRE(wg_supported(d->kh, d->kw, d->stride), "wgrad: unsupported kernel %dx%d stride %d", d->kh, d->kw, d->stride);
    SPK_REQUIRE(d->fold <= 1 || (d->groups > 1 && d->groups % d->fold == 0), "wgrad: fold %d must divide groups %d", d->fold, d->groups);
    const bool ups = d->flags & SPK_CONV_UPSAMPLE2X, aff = d->flags & SPK_CONV_IN_AFFINE_RELU, bsc = d->flags & SPK_CONV_IN_BATCH_SCALE;
    SPK_REQUIRE(!(ups && aff) && !(bsc && aff), "wgrad: IN_AFFINE_RELU excludes UPSAMPLE2X and IN_BATCH_SCALE");
    SPK_REQUIRE(!ups || (d->kh == 3 && d->stride == 1), "wgrad: UPSAMPLE2X needs a 3x3 stride-1 kernel");
    SPK_REQUIRE(!aff || (d->in_scale && d->in_shift), "wgrad: IN_AFFINE_RELU without in_scale/in_shift");
    const int pad = (d->kh - 1) / 2;
    if (ups) SPK_REQUIRE(d->H == 2 * d->Hin && d->W == 2 * d->Win, "wgrad: upsampled size mismatch");
    else SPK_REQUIRE(d->H == (d->Hin + 2 * pad - d->kh) / d->stride + 1 && d->W == (d->Win + 2 * pad - d->kw) / d->stride + 1,
                     "wgrad: output size %dx%d does not match input %dx%d", d->H, d->W, d->Hin, d->Win);
    const int mode = aff ? WG_AFFINE_RELU : WG_PLAIN;
    // SPK_CONV_UPSAMPLE2X: x is the low-resolution tensor; the x2 plane is interpolated LDS -> LDS from a source patch
    // (wgrad3x3_up_kernel).  Shapes it does not take (W % 8 != 0, planes under 16 x 4): callers upsample with
    // spk_upsample2x_bilinear_fwd first -- spk_conv2d_wgrad_up_supported tells which.
    if (bsc) {
        // the modulated convolution's weight gradient (StyleGAN2 variant): x * s[b,ci] and g * d'[b,co] formed while staging
        SPK_REQUIRE(d->in_scale && d->g_scale, "wgrad: IN_BATCH_SCALE needs in_scale = s[B,Cin] and g_scale = d'[B,Cout]");
        SPK_REQUIRE(d->kh == 3 && d->stride == 1 && d->groups <= 1, "wgrad: IN_BATCH_SCALE is built for ungrouped 3x3 stride-1 convs");
        SPK_REQUIRE(!ups || (d->flags & SPK_CONV_UP_FIR1331), "wgrad: IN_BATCH_SCALE with UPSAMPLE2X is the upfirdn2d [1,3,3,1] form (SPK_CONV_UP_FIR1331)");
        if (ups) {
            if (up_takes(d)) return plan_up(d, WG_BATCH_SCALE, p);
        } else if (wide_takes(d)) {
            return plan_wide(d, WG_BATCH_SCALE, p);
        }
        return spk::fail(SPK_EUNSUPPORTED, "wgrad: IN_BATCH_SCALE does not take this shape (spk_conv2d_wgrad_mod_supported): pass rescaled tensors");
    }
    SPK_REQUIRE(!(d->flags & SPK_CONV_UP_FIR1331), "wgrad: UP_FIR1331 goes with IN_BATCH_SCALE");
    if (ups) {
        if (up_takes(d)) return plan_up(d, WG_PLAIN, p);
        return spk::fail(SPK_EUNSUPPORTED, "wgrad: SPK_CONV_UPSAMPLE2X does not take this shape: pass the upsampled input (spk_upsample2x_bilinear_fwd)");
    }
    if (g1_takes(d)) return plan_g1(d, mode, p);
    if (wide_takes(d)) return plan_wide(d, mode, p);
    if (s2_takes(d)) return plan_s2(d, mode, p);
    if (d->kh == 4) SPK_REQUIRE(!aff, "wgrad: the 4x4 stride-2 form takes a plain input");
    if (!aff && stem_takes(d)) return plan_stem(d, p);
    return plan_tap(d, mode, p);
}

// raise, launch, check; then the reduce
int launch_wgrad(const WgradPlan& p, hipStream_t stream) {
    int rc = SPK_OK;
    switch (p.form) {
        case SPK_WGRAD_TAP: case SPK_WGRAD_TAP_FIXED: rc = p.kh == 3 && p.stride == 1 ? launch_tap3x3s1(p, stream) : launch_tap(p, stream); break;
        case SPK_WGRAD_PIPE: case SPK_WGRAD_UP: rc = launch_pipe_up(p, stream); break;
        case SPK_WGRAD_WIDE16: case SPK_WGRAD_WIDE8: rc = launch_wide(p, stream); break;
        case SPK_WGRAD_S2_16: case SPK_WGRAD_S2_8: case SPK_WGRAD_STEM: rc = launch_s2_stem(p, stream); break;
        case SPK_WGRAD_GEMM1X1: case SPK_WGRAD_GEMM1X1_DMA: rc = launch_gemm1x1(p, stream); break;
        default: return spk::fail(SPK_EINVAL, "wgrad: no kernel for form %d", p.form);
    }
    if (rc != SPK_OK) return rc;
    return launch_wgrad_reduce(stream, p.args.slabs, p.dw, p.n_slabs, p.red_cout, p.red_cin, p.taps, p.scale, p.accumulate, p.fold);
}

}  // namespace

extern "C" {

int64_t spk_conv2d_wgrad_workspace_bytes(int kh, int kw, int stride, int splits, int B, int Cin, int Cout, int H, int W) {
    if (!wg_supported(kh, kw, stride) || B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return -1;
    // Cout here is the channel count of the gradient tensor (groups * Cout for a grouped launch); mode, alignment and the group
    // count are not known: the most slabs over the forms this shape could reach, each asked through its own geometry function
    int slabs = tap_geom(kh, stride, B, Cin, Cout, H, W, splits).ws_slabs;
    if (kh == 1 && g1_shape(H, W))
        for (int mt = 1; mt <= 2; ++mt) slabs = std::max(slabs, g1_geom(mt, g1_nt(Cin), B, Cin, Cout, H, W, splits).ws_slabs);
    if (kh == 3 && stride == 1 && wide_shape(H, W)) slabs = std::max(slabs, wide_geom(B, Cin, Cout, H, W, splits).ws_slabs);
    if (kh == 3 && stride == 1 && up_shape(H, W)) slabs = std::max(slabs, up_geom(B, Cin, Cout, H, W, splits).ws_slabs);
    if (kh == 3 && stride == 2 && s2_shape(H, W)) slabs = std::max(slabs, s2_geom(B, Cin, Cout, H, W, splits).ws_slabs);
    if (kh == 7 && stem_shape(Cin, Cout, W)) slabs = std::max(slabs, stem_geom(B, Cout / 64, H, W, splits).ws_slabs);
    return (int64_t)slabs * Cout * Cin * kh * kw * (int64_t)sizeof(float);
}

int spk_conv2d_wgrad_up_supported(int B, int Cin, int Cout, int H, int W) {
    // Measured (tools/bench_wgrad.py --upsample, B = 8): the folded form beats "upsample, then the plain kernel" at 256^2
    // (744 vs 775 us, and 268 MB less written and read back), is level with it at 128^2 (668 vs 668, 134 MB less) and 2 %
    // behind at 32^2..64^2, whose x2 images are small (8..67 MB): by default it takes planes at least 128 wide
    // (SPK_WGRAD_UP_MIN_W overrides).
    static const int min_w = [] { const char* e = getenv("SPK_WGRAD_UP_MIN_W"); return e ? atoi(e) : 128; }();
    if (W < min_w) return 0;
    return (B > 0 && Cin > 0 && Cout > 0 && up_shape(H, W) && (long long)Cout * H * W < (1ll << 31) &&
            (long long)Cin * H * W / 4 < (1ll << 31)) ? 1 : 0;
}

int spk_conv2d_wgrad_mod_supported(int B, int Cin, int Cout, int H, int W, int upsample) {
    // shapes (OUTPUT size H x W) whose modulated weight gradient runs fused (SPK_CONV_IN_BATCH_SCALE); 16-byte aligned tensors
    // are a further, per-call condition.  Everything else: rescale the operands first (tiny layers only: 4^2).
    if (B <= 0 || Cin <= 0 || Cout <= 0 || (long long)Cout * H * W >= (1ll << 31) || (long long)Cin * H * W >= (1ll << 31)) return 0;
    return (upsample ? up_shape(H, W) : wide_shape(H, W)) ? 1 : 0;
}

int spk_wgrad_reduce_slabs(const float* slabs, float* dw, int n_slabs, int Cout, int Cin, int taps, float scale, int accumulate, int fold,
                           void* stream) {
    SPK_REQUIRE(slabs && dw && n_slabs > 0 && Cout > 0 && Cin > 0 && taps > 0, "wgrad reduce: bad arguments");
    return launch_wgrad_reduce((hipStream_t)stream, slabs, dw, n_slabs, Cout, Cin, taps, scale, accumulate ? 1 : 0, fold > 1 ? fold : 1);
}

int spk_wgrad_reduce_form(const float* slabs, float* dw, int n_slabs, int Cout, int Cin, int taps, int fold, spk_wgrad_form* out) {
    SPK_REQUIRE(out, "wgrad reduce form: null pointer");
    *out = spk_wgrad_form{};
    SPK_REQUIRE(slabs && dw && n_slabs > 0 && Cout > 0 && Cin > 0 && taps > 0, "wgrad reduce: bad arguments");
    out->fold = fold > 1 ? fold : 1; out->taps = taps; out->n_slabs = n_slabs;
    out->reducer = pick_reducer(slabs, dw, n_slabs, (size_t)Cout * Cin * taps, Cin, out->fold);
    return SPK_OK;
}

int spk_conv2d_wgrad_launch_form(const spk_wgrad_desc* d, spk_wgrad_form* out) {
    SPK_REQUIRE(d && out, "wgrad launch form: null pointer");
    *out = spk_wgrad_form{};
    out->kernel = -1;
    SPK_REQUIRE(d->g && d->x && d->dw, "wgrad: null pointer");
    WgradPlan p;
    const int rc = (d->flags & SPK_CONV_WINOGRAD) ? plan_wino(d, p) : plan_wgrad(d, p);
    if (rc != SPK_OK) return rc;
    spk_wgrad_form& f = *out;
    f.kernel = p.form; f.mode = form_mode(p.mode); f.TW = p.TW; f.TH = p.TH; f.TB = p.TB; f.MT = p.MT; f.NT = p.NT;
    f.n_tiles = p.n_tiles; f.splits = p.splits; f.tiles_per_split = p.tiles_per_split; f.n_slabs = p.n_slabs;
    f.grid_x = (int)p.grid.x; f.grid_y = (int)p.grid.y; f.grid_z = (int)p.grid.z;
    f.reducer = p.reducer; f.fold = p.fold; f.taps = p.taps;
    f.lds_bytes = (int64_t)p.lds_bytes; f.slab_floats = (int64_t)p.slab_floats;
    f.workspace_bytes = (int64_t)(p.ws_slabs * p.slab_floats * sizeof(float));
    return SPK_OK;
}

int spk_conv2d_wgrad(const spk_wgrad_desc* d, void* stream) {
    SPK_REQUIRE(d && d->g && d->x && d->dw, "wgrad: null pointer");
    if (d->flags & SPK_CONV_WINOGRAD) return spk_conv2d_wgrad_wino(d, stream);
    WgradPlan p;
    const int rc = plan_wgrad(d, p);
    if (rc != SPK_OK) return rc;
    return launch_wgrad(p, (hipStream_t)stream);
}

}  // extern "C"
