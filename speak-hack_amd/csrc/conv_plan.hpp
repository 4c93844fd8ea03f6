// Host side of the forward conv family: every launch is PLANNED from its descriptor without a HIP call -- the requirements, the
// kernel choice as integers, the filled argument block, grid, LDS bytes, the split and the finisher -- and then LAUNCHED from the
// plan.  spk_conv2d_launch_form / spk_conv2d_gemm_form copy a plan out instead of launching it (conv_api.hip).
//   tap kernel (configs 0-11)    plan_tap / launch_tap (conv_api.hip); the conv_inst_*.hip units hold the kernel lookups
//   every other family           plan_*(d, plan) states what the form queries report, fwd_*(d, stream) plans the same way with the
//                                unit's own argument block and launches from that plan (the block stays private to the unit: the
//                                kernels' signatures name it)
#pragma once
#include "conv_mfma_f32.hpp"

namespace spkconv {

constexpr int kNumConfigs = 17;   // 12 = the GEMM form of a stride-1 1x1 (conv1x1_gemm.hip): 128co x 128px block, 32-channel k-tiles
constexpr int kTapConfigs = 12;   // 0-11: the tap kernel's tiles (conv_mfma_f32.hpp)
constexpr int kGemmConfig = 12;
constexpr int kDgradS2Config = 13;   // the exact-tap data gradient of a 3x3 stride-2 conv (dgrad3x3s2.hip): 64co x 128px block, 8-channel chunks
constexpr int kGemm2Config = 14;     // the three-per-CU GEMM form of a stride-1 1x1 (conv1x1_gemm2.hip): 128co x 128px block, 16-channel k-tiles
constexpr int kGemm2NarrowConfig = 15;   // the same with a 64co x 128px block (four per CU)
inline bool is_gemm2(int cfg) { return cfg == kGemm2Config || cfg == kGemm2NarrowConfig; }
constexpr int kStemConfig = 16;          // the 7x7 stride-2 stem, Cin 3 -> Cout 64 per group (conv7x7_stem.hip): K = 147 exactly, 16 x 32 pixel tiles

// ---- the tap kernel's tile shape as runtime integers -------------------------------------------------------------------
// What the host needs of Cfg<> and Shape<>, from the same formulas; tap_kernel_ptr() below asserts the two equal for every
// kernel a unit instantiates.
struct TileDesc {
    int CO_T, CI_T, PIX_T, NW, NTHREADS, MT;
    int KH, KW, S, SL, NSLOT, W_FLOATS;
};
//                                             WM WN MT NT CI_T  (the Cfg0 .. Cfg11 typedefs)
constexpr int kTapCfg[kTapConfigs][5] = {{2, 2, 2, 2, 8},  {1, 4, 2, 2, 8},  {2, 2, 1, 1, 8},  {1, 4, 1, 1, 8},
                                         {2, 2, 2, 2, 4},  {1, 4, 2, 2, 4},  {2, 2, 1, 1, 4},  {1, 4, 1, 1, 4},
                                         {2, 2, 2, 2, 16}, {1, 4, 2, 2, 16}, {2, 2, 1, 1, 16}, {1, 4, 1, 1, 16}};
constexpr TileDesc tile_desc(int cfg, int kh, int kw, int s) {
    const int WM = kTapCfg[cfg][0], WN = kTapCfg[cfg][1], MT = kTapCfg[cfg][2], NT = kTapCfg[cfg][3], CI_T = kTapCfg[cfg][4];
    TileDesc t{};
    t.NW = WM * WN; t.NTHREADS = t.NW * 64; t.MT = MT; t.CI_T = CI_T;
    t.CO_T = WM * MT * 32; t.PIX_T = WN * NT * 32;
    t.KH = kh; t.KW = kw; t.S = s;
    t.SL = kh * kw == 1 ? 1 : s;
    const int ph_max = (t.PIX_T / 32 - 1) * t.SL + kh, pw_max = 31 * t.SL + kw;
    const int ppw = CI_T / t.NW > 0 ? CI_T / t.NW : 1;
    t.NSLOT = (ppw * ph_max * pw_max + 63) / 64;
    t.W_FLOATS = kh * kw * CI_T * t.CO_T;
    return t;
}
template <class C, int KH, int KW, int S>
constexpr bool tile_matches(int cfg) {
    using SH = Shape<C, KH, KW, S>;
    const TileDesc t = tile_desc(cfg, KH, KW, S);
    return t.CO_T == C::CO_T && t.CI_T == C::CI_T && t.PIX_T == C::PIX_T && t.NW == C::NW && t.NTHREADS == C::NTHREADS && t.MT == C::MT &&
           t.SL == SH::SL && t.NSLOT == SH::NSLOT && t.W_FLOATS == SH::W_FLOATS;
}
// the one way a unit names a kernel: config ID's tile must be C, or the planner's geometry would not be the kernel's
template <int ID, class C, int KH, int KW, int S, int MODE, bool FG = false>
const void* tap_kernel_ptr() {
    static_assert(tile_matches<C, KH, KW, S>(ID), "tile_desc() disagrees with Cfg<> / Shape<>");
    return reinterpret_cast<const void*>(&conv_kernel<C, KH, KW, S, MODE, FG>);
}
#define SPK_TAP_CFG(id_) id_, Cfg##id_

struct Geometry {
    int TW, TH, TB, PLANE, tiles_x, tiles_y, tiles_b, n_chunks, co_tiles;
    size_t lds_bytes;
    bool ok, one_slot;
};

inline Geometry geometry(const TileDesc& t, int B, int Cin, int Cout, int H, int W) {
    Geometry g;
    g.TW = std::min(32, spk::pow2_ceil(W));
    g.TH = std::min(t.PIX_T / g.TW, spk::pow2_ceil(H));
    g.TB = t.PIX_T / (g.TW * g.TH);
    auto plane = [&]() { return ((g.TH - 1) * t.SL + t.KH) * ((g.TW - 1) * t.SL + t.KW); };
    // the wave's share of the input tile must fit its prefetch slots
    auto slots = [&]() { return spk::ceil_div(t.CI_T * g.TB / t.NW * plane(), 64); };
    while (slots() > t.NSLOT && g.TB > 1 && (t.CI_T * (g.TB / 2)) % t.NW == 0) g.TB >>= 1;  // idle pixel groups
    while (slots() > t.NSLOT && g.TH > 1) g.TH >>= 1;
    g.PLANE = plane();
    g.ok = slots() <= t.NSLOT && (t.CI_T * g.TB) % t.NW == 0 && t.CI_T <= 64;
    g.tiles_x = spk::ceil_div(W, g.TW);
    g.tiles_y = spk::ceil_div(H, g.TH);
    g.tiles_b = spk::ceil_div(B, g.TB);
    g.n_chunks = spk::ceil_div(Cin, t.CI_T);
    g.co_tiles = spk::ceil_div(Cout, t.CO_T);
    const size_t in_floats = ((size_t)t.CI_T * g.TB * g.PLANE + 3) & ~(size_t)3;
    g.one_slot = t.KH * t.KW > 9 && g.n_chunks == 1;   // rolled-loop kernel with a single chunk: no ring needed
    g.lds_bytes = (g.one_slot ? 1 : 3) * (t.W_FLOATS + in_floats + 4) * sizeof(float);   // three-slot ring
    if (g.lds_bytes > 160 * 1024) g.ok = false;
    return g;
}

// number of ci-chunk slices so that the grid fills the chip (about 2 workgroups per CU)
inline int pick_ksplit(const Geometry& g) {
    const long long tiles = (long long)g.tiles_x * g.tiles_y * g.tiles_b * g.co_tiles;
    static const int target = [] { const char* e = getenv("SPK_KSPLIT_TARGET"); return e ? atoi(e) : 512; }();
    int ks = 1;
    while (tiles * ks < target && g.n_chunks / (ks * 2) >= 4 && ks < 64) ks *= 2;
    return ks;
}

inline int resolve_ksplit(const Geometry& g, int requested, int* chunks_per_split) {
    int ks = requested > 0 ? requested : pick_ksplit(g);
    ks = std::max(1, std::min(ks, g.n_chunks));
    const int cps = spk::ceil_div(g.n_chunks, ks);
    if (chunks_per_split) *chunks_per_split = cps;
    return spk::ceil_div(g.n_chunks, cps);
}

// ---- pieces every planner shares ----------------------------------------------------------------------------------------
// A grouped launch: G convs of Cin -> Cout channels side by side; group g reads x channels [g * gin, g * gin + Cin) of Cx (gin = 0:
// every group reads the same input), y has Cy = G * Cout channels.  (64-bit: two planners check the tensors' sizes with them)
struct Groups {
    int G, gin;
    long long Cx, Cy;
};
inline Groups groups_of(const spk_conv2d_desc& d) {
    Groups q;
    q.G = d.groups > 1 ? d.groups : 1;
    q.gin = q.G > 1 ? d.group_in_stride : d.Cin;
    q.Cx = (long long)q.gin * (q.G - 1) + d.Cin;
    q.Cy = (long long)q.G * d.Cout;
    return q;
}
inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
inline float act_gain_of(const spk_conv2d_desc& d) { return d.act_gain != 0.f ? d.act_gain : 1.f; }      // 0 = unset

// The split-K finisher's arguments: the epilogue operands of `d` and its output tensor -- `flags` and `out_scale` as the sliced
// kernel leaves them to the finisher.
inline ConvArgs finisher_args(const spk_conv2d_desc& d, const Groups& q, unsigned flags, float out_scale) {
    ConvArgs f = {};
    f.bias = d.bias; f.noise_w = d.noise_w; f.noise = d.noise; f.style = d.style; f.out_scale_bc = d.out_scale_bc;
    f.stats = d.stats; f.residual = (flags & SPK_EPI_RESIDUAL) ? d.residual : nullptr;
    f.y = d.y; f.y_pre = d.y_pre;
    f.B = d.B; f.Cin = d.Cin; f.Cout = d.Cout; f.H = d.H; f.W = d.W;
    f.G = q.G; f.Cx = (int)q.Cx; f.Cy = (int)q.Cy;
    f.style_stride = d.style_stride; f.flags = flags; f.slope = d.lrelu_slope; f.out_scale = out_scale; f.act_gain = act_gain_of(d);
    f.out_scale_dev = d.out_scale_dev;
    return f;
}

// What runs behind a sliced launch: ksplit > 1 = launch_splitk_epilogue(args, ws, ksplit); ksplit == 1 = nothing.
struct Finish {
    ConvArgs args;
    const float* ws;
    int ksplit;
};
int launch_splitk_epilogue(const ConvArgs& a, const float* ws, int ksplit, hipStream_t stream);
// the finisher launch_splitk_epilogue runs for these tensors: 2 = vector (*seg lanes of a wave share a plane), 1 = scalar (*seg = 0)
int splitk_finisher(const ConvArgs& a, const float* ws, int* seg);
inline int launch_finish(const Finish& f, hipStream_t stream) {
    return f.ksplit > 1 ? launch_splitk_epilogue(f.args, f.ws, f.ksplit, stream) : (int)SPK_OK;
}

// ---- the tap kernel (conv_api.hip) --------------------------------------------------------------------------------------
// Where spk_conv2d_fwd's routing sends a descriptor.  d: the descriptor the family plans -- config resolved; for the 2x2 parity forms
// of SPK_CONV_DGRAD_S2 / SPK_CONV_TRANSPOSE4X4_S2 rewritten to the four-class 2x2 conv, whose destination is Hd x Wd.
enum Family { FAM_TAP, FAM_GEMM, FAM_GEMM2, FAM_STEM, FAM_DGRAD_S2, FAM_WINO, FAM_BF16X3 };
struct Route {
    int family;
    spk_conv2d_desc d;
    int mode;                // input-stage mode of a tap / GEMM / stem launch
    int Hd, Wd, pshift;      // 2x2 parity forms (else 0)
};

struct TapPlan {
    int config, mode;        // the kernel: tap_kernel(kh, stride, config, mode, fixed_geometry)
    bool fixed_geometry, ragged;
    const void* kernel;
    Geometry g;              // co_tiles counts every group (grid.y); lds_bytes is the launch's (ring, or the staged epilogue's tile)
    ConvArgs args;
    dim3 grid;
    int nthreads;
    Finish finish;           // finish.ksplit = grid.z
};
int plan_tap(const Route& r, TapPlan& p);
int launch_tap(const TapPlan& p, hipStream_t stream);

// one lookup per kernel unit: the instantiation for (config, mode, fixed geometry), null where the unit builds none
const void* tap_kernel_3x3s1_a(int cfg, int mode, bool fg);            // ids 0-3
const void* tap_kernel_3x3s1_b(int cfg, int mode, bool fg);            // ids 4-7
const void* tap_kernel_3x3s1_stats(int cfg, int mode, bool fg);        // ids 0-7, MODE_PLAIN_STATS
const void* tap_kernel_s2(int kh, int cfg, int mode, bool fg);         // ids 4-7: 3x3, 4x4 and 7x7 stride 2
const void* tap_kernel_1x1(int stride, int cfg, int mode, bool fg);    // ids 8-11
const void* tap_kernel_2x2(int cfg, int mode, bool fg);                // ids 0-3

// ---- the GEMM forms of a 1x1 (configs 12, 14, 15) and the stem (16) --------------------------------------------------------
struct GemmPlan {
    spk_gemm_form form;      // the plan's integers are the public form's, field for field (include/spk.h)
    dim3 grid;
    size_t lds_bytes;
};
int plan_1x1_gemm(const spk_conv2d_desc* d, GemmPlan& p);                                  // id 12
int fwd_1x1_gemm(const spk_conv2d_desc* d, hipStream_t s);
int plan_1x1_gemm2(const spk_conv2d_desc* d, GemmPlan& p);                                 // ids 14, 15
int fwd_1x1_gemm2(const spk_conv2d_desc* d, hipStream_t s);
int plan_stem(const spk_conv2d_desc* d, GemmPlan& p);                                      // id 16
int fwd_stem(const spk_conv2d_desc* d, hipStream_t s);

// ---- the sliced families: the exact-tap stride-2 data gradient (config 13) and Winograd -------------------------------------
struct SlicedPlan {
    int config;              // 13, or -1 (Winograd)
    Finish finish;           // finish.ksplit = contraction slices of the launch
};
int plan_dgrad_s2_fused(const spk_conv2d_desc* d, SlicedPlan& p);                          // id 13
int fwd_dgrad_s2_fused(const spk_conv2d_desc* d, hipStream_t s);
int plan_wino(const spk_conv2d_desc* d, SlicedPlan& p);                                    // conv3x3_wino_f32.hip; launched by
                                                                                           // spk_conv2d_wino_fwd (include/spk.h)

bool dgrad_s2_fused_takes(int B, int K, int Cc, int Hg, int Wg);
int dgrad_s2_ksplit(int B, int K, int Cc, int Hg, int Wg, int G);         // contraction slices of the exact-tap kernel (1 = none)
long long dgrad_s2_fused_packed_floats(int K, int Cc);
bool gemm1x1_takes(int kh, int stride, int Cin, int H, int W);
long long gemm1x1_pixel_tiles(int B, int H, int W);
bool gemm2_takes(int kh, int stride, int Cin, int Cout, int H, int W);
int gemm2_co_tile(int config);
long long gemm2_pixel_tiles(int B, int H, int W);
long long gemm2_packed_floats(int config, int Cin, int Cout);
bool stem_takes(int kh, int stride, int Cin, int Cout, int H, int W);
long long stem_packed_floats();
void stem_tiles(int H, int W, int* tiles_x, int* tiles_y);

// several weight tensors of one shape on one launch (blockIdx.y = which): their packed images one after another, as a
// grouped conv launch reads them
struct PackList { const float* w[SPK_PACK_LIST_MAX]; };
int pack_gemm2(const PackList& list, int n_list, float* w_packed, int Cin, int Cout, int config, int tf, hipStream_t stream);
int pack_stem(const PackList& list, int n_list, float* w_packed, int Cin, int Cout, int tf, hipStream_t stream);

}  // namespace spkconv
