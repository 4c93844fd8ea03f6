// 3x3 stride-1 pad-1 convolution as Winograd F(2x2, 3x3) on the gfx950 f32 MFMA pipe -- fp32 operands, fp32 products, fp32
// accumulation, 16 multiplies per 2x2 output tile and (ci, co) pair where the direct form spends 36: 2.25x fewer matrix
// instructions for the same convolution.  This is what the reference's own backend does for these layers (PyTorch hands an
// fp32 3x3 nn.Conv2d -- styleganv1.py:615-616,625,630; the discriminator's conv1 of every block, styleganv1.py:662-672 -- to
// MIOpen, whose fp32 3x3 solvers are Winograd kernels); the arithmetic differs from the direct form only in summation order
// and in the +-1, 1/2 transforms: 1e-6-class rel-L2 per layer, asserted in tests/test_wino_gpu.py (bound of the path: 1e-3).
//
//   Y = A^T [ (G g G^T) (.) (B^T d B) ] A      per 2x2 output tile, per (co, ci);  d = the 4x4 input patch of the tile
//     U[xi][co][ci] = G g G^T     -- weights, transformed at PACK time (spk_conv2d_pack_weights_wino), xi = 4 i + j in 0..15
//     V[xi][ci][t]  = B^T d B     -- input patches, transformed while staging (32 adds per patch)
//     M[xi][co][t]  = sum_ci U[xi][co][ci] V[xi][ci][t]   -- SIXTEEN independent GEMMs: v_mfma_f32_32x32x2_f32, A = U, B = V
//     Y = A^T M A                 -- 24 adds per (co, tile), lane-local: the 16 M[xi] of a (co, tile) sit in the same
//                                    accumulator position of 16 accumulator tiles
//
// Block = 64 co x 64 tiles (16 x 4 tiles = 32 x 8 output pixels), 4 waves (2 x 2: 32 co x 32 tiles each), ci chunks of 8.
// A wave holds 16 accumulator tiles = 256 registers: ONE wave per SIMD, one workgroup per CU, so the wave hides its own
// latencies (the weight-gradient kernels' situation): everything that feeds chunk i + 1 is interleaved, one piece behind one
// MFMA, with the 64 MFMAs of chunk i.
//   * U: LDS-DMA (global_load_lds_dwordx4) of the chunk's contiguous 32 KB packed block, one chunk ahead, 2 slots;
//   * raw input: `buffer_load_dword ... lds` gathers -- a lane fetches any address, the wave's 64 dwords land consecutively in
//     LDS; addresses outside the image are out of range of the buffer descriptor and return 0, which IS the zero padding: no
//     select, no mask, no vector instruction.  Wave w stages the planes of channels w and w + 4 for itself (10 x 34 floats
//     each, two chunks ahead, 2 slots) and transforms them: no other wave reads its raw tile;
//   * V: wave w transforms its two planes for all 64 tiles (a lane = a tile: 8 ds_read_b64 + 32 adds + 16 ds_write_b32 per
//     plane; the x2 form: a lane = a pair of tiles of one plane, below), 2 slots;  one barrier per chunk.
// LDS: 2 x 32 KB (U) + 2 x 32 KB (V) + 2 x 11 KB (raw) = 150 KB.  Vector instructions per chunk of 64 MFMAs: 64 adds.
// Epilogue: output transform and the f32 kernel's epilogue element for element (out_scale, bias, noise, LeakyReLU, [y_pre], style,
// [accumulate]) in registers; a lane stores its tile's 2 x 2 pixels as two 8-byte stores, 16 lanes a whole 128-byte line.
// A bilinear x2 layer (SPK_CONV_UPSAMPLE2X, template parameter UP) reads the low-resolution tensor: B^T (bilinear) B collapses into one
// 4 x 3 matrix per dimension (up1d_, 7 vector ops) on a 3 x 3 raw window per tile; no x2 image exists.  There a lane is NOT a tile: a
// half-wave takes one of the wave's two planes and a lane a vertical PAIR of tiles, whose 3 x 3 windows share two raw rows -- the row
// pass (up1d_ along a raw row; its edge coefficients depend on the tile column only) runs once per shared row: a 4 x 3 window, 4
// ds_read2_b32 + 4 ds_read_b32, 4 + 2 x 4 = 12 up1d_ = 84 vector ops, 32 ds_write_b32 per lane and chunk, where a lane per tile and
// plane took 12 reads, 14 up1d_ = 98 ops, 32 writes.  Every V value keeps its bits.  (The plain form's horizontal pairs --
// 6 shared columns, 56 adds for 64 -- were measured and bought nothing: DESIGN.md 4.12.)
#include "conv_plan.hpp"

namespace spkwino {

using spkconv::f32x16;
using spkconv::lds_f32_t;
using spkconv::static_for;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) f32x2 lds_f32x2_t;
typedef __attribute__((address_space(3))) f32x2 __attribute__((aligned(4))) lds_f32x2u_t;     // an 8-byte LDS access at any 4-byte address

constexpr int CO_T = 64, CI_T = 8, NTILE = 64, NT = 256;
// region shapes (64 tiles each): WIDE = 32 x 8 output pixels (16 x 4 tiles) -- whole 128-byte output lines; SQUARE = 16 x 16 (8 x 8 tiles)
// for images narrower than 32 pixels.  Raw plane with its halo: 34 x 10 = 340 / 18 x 18 = 324 floats, both within the 352-float pitch.
constexpr int WIDE = 0, SQUARE = 1;
constexpr int region_w(int shape) { return shape == SQUARE ? 16 : 32; }
constexpr int region_h(int shape) { return shape == SQUARE ? 16 : 8; }
constexpr int RAW_PLANE = 352, RAW_WAVE = 2 * RAW_PLANE;                    // 704 = 11 x 64: a wave's two planes = 11 gathers
constexpr int RAW_GATHERS = RAW_WAVE / 64;
constexpr int U_FLOATS = 16 * CI_T * CO_T, V_FLOATS = 16 * CI_T * NTILE, RAW_FLOATS = 4 * RAW_WAVE;
constexpr int U_OFF = 0, V_OFF = 2 * U_FLOATS, RAW_OFF = V_OFF + 2 * V_FLOATS;
constexpr int PRM_OFF = RAW_OFF + 2 * RAW_FLOATS;                            // [64 co][bias, noise weight, style s0 + 1, style s1] of the region
constexpr int DEM_OFF = PRM_OFF + 4 * CO_T;                                  // [64 co] demodulation d[b, co] of the region's image (modulated convs)
constexpr int RGBW_OFF = DEM_OFF + CO_T;                                     // [3][64 co] weights of a fused toRGB (SPK_EPI_TORGB)
constexpr int LDS_FLOATS = RGBW_OFF + 3 * CO_T;
constexpr int LDS_BYTES = LDS_FLOATS * 4;                                    // 155 648
constexpr int RGB_PART_OFF = V_OFF + V_FLOATS;                               // toRGB partial sums [4 channel groups][64 tiles][3][4 px]: V slot 1, idle during an epilogue
static_assert(RAW_GATHERS == 11 && 34 * 10 <= RAW_PLANE && 18 * 18 <= RAW_PLANE, "geometry");
// UP (a bilinear x2 layer, SPK_CONV_UPSAMPLE2X): the raw plane is the LOW-resolution window of the region with a one-pixel halo --
// 18 x 6 (WIDE) / 10 x 10 (SQUARE) floats at a pitch of 128 inside the wave's 704: a wave's two planes = 4 gathers
constexpr int UP_PLANE = 128, UP_GATHERS = 2 * UP_PLANE / 64;
static_assert(18 * 6 <= UP_PLANE && 10 * 10 <= UP_PLANE && 2 * UP_PLANE <= RAW_WAVE, "geometry");
constexpr int U_DMA = U_FLOATS * 4 / 1024 / 4;                               // 1 KB blocks per wave and chunk (8)
// LAB knock-outs of the K loop (tools/build_wino_lab.py, one switch per library): a switch removes instructions
// only -- never a wait or the barrier -- and every LDS and global address stays in range.  The results are wrong: only the time is read.
#if defined(SPK_WINO_LAB) && defined(SPK_WINO_KO)
constexpr int KO = SPK_WINO_KO;
#else
constexpr int KO = 0;
#endif
constexpr bool KO_U = KO & 1;            // no U pieces
constexpr bool KO_RAW = KO & 2;          // no raw gathers
constexpr bool KO_TVALU = KO & 4;        // no transform vector ops (the raw reads and the V writes stay: V = raw values)
constexpr bool KO_VWRITE = KO & 8;       // no V writes
constexpr bool KO_UBARE = KO & 16;       // U pieces without their scalar companions: m0 once per chunk, all eight to one address

struct Args {
    const float* x;
    const float* wp;
    const float* bias;
    const float* noise_w;
    const float* noise;
    const float* style;
    float* y;
    float* y_pre;
    const float* out_scale_dev;
    const float* in_scale;       // MOD: [B, Cin] modulation s[b, ci] (SPK_CONV_IN_BATCH_SCALE): the conv runs on x * s
    const float* out_scale_bc;   // MOD: [B, Cout] demodulation d[b, co] applied right after the contraction, or null
    const float* rgb_w;          // RGB: [3][Cout] weights / [3] bias of the 1x1 conv fused behind the epilogue, its output [B,3,H,W]
    const float* rgb_bias;
    float* rgb_y;
    int B, Cin, Cout, H, W;
    int G, gin, Cx, Cy, co_tiles_g;   // groups (the encoders' passes side by side): Cin / Cout per group; x has Cx = gin * (G - 1) + Cin channels,
                                 // y has Cy = G * Cout; blockIdx.y = group * co_tiles_g + channel tile; the groups' images one after another
    int regions_x, regions_y;
    int n_chunks;                // of the whole contraction (the packed image's chunk count)
    int ksplit, cps;             // the contraction in `ksplit` slices of `cps` chunks (even), a work item = (region, slice)
    size_t slice_floats;         // ksplit > 1: slice z writes its partial sums at y + z * slice_floats (the caller's split-K workspace)
    int style_stride;
    unsigned flags;
    unsigned x_bytes;
    float slope, out_scale, act_gain;
};

// ---- weights: U = G g G^T, image [co tile 64][chunk 8][xi 16][ci 8][co 64] (zero padded), one 32 KB block per (co tile, chunk) ----
__global__ void pack_wino_kernel(const float* __restrict__ w, float* __restrict__ out, int Cin, int Cout, int opCin, int opCout,
                                 int transpose_flip, int n_chunks, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int co_l = (int)(idx % CO_T);
    long long r = idx / CO_T;
    const int ci_l = (int)(r % CI_T);
    r /= CI_T;
    const int xi = (int)(r % 16);
    r /= 16;
    const int chunk = (int)(r % n_chunks), co_tile = (int)(r / n_chunks);
    const int co = co_tile * CO_T + co_l, ci = chunk * CI_T + ci_l;
    float v = 0.f;
    if (co < opCout && ci < opCin) {
        float g[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b)
                // transpose_flip: the data-gradient operator, w'[co][ci][a][b] = w[ci][co][2-a][2-b] (co indexes the forward conv's Cin)
                g[a][b] = transpose_flip ? w[(((size_t)ci * Cin + co) * 3 + (2 - a)) * 3 + (2 - b)] : w[(((size_t)co * Cin + ci) * 3 + a) * 3 + b];
        const int i = xi >> 2, j = xi & 3;
        // rows of G: [1,0,0], [.5,.5,.5], [.5,-.5,.5], [0,0,1]
        float t[3];   // (G g)[i][b]
#pragma unroll
        for (int b = 0; b < 3; ++b)
            t[b] = i == 0 ? g[0][b] : (i == 3 ? g[2][b] : 0.5f * ((g[0][b] + g[2][b]) + (i == 1 ? g[1][b] : -g[1][b])));
        v = j == 0 ? t[0] : (j == 3 ? t[2] : 0.5f * ((t[0] + t[2]) + (j == 1 ? t[1] : -t[1])));
    }
    out[idx] = v;
}

// the same for up to 32 weights in ONE launch (blockIdx.y = item): a training step re-packs both images of every decoder layer after
// each optimizer step -- 20 launches of 26-35 us beside a busy second stream
struct PackWinoList {
    const float* w[SPK_WINO_PACK_MAX];
    float* out[SPK_WINO_PACK_MAX];
    int Cin[SPK_WINO_PACK_MAX], Cout[SPK_WINO_PACK_MAX], tf[SPK_WINO_PACK_MAX];
};

__global__ void pack_wino_list_kernel(const PackWinoList a) {
    const int it = blockIdx.y;
    const float* __restrict__ w = a.w[it];
    float* __restrict__ out = a.out[it];
    const int Cin = a.Cin[it], Cout = a.Cout[it], transpose_flip = a.tf[it];
    const int opCin = transpose_flip ? Cout : Cin, opCout = transpose_flip ? Cin : Cout;
    const int n_chunks = (opCin + CI_T - 1) / CI_T;
    const long long total = (long long)((opCout + CO_T - 1) / CO_T) * n_chunks * U_FLOATS;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int co_l = (int)(idx % CO_T);
        long long r = idx / CO_T;
        const int ci_l = (int)(r % CI_T);
        r /= CI_T;
        const int xi = (int)(r % 16);
        r /= 16;
        const int chunk = (int)(r % n_chunks), co_tile = (int)(r / n_chunks);
        const int co = co_tile * CO_T + co_l, ci = chunk * CI_T + ci_l;
        float v = 0.f;
        if (co < opCout && ci < opCin) {            // (the arithmetic of pack_wino_kernel, expression for expression)
            float g[3][3];
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    g[p][q] = transpose_flip ? w[(((size_t)ci * Cin + co) * 3 + (2 - p)) * 3 + (2 - q)] : w[(((size_t)co * Cin + ci) * 3 + p) * 3 + q];
            const int i = xi >> 2, j = xi & 3;
            float t[3];
#pragma unroll
            for (int q = 0; q < 3; ++q)
                t[q] = i == 0 ? g[0][q] : (i == 3 ? g[2][q] : 0.5f * ((g[0][q] + g[2][q]) + (i == 1 ? g[1][q] : -g[1][q])));
            v = j == 0 ? t[0] : (j == 3 ? t[2] : 0.5f * ((t[0] + t[2]) + (j == 1 ? t[1] : -t[1])));
        }
        out[idx] = v;
    }
}

// One vector add / subtract, spelled out: given the whole transform, the compiler pairs the operands for v_pk_add_f32 and pays for
// it with a v_mov_b32 per pair (24 moves per chunk of 64 MFMAs; a packed op costs its two scalar ones on this part anyway).
__device__ __forceinline__ float fadd_(float a, float b) { float r; asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float fsub_(float a, float b) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// UP: the 1-D input transform of a tile of a bilinear x2 layer, from the tile's three LOW-resolution pixels.  The tile's 4-wide window
// of the x2 image, times 4, is (3a + b, a + 3b, 3b + c, b + 3c) for raw neighbours a, b, c (align_corners=False: taps 1/4, 3/4; at an
// image edge the missing neighbour is the edge pixel itself: the gather's business), and B^T of it
//   o0 = 3a - 2b - c,  o1 = a + 6b + c,  o2 = c - a,  o3 = a + 2b - 3c
// With e = c - a, s = a + c: o1 = 6b + s, o2 = e, o0 = (s - kL b) - 2e, o3 = -2e - (s - kR b), kL = kR = 2.  The conv's ZERO padding of
// the x2 image -- window element 0 (3) of a tile in the image's first (last) tile column is 0, not the clamped interpolation -- is
// kL = 6 (kR = 6): with a = b, o0 = (3 - kL) b - c = -3b - c.  7 vector ops for 3 -> 4 values; nkl / nkr hold -kL / -kR.  Two passes
// (rows, columns) give 16 V: the factor is exact and leaves through out_scale.
__device__ __forceinline__ void up1d_(float a, float b, float c, float nkl, float nkr, float six, float& o0, float& o1, float& o2, float& o3) {
    // ONE asm statement: between two asm statements of which the second reads a register the first wrote, the compiler -- it cannot see
    // what the instructions are -- puts an s_nop (24.5 per chunk of 64 MFMAs in the K loop); no vector-ALU pair here needs one
    float e, s, hl, hr;
    asm("v_sub_f32 %0, %9, %7\n\tv_add_f32 %1, %7, %9\n\tv_fma_f32 %2, %8, %12, %1\n\tv_fma_f32 %3, %8, %10, %1\n\t"
        "v_fma_f32 %4, %8, %11, %1\n\tv_fma_f32 %5, %0, -2.0, %3\n\tv_fma_f32 %6, %0, -2.0, -%4"
        : "=&v"(e), "=&v"(s), "=&v"(o1), "=&v"(hl), "=&v"(hr), "=&v"(o0), "=v"(o3)
        : "v"(a), "v"(b), "v"(c), "v"(nkl), "v"(nkr), "s"(six));
    o2 = e;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() is a fence: it waits for vmcnt(0) too, i.e. for every global
// STORE the wave has issued -- behind the epilogue's stores that is a full HBM write latency (~5 000 cycles, measured with
// tools/lab_wino_phases.py) with the matrix pipe idle, twice per region.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// MOD: the modulated convolution of the StyleGAN2 variant.  B^T (d s) B = s B^T d B: the modulation of the
// plane's channel -- one scalar per plane, the region lies in one image -- multiplies the 16 transformed values (16 more vector ops
// per plane); the demodulation rides on the epilogue's out_scale through a second LDS table.
// RGB (SPK_EPI_TORGB): the layer's 64 output channels sit in ONE workgroup (Cout <= 64), so the 1x1 conv to 3 channels that follows the
// last block (styleganv1.py:607) is a reduction over the epilogue's own registers: 12 fused multiply-adds per channel row, the four
// channel groups (2 waves x 2 half-waves) meet through LDS.  The 134 MB activation is then neither re-read nor -- y == NULL -- written.
// UP (SPK_CONV_UPSAMPLE2X, plain launches): p.x is the LOW-resolution tensor [B, Cx, H/2, W/2]; everything that speaks of the output
// keeps H, W.  Raw plane, gathers and input transform change (up1d_), nothing behind V does.
// EPI: the form of the epilogue's channel rows, chosen by the host.  GENERIC: every per-launch condition inside the row (a partial last
// channel tile, y_pre, SPK_EPI_ACCUM, the modulated forms).  LEAN: whole channel tiles, no y_pre, no accumulate, 0 < slope <= 1 -- a row
// is straight-line code: no branch, a wave-uniform base plus one 32-bit lane offset as store address, LeakyReLU as multiply / max.
// LEAN_NOSTORE (RGB only): the same without the activation's stores (y == NULL: only the fused toRGB's image leaves).
constexpr int GENERIC = 0, LEAN = 1, LEAN_NOSTORE = 2;
template <bool MOD, int SHAPE, bool RGB = false, bool UP = false, int EPI = GENERIC>
__global__ __launch_bounds__(NT) void wino_kernel(const Args p) {
    static_assert(!(UP && MOD), "the modulated conv keeps its x2 pass");
    static_assert(EPI == GENERIC || !MOD, "the modulated forms keep the generic rows");
    static_assert(EPI != LEAN_NOSTORE || RGB, "only a fused toRGB launch may leave the activation unwritten");
    constexpr int RW = region_w(SHAPE), RH = region_h(SHAPE), TXN = RW / 2, TYN = RH / 2;
    constexpr int RAW_W = UP ? RW / 2 + 2 : RW + 2, RAW_H = UP ? RH / 2 + 2 : RH + 2, RAW_USED = RAW_W * RAW_H;
    constexpr int PLANE = UP ? UP_PLANE : RAW_PLANE, NG = UP ? UP_GATHERS : RAW_GATHERS;       // a raw plane's pitch; a wave's gathers per chunk
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l32 = lane & 31;
    const int wm = wave >> 1, wn = wave & 1;

    // PERSISTENT workgroups (one per CU: the kernel holds 512 registers per lane): workgroup w walks regions of its XCD's
    // contiguous share of the region list (the hardware deals workgroup w to XCD w % 8), neighbours in the list running
    // side by side on the same L2 -- and, the point of it, the first loads of region r + 1 are requested BEFORE the epilogue
    // of region r, so that a region's global-load latency hides behind its predecessor's output transform and stores.
    const int n_regions = p.regions_x * p.regions_y * p.B * p.ksplit;      // work items: (region, contraction slice), slice fastest
    const int xcd = (int)blockIdx.x & 7, wk = (int)blockIdx.x >> 3, wpx = (int)gridDim.x >> 3;      // (host: gridDim.x % 8 == 0)
    const int share_q = n_regions >> 3, share_r = n_regions & 7;
    const int reg_begin = xcd * share_q + min(xcd, share_r), reg_end = reg_begin + share_q + (xcd < share_r ? 1 : 0);
    const int grp = (int)blockIdx.y / p.co_tiles_g, co_tile = (int)blockIdx.y - grp * p.co_tiles_g, co0 = co_tile * CO_T;     // co0: within the group
    const size_t HW = (size_t)p.H * p.W;
    const int Win = UP ? p.W >> 1 : p.W;                   // the input's row pitch / plane size
    const size_t HWin = UP ? HW >> 2 : HW;

    // ---- the raw gathers: byte offsets of this lane's 11 (UP: 4) elements (plane j of channel wave + 4 j), or out of range ----
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)p.x_bytes, 0x00020000);
    unsigned voff[NG], voff_next[NG];   // the gathers of the region being requested / of the region after it
    auto region_coords = [&](int item, int& b_, int& y0_, int& x0_, int& kb_) {
        const int reg = item / p.ksplit;
        kb_ = (item - reg * p.ksplit) * p.cps;               // first chunk of the item's slice
        const int rx_ = reg % p.regions_x;
        const int t_ = reg / p.regions_x;
        b_ = t_ / p.regions_y;
        y0_ = (t_ - b_ * p.regions_y) * RH;
        x0_ = rx_ * RW;
    };
    // per lane and gather, once: the element's byte offset from the region's origin pixel in plane 0 of the image (wraps for the
    // halo's row -1 / column -1: the sum with the origin is in range whenever the element exists), and which image edges would
    // put it outside (bit 0: region at the top edge, 1: bottom, 2: left, 3: right, 4: the pitch's padding -- never loaded); the edge
    // bits of six gathers share a register (they are alive through the whole kernel: 2 registers for 11 gathers, not 11)
    constexpr int NE = (NG + 5) / 6;
    unsigned rel[NG], edges[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) edges[k] = 0u;
#define WINO_EDGE(k_) ((edges[(k_) / 6] >> (5 * ((k_) % 6))) & 31u)
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const int e = k * 64 + lane;
        const int j = e >= PLANE ? 1 : 0, q = e - j * PLANE;
        const int r = q / RAW_W, c = q - r * RAW_W;
        rel[k] = ((unsigned)(wave + 4 * j) * (unsigned)HWin + (unsigned)((r - 1) * Win + (c - 1))) * 4u;
        edges[k / 6] |= ((r == 0 ? 1u : 0u) | (r == RAW_H - 1 ? 2u : 0u) | (c == 0 ? 4u : 0u) | (c == RAW_W - 1 ? 8u : 0u) | (q >= RAW_USED ? 16u : 0u)) << (5 * (k % 6));
    }
    auto set_voff = [&](unsigned (&vo)[NG], int b_, int y0_, int x0_) {
        // (host: the whole tensor is below 2^29 floats)
        const unsigned origin = (((unsigned)b_ * (unsigned)p.Cx + (unsigned)(grp * p.gin)) * (unsigned)HWin +
                                 (unsigned)(UP ? (y0_ >> 1) * Win + (x0_ >> 1) : y0_ * p.W + x0_)) * 4u;
        const unsigned at = (y0_ == 0 ? 1u : 0u) | (y0_ + RH >= p.H ? 2u : 0u) | (x0_ == 0 ? 4u : 0u) | (x0_ + RW >= p.W ? 8u : 0u) | 16u;
        if constexpr (UP) {
            // a halo element outside the image reads the CLAMPED neighbour (the bilinear pass's edge rule): one row / one column
            // back inside -- always in range; the zero padding of the x2 image is the edge tiles' coefficient (set_nk)
            const unsigned row_bytes = (unsigned)Win * 4u;
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                const unsigned h = WINO_EDGE(k) & at;
                vo[k] = (h & 16u) ? 0x80000000u
                                  : origin + rel[k] + ((h & 1u) ? row_bytes : 0u) - ((h & 2u) ? row_bytes : 0u) + ((h & 4u) ? 4u : 0u) - ((h & 8u) ? 4u : 0u);
            }
        } else {
#pragma unroll
            for (int k = 0; k < NG; ++k) vo[k] = (WINO_EDGE(k) & at) ? 0x80000000u : origin + rel[k];
        }
    };
    const unsigned chunk_bytes = (unsigned)(CI_T * HWin * 4);
    const float* wsrc = p.wp + (size_t)blockIdx.y * p.n_chunks * U_FLOATS;

    // LDS-DMA as inline assembly: the compiler treats a pending `... lds` load as a flat access that may complete out of order
    // with the ds_reads and answers with s_waitcnt lgkmcnt(0) in front of EVERY fragment use until the next vmcnt(0) -- with one
    // wave per SIMD that is an LDS round trip per four MFMAs.  Issued behind its back, the fragment reads keep their counted
    // waits (lgkmcnt(6)); completion is this kernel's business: s_waitcnt vmcnt(0) before the chunk barrier.  (LDS base = 0:
    // the kernel has no static LDS.)
#define WINO_DMA_RAW(vo_in_, chunk_, slot_, k_)                                                                         \
    {   /* (operands through locals: an asm operand inside a lambda does not capture) */                                \
        const unsigned m0_ = (unsigned)((RAW_OFF + (slot_) * RAW_FLOATS + (k_) * 64) * 4) + raw_m0, vo_ = (vo_in_);     \
        const unsigned so_ = (unsigned)(chunk_) * chunk_bytes;                                                          \
        const __amdgpu_buffer_rsrc_t rs_ = rsrc;                                                                        \
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds" :: "s"(m0_), "v"(vo_), "s"(rs_), "s"(so_)); \
    }
#define WINO_DMA_U(chunk_, slot_, k_)                                                                                   \
    {                                                                                                                   \
        const unsigned m0_ = (unsigned)((U_OFF + (slot_) * U_FLOATS) * 4 + (k_) * 1024) + u_m0, vo_ = lane16;           \
        const float* sb_ = wsrc + (size_t)(chunk_) * U_FLOATS + (wave * U_DMA + (k_)) * 256;                            \
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" :: "s"(m0_), "v"(vo_), "s"(sb_));   \
    }
#define WINO_DMA_U_BARE(chunk_, slot_, k_)        /* LAB (KO_UBARE) */                                                  \
    {                                                                                                                   \
        const unsigned m0_ = (unsigned)((U_OFF + (slot_) * U_FLOATS) * 4) + u_m0, vo_ = lane16;                         \
        const float* sb_ = wsrc + (size_t)(chunk_) * U_FLOATS + (wave * U_DMA) * 256;                                   \
        if constexpr ((k_) == 0) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" :: "s"(m0_));                               \
        asm volatile("global_load_lds_dwordx4 %0, %1" :: "v"(vo_), "s"(sb_));                                           \
    }
    const unsigned raw_m0 = (unsigned)(wave * RAW_WAVE * 4), u_m0 = (unsigned)(wave * U_DMA * 1024), lane16 = (unsigned)lane * 16u;

    // ---- per-lane LDS bases (floats); everything else is an instruction immediate ----
    // (made opaque: the compiler then folds only the small compile-time parts into the 16-bit instruction offsets instead of
    // materialising one address register per constant that does not fit)
    int a_base = U_OFF + half * CO_T + wm * 32 + l32;               // + slot * U_FLOATS + (xi * 8 + 2 kk) * 64
    int b_base = V_OFF + half * NTILE + wn * 32 + l32;              // + slot * V_FLOATS + (xi * 8 + 2 kk) * 64
    // The input transform's lanes.  Plain and modulated forms: a lane = tile `lane` of the region, for both of the wave's planes.
    // UP: half-wave `half` transforms plane `half` of the wave (channel wave + 4 half of the chunk), lane l32 of it a PAIR of tiles, (ty_l,
    // tx_l) and the one below it (ty_l is even, as is TYN): the first 1-D pass runs once over the two raw rows the tiles share.
    static_assert(TYN % 2 == 0, "UP: vertical tile pairs");
    const int ty_l = UP ? 2 * (l32 / TXN) : lane / TXN, tx_l = UP ? l32 % TXN : lane % TXN;
    int raw_rd = (RAW_OFF + wave * RAW_WAVE + 2 * ty_l * RAW_W + 2 * tx_l) >> 1;   // in float pairs; + slot * RAW_FLOATS + j * RAW_PLANE + r * 34 + {0, 2}
    // + slot * V_FLOATS + (xi * 8 + 4 j) * 64;  UP: the lane's plane is part of the base, + slot * V_FLOATS + xi * 8 * 64 (+ TXN: the tile below)
    int v_wr = UP ? V_OFF + (wave + 4 * half) * NTILE + ty_l * TXN + tx_l : V_OFF + wave * NTILE + lane;
    asm volatile("" : "+v"(a_base), "+v"(b_base), "+v"(raw_rd), "+v"(v_wr));
    // UP: a lane (tiles ty_l, ty_l + 1 of column tx_l) reads rows ty_l .. ty_l + 3, columns tx_l .. tx_l + 2 of the haloed low-resolution
    // plane: 4-byte aligned only (ds_read2_b32 + ds_read_b32, whose offsets reach 1 KB: one base per raw slot)
    int raw_u[2];
    // -kT of the pair's top tile, -kB of its bottom tile, -kL, -kR of both, in the item whose planes are being transformed / in the next
    // item; the pair's inner two (the top tile's kB, the bottom tile's kT) are 2 everywhere: neg2
    float nk[4] = {-2.f, -2.f, -2.f, -2.f}, nkn[4] = {-2.f, -2.f, -2.f, -2.f};
    float neg2 = -2.f;
    const float six = 6.f;
    auto set_nk = [&](float (&k_)[4], int y0_, int x0_) {
        k_[0] = (y0_ == 0 && ty_l == 0) ? -6.f : -2.f;
        k_[1] = (y0_ + RH >= p.H && ty_l + 1 == TYN - 1) ? -6.f : -2.f;
        k_[2] = (x0_ == 0 && tx_l == 0) ? -6.f : -2.f;
        k_[3] = (x0_ + RW >= p.W && tx_l == TXN - 1) ? -6.f : -2.f;
    };
    if constexpr (UP) {
        asm volatile("" : "+v"(neg2));               // (one register for the kernel, not a move in front of every use)
#pragma unroll
        for (int rs = 0; rs < 2; ++rs) {
            raw_u[rs] = RAW_OFF + wave * RAW_WAVE + half * PLANE + ty_l * RAW_W + tx_l + rs * RAW_FLOATS;
            asm volatile("" : "+v"(raw_u[rs]));
        }
    }

    f32x16 acc[16];
    f32x16 zero16;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero16[r] = 0.f;

    // the input transform of plane j of raw slot rs into V slot vs, in three kinds of pieces (reads, adds, writes)
    float d[2][16], tq[2][16], tv[2][16];
#define WINO_T_READ(rs_, j_, r_)                                                                                        \
    {                                                                                                                   \
        const f32x2 lo_ = *((const volatile lds_f32x2_t*)0 + (raw_rd + ((rs_) * RAW_FLOATS + (j_) * RAW_PLANE + (r_) * RAW_W) / 2)); \
        const f32x2 hi_ = *((const volatile lds_f32x2_t*)0 + (raw_rd + ((rs_) * RAW_FLOATS + (j_) * RAW_PLANE + (r_) * RAW_W + 2) / 2)); \
        d[j_][4 * (r_) + 0] = lo_.x; d[j_][4 * (r_) + 1] = lo_.y; d[j_][4 * (r_) + 2] = hi_.x; d[j_][4 * (r_) + 3] = hi_.y; \
    }
    // B^T d over the rows (column c_): t0 = d0 - d2, t1 = d1 + d2, t2 = d2 - d1, t3 = d1 - d3
#define WINO_T_ROWS(j_, c_)                                                                                             \
    {                                                                                                                   \
        tq[j_][c_] = fsub_(d[j_][c_], d[j_][8 + (c_)]); tq[j_][4 + (c_)] = fadd_(d[j_][4 + (c_)], d[j_][8 + (c_)]);     \
        tq[j_][8 + (c_)] = fsub_(d[j_][8 + (c_)], d[j_][4 + (c_)]); tq[j_][12 + (c_)] = fsub_(d[j_][4 + (c_)], d[j_][12 + (c_)]); \
    }
    // (.) B over the columns (row i_); MOD: times the plane's modulation
#define WINO_T_SCALE(j_, i_, sc_)                                                                                       \
    { tv[j_][4 * (i_)] *= (sc_); tv[j_][4 * (i_) + 1] *= (sc_); tv[j_][4 * (i_) + 2] *= (sc_); tv[j_][4 * (i_) + 3] *= (sc_); }
#define WINO_T_COLS(j_, i_)                                                                                             \
    {                                                                                                                   \
        tv[j_][4 * (i_)] = fsub_(tq[j_][4 * (i_)], tq[j_][4 * (i_) + 2]); tv[j_][4 * (i_) + 1] = fadd_(tq[j_][4 * (i_) + 1], tq[j_][4 * (i_) + 2]); \
        tv[j_][4 * (i_) + 2] = fsub_(tq[j_][4 * (i_) + 2], tq[j_][4 * (i_) + 1]); tv[j_][4 * (i_) + 3] = fsub_(tq[j_][4 * (i_) + 1], tq[j_][4 * (i_) + 3]); \
    }
#define WINO_T_WRITE(vs_, j_, xi_)                                                                                      \
    *((volatile lds_f32_t*)0 + (v_wr + ((vs_) * V_FLOATS + ((xi_) * CI_T + 4 * (j_)) * NTILE))) = tv[j_][xi_];
    // LAB: the K loop's write, with its knock-outs (KO_TVALU: the raw value instead of the transformed one; KO_VWRITE: the value is kept alive, not written)
#define WINO_T_WRITE_LOOP(vs_, j_, xi_)                                                                                 \
    {                                                                                                                   \
        if constexpr (KO_VWRITE) { if constexpr (!KO_TVALU) asm volatile("" :: "v"(tv[j_][xi_])); }                     \
        else if constexpr (KO_TVALU) *((volatile lds_f32_t*)0 + (v_wr + ((vs_) * V_FLOATS + ((xi_) * CI_T + 4 * (j_)) * NTILE))) = d[j_][xi_]; \
        else WINO_T_WRITE(vs_, j_, xi_)                                                                                 \
    }
    // UP, the lane's pair of tiles (tv[e]: tile e of the pair, 0 the upper one) of its one plane: four raw rows of three (d[0]: 4 x 3); the
    // 1-D transform along each raw row (tq[0]: 4 x 4), ONCE for both tiles; then, per tile e_, along each of the 4 columns of its three rows
    // e_ .. e_ + 2 (tv[e_]: 4 x 4) -- the tile's own operations on its own operands: every V value has the bits of a lane-per-tile transform
#define WINO_U_READ(rs_, r_)                                                                                            \
    {                                                                                                                   \
        const volatile lds_f32_t* q_ = (const volatile lds_f32_t*)0 + (raw_u[rs_] + (r_) * RAW_W);                      \
        const f32x2 lo_ = *reinterpret_cast<const volatile lds_f32x2u_t*>(q_);                                          \
        d[0][3 * (r_) + 0] = lo_.x; d[0][3 * (r_) + 1] = lo_.y; d[0][3 * (r_) + 2] = q_[2];                             \
    }
#define WINO_U_H(r_, nk_)                                                                                               \
    up1d_(d[0][3 * (r_)], d[0][3 * (r_) + 1], d[0][3 * (r_) + 2], (nk_)[2], (nk_)[3], six,                              \
          tq[0][4 * (r_)], tq[0][4 * (r_) + 1], tq[0][4 * (r_) + 2], tq[0][4 * (r_) + 3]);
#define WINO_U_V(e_, c_, nk_)                                                                                           \
    up1d_(tq[0][4 * (e_) + (c_)], tq[0][4 * (e_) + 4 + (c_)], tq[0][4 * (e_) + 8 + (c_)], (e_) == 0 ? (nk_)[0] : neg2, (e_) == 0 ? neg2 : (nk_)[1], six, \
          tv[e_][c_], tv[e_][4 + (c_)], tv[e_][8 + (c_)], tv[e_][12 + (c_)]);
    // V[xi] of both tiles: TXN floats apart in [xi][ci][tile] -- two ds_write_b32 (the offsets of ds_write2_b32, 8 bits of dwords, do not
    // reach the 2 KB from one xi to the next: it would take an address per xi)
#define WINO_U_WRITE2(vs_, xi_, v0_, v1_)                                                                               \
    {                                                                                                                   \
        *((volatile lds_f32_t*)0 + (v_wr + ((vs_) * V_FLOATS + (xi_) * CI_T * NTILE))) = (v0_);                         \
        *((volatile lds_f32_t*)0 + (v_wr + ((vs_) * V_FLOATS + (xi_) * CI_T * NTILE + TXN))) = (v1_);                   \
    }
#define WINO_U_WRITE(vs_, xi_) WINO_U_WRITE2(vs_, xi_, tv[0][xi_], tv[1][xi_])
#define WINO_U_WRITE_LOOP(vs_, xi_)               /* LAB: as WINO_T_WRITE_LOOP */                                       \
    {                                                                                                                   \
        if constexpr (KO_VWRITE) { if constexpr (!KO_TVALU) asm volatile("" :: "v"(tv[0][xi_]), "v"(tv[1][xi_])); }     \
        else if constexpr (KO_TVALU) WINO_U_WRITE2(vs_, xi_, d[0][(xi_) % 12], d[0][((xi_) + 6) % 12])                  \
        else WINO_U_WRITE(vs_, xi_)                                                                                     \
    }

    if constexpr (RGB) {             // (published by the first chunk barrier, long before the first epilogue)
        if (tid < 3 * CO_T) smem[RGBW_OFF + tid] = (tid & (CO_T - 1)) < p.Cout ? p.rgb_w[(tid >> 6) * p.Cout + (tid & (CO_T - 1))] : 0.f;
    }
    const int n = p.cps;
    int reg = reg_begin + wk;
    if (reg >= reg_end) return;
    int b, y0, x0, kb, b_cur, kb_cur;   // b, kb: image / first chunk of the item whose operands are being requested; *_cur: of the item being computed
    region_coords(reg, b, y0, x0, kb);
    b_cur = b;
    kb_cur = kb;
    set_voff(voff, b, y0, x0);
    if constexpr (UP) set_nk(nk, y0, x0);
    // ---- first region: U_0, raw_0, raw_1 requested; raw_0 -> V_0 ----
    static_for<0, U_DMA>([&](auto k) { WINO_DMA_U(kb, 0, decltype(k)::value); });
    static_for<0, NG>([&](auto k) { WINO_DMA_RAW(voff[decltype(k)::value], kb, 0, decltype(k)::value); });
    static_for<0, NG>([&](auto k) { WINO_DMA_RAW(voff[decltype(k)::value], kb + 1, 1, decltype(k)::value); });
    __builtin_amdgcn_s_waitcnt(0x0f70);              // vmcnt(0): this wave's DMA has landed (its raw planes are its own)
    if constexpr (UP) {
        static_for<0, 4>([&](auto r) { WINO_U_READ(0, decltype(r)::value); });
        static_for<0, 4>([&](auto r) { WINO_U_H(decltype(r)::value, nk); });
        static_for<0, 8>([&](auto k) { WINO_U_V(decltype(k)::value & 1, decltype(k)::value >> 1, nk); });
        static_for<0, 16>([&](auto xi) { WINO_U_WRITE(0, decltype(xi)::value); });
        __builtin_amdgcn_sched_barrier(0);
    } else {
        static_for<0, 2>([&](auto j) {
            static_for<0, 4>([&](auto r) { WINO_T_READ(0, decltype(j)::value, decltype(r)::value); });
            static_for<0, 4>([&](auto c) { WINO_T_ROWS(decltype(j)::value, decltype(c)::value); });
            static_for<0, 4>([&](auto i) { WINO_T_COLS(decltype(j)::value, decltype(i)::value); });
            if constexpr (MOD) {
                const float sc0_ = p.in_scale[(size_t)b * p.Cin + kb * CI_T + wave + 4 * decltype(j)::value];
                static_for<0, 4>([&](auto i) { WINO_T_SCALE(decltype(j)::value, decltype(i)::value, sc0_); });
            }
            static_for<0, 16>([&](auto xi) { WINO_T_WRITE(0, decltype(j)::value, decltype(xi)::value); });
            __builtin_amdgcn_sched_barrier(0);       // one plane at a time: the register peak of this block decides what is spilled kernel-wide
        });
    }
    __syncthreads();

    // ---- main loop.  The chunks of ALL the workgroup's regions form one stream: chunk i of a region runs out of U / V slot
    // i & 1 (n is even: every region starts in slot 0); during it the weights of the stream's next chunk and the raw planes of
    // the one after that are requested, and the raw planes of the next chunk become its V -- across a region boundary these
    // belong to the NEXT region, so that a region's first operands are in LDS when its predecessor's epilogue ends ----
#ifndef SPK_WINO_PD
#define SPK_WINO_PD 4
#endif
    constexpr int PD = SPK_WINO_PD;                  // fragment prefetch distance in MFMAs (lab: -DSPK_WINO_PD=n)
    float fa[PD + 1], fb[PD + 1];
#define WINO_FRAG(slot_, s_, reg_)                                                                                      \
    {                                                                                                                   \
        constexpr int kk_ = (s_) >> 4, xi_ = (s_) & 15;                                                                 \
        fa[reg_] = *((const volatile lds_f32_t*)0 + (a_base + ((slot_) * U_FLOATS + (xi_ * CI_T + 2 * kk_) * CO_T)));   \
        fb[reg_] = *((const volatile lds_f32_t*)0 + (b_base + ((slot_) * V_FLOATS + (xi_ * CI_T + 2 * kk_) * NTILE)));  \
    }
    // nk_: UP -- the edge coefficients of the item the planes of chunk c1 belong to
    auto chunk_body = [&](auto slot_c, auto first_c, const int i, const float (&nk_)[4]) __attribute__((always_inline)) {
        constexpr int S = decltype(slot_c)::value, O = 1 - S;     // this chunk's slot; the other one receives the next chunk
        constexpr bool FIRST = decltype(first_c)::value;          // a region's first chunk: its first 16 MFMAs START the accumulators (C = 0)
        const int c1 = i + 1 < n ? kb_cur + i + 1 : kb;           // the stream's next chunk (weights: the same channel tile; past n: the next item's first)
        const int c2 = i + 2 >= n ? kb + i + 2 - n : kb_cur + i + 2;      // the chunk after it (past n: in the next item -- `voff` is that item's by then)
        float msc[2] = {1.f, 1.f};                                // MOD: the modulation of the two planes being transformed (chunk c1)
        if constexpr (MOD) {
            const float* ms_ = p.in_scale + (size_t)(i + 1 < n ? b_cur : b) * p.Cin + c1 * CI_T + wave;
            msc[0] = ms_[0];
            msc[1] = ms_[4];
        }
        static_for<0, PD>([&](auto s) { WINO_FRAG(S, decltype(s)::value, decltype(s)::value); });
        static_for<0, 64>([&](auto s_c) {
            constexpr int s = decltype(s_c)::value;
            if constexpr (s + PD < 64) { WINO_FRAG(S, s + PD, (s + PD) % (PD + 1)); }
            if constexpr (FIRST && s < 16) acc[s & 15] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s % (PD + 1)], fb[s % (PD + 1)], zero16, 0, 0, 0);
            else acc[s & 15] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s % (PD + 1)], fb[s % (PD + 1)], acc[s & 15], 0, 0, 0);
            // requests: the next chunk's weights into the other U slot, the raw planes of the chunk after it into THIS raw
            // slot (its planes became this chunk's V one chunk ago)
            if constexpr (s < U_DMA) {
                if constexpr (KO_UBARE) { WINO_DMA_U_BARE(c1, O, s); }
                else if constexpr (!KO_U) { WINO_DMA_U(c1, O, s); }
            } else if constexpr (s < U_DMA + NG && !KO_RAW) { WINO_DMA_RAW(voff[s - U_DMA], c2, S, s - U_DMA); }
            // raw slot O -> V slot O
            if constexpr (UP) {
                // the pair of tiles of the lane's plane, one piece (a row's reads, one up1d_ = 7 ops, V[xi] of both tiles) behind one MFMA:
                // reads 2-5, the four rows' first pass 8-11, the second pass 12-19 (per column: upper tile, lower tile), writes 20-35 in the
                // order the columns were finished (xi = c, 4 + c, 8 + c, 12 + c)
                if constexpr (s >= 2 && s < 6) { WINO_U_READ(O, s - 2); }
                if constexpr (!KO_TVALU && s >= 8 && s < 12) { WINO_U_H(s - 8, nk_); }
                if constexpr (!KO_TVALU && s >= 12 && s < 20) { WINO_U_V((s - 12) & 1, (s - 12) >> 1, nk_); }
                if constexpr (s >= 20 && s < 36) { WINO_U_WRITE_LOOP(O, 4 * ((s - 20) & 3) + ((s - 20) >> 2)); }
            } else {
                // plane 0: reads behind MFMAs 2-5, adds 8-15, writes 16-23; plane 1: 12-15, 24-31, 32-39
                static_for<0, 2>([&](auto j_c) {
                    constexpr int j = decltype(j_c)::value, tr = 2 + 10 * j, ta = 8 + 16 * j;
                    if constexpr (s >= tr && s < tr + 4) { WINO_T_READ(O, j, s - tr); }
                    if constexpr (!KO_TVALU && s >= ta && s < ta + 4) { WINO_T_ROWS(j, s - ta); }
                    if constexpr (!KO_TVALU && s >= ta + 4 && s < ta + 8) { WINO_T_COLS(j, s - ta - 4); if constexpr (MOD) { WINO_T_SCALE(j, s - ta - 4, msc[j]); } }
                    if constexpr (s >= ta + 8 && s < ta + 16) { WINO_T_WRITE_LOOP(O, j, 2 * (s - ta - 8)); WINO_T_WRITE_LOOP(O, j, 2 * (s - ta - 8) + 1); }
                });
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        __builtin_amdgcn_s_waitcnt(0x0f70);          // vmcnt(0): the requested weights and this wave's raw planes have landed
        __syncthreads();                             // the next chunk's V is complete, every wave is done with slot S
    };
    const bool f_bias = p.flags & SPK_EPI_BIAS, f_noise = p.flags & SPK_EPI_NOISE;
    const bool f_lrelu = p.flags & SPK_EPI_LRELU, f_style = p.flags & SPK_EPI_STYLE, f_accum = p.flags & SPK_EPI_ACCUM;
    const float osc = p.out_scale_dev ? p.out_scale * *p.out_scale_dev : p.out_scale;
    const float slope_ = f_lrelu ? p.slope : 1.f, gain_ = f_lrelu ? p.act_gain : 1.f;    // (no LeakyReLU: slope 1, gain 1)
    // epilogue geometry: lane = tile of the region (l32 + 32 wn) -> its 2 x 2 output pixels; accumulator register r of the lane's
    // half = channel row (r & 3) + 8 (r >> 2) + 4 half of the wave's 32
    const int tile = wn * 32 + l32, oy = 2 * (tile / TXN), ox = 2 * (tile % TXN);
    const int row_lane = wm * 32 + 4 * half;                              // + (r & 3) + 8 (r >> 2): row of the 64-channel tile
    float rgb_bo = 0.f;                                                   // RGB: the bias of the image channel this wave finishes
    if constexpr (RGB) { if (p.rgb_bias) rgb_bo = p.rgb_bias[min(wave, 2)]; }

    using F_ = std::false_type;
#ifdef SPK_WINO_LAB      // tools/lab_wino_phases.py: cycle stamps of one workgroup's second region, written over the output's first floats
    unsigned long long lab_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int lab_region = 0;
#define LAB_STAMP(k_) { if (lab_region == 1) lab_t[k_] = __builtin_readcyclecounter(); }
#else
#define LAB_STAMP(k_)
#endif
    for (;;) {
        LAB_STAMP(0)
#pragma unroll
        for (int xi = 0; xi < 16; ++xi)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[xi][r] = 0.f;
        // the region after this one (the last region repeats itself: loads nobody uses)
        const int cur_b = b, cur_y0 = y0, cur_x0 = x0;
        b_cur = b;
        kb_cur = kb;
        // everything the epilogue reads from global memory is requested NOW and lands behind the region's MFMAs: the noise of
        // this thread's four pixels, and (wave 0: one channel per lane) the channel's bias / noise weight / style pair, which
        // reach the other waves through a 1 KB LDS table -- no load latency between the last MFMA and the stores
        const size_t pix = (size_t)(cur_y0 + oy) * p.W + (cur_x0 + ox);          // this lane's tile: pixels (pix, pix + 1), (pix + W, pix + W + 1)
        f32x2 nz0, nz1;
        nz0.x = nz0.y = nz1.x = nz1.y = 0.f;
        if (f_noise) {
            nz0 = *reinterpret_cast<const f32x2*>(p.noise + (size_t)cur_b * HW + pix);
            nz1 = *reinterpret_cast<const f32x2*>(p.noise + (size_t)cur_b * HW + pix + p.W);
        }
        // the operand table of the epilogue: thread t fetches operand t & 3 (bias, noise weight, style scale + 1, style shift) of channel
        // t >> 2, or its neutral value.  (From an opaque copy of the thread index, per region: the operand's 64-bit address and its
        // companions are rebuilt by a dozen vector ops instead of living in five registers through the K loop.)
        int prm_t = tid;
        asm volatile("" : "+v"(prm_t));
        const int prm_which = prm_t & 3, prm_c = co0 + (prm_t >> 2);
        const bool prm_on = prm_c < p.Cout && (prm_which == 0 ? f_bias : (prm_which == 1 ? f_noise : f_style));
        const float* const prm_src = (prm_which == 0 ? p.bias : (prm_which == 1 ? p.noise_w : p.style + (prm_which == 3 ? p.Cout : 0))) + prm_c;
        // The loaded value is not touched before the epilogue: an instruction on it here would wait for vmcnt(0), that is for every
        // store of the previous region's epilogue (900 cycles in front of the K loop, measured with tools/lab_wino_phases.py).
        float prm_raw = 0.f;                             // absent: + 0, + 0 * noise, * (0 + 1), + 0
        if (prm_on) prm_raw = prm_src[prm_which >= 2 ? (size_t)cur_b * p.style_stride : 0];      // ONE load per thread, no branch per operand kind
        float dem = 1.f;
        if constexpr (MOD) {
            if (p.out_scale_bc && tid < CO_T && co0 + tid < p.Cout) dem = p.out_scale_bc[(size_t)cur_b * p.Cout + co0 + tid];
        }
        const bool more = reg + wpx < reg_end;
        if (more) {
            reg += wpx;
            region_coords(reg, b, y0, x0, kb);
        }
        set_voff(voff_next, b, y0, x0);
        if constexpr (UP) {              // (this item's coefficients from its own coordinates; the next item's beside its offsets)
            set_nk(nk, cur_y0, cur_x0);
            set_nk(nkn, y0, x0);
        }

        // (host: n is even.)  From the last pair of chunks on, every raw request belongs to the next region: its offsets move in,
        // once, by selects (no branch in the body).
        // ONE loop body, entered once per region: the 256 accumulator registers never cross a control-flow merge other than the
        // loop header and stay in the AGPR file.  (Peeling the first pair of chunks so that its MFMAs start from C = 0 -- no
        // zero fill -- was tried: the compiler then copies all accumulators to VGPRs at the loop exit and spills.)
        LAB_STAMP(1)
        for (int i = 0; i < n; i += 2) {
            const bool last_pair = i + 2 >= n;
            // Plain and modulated forms: a scalar BRANCH around 11 moves instead of 11 selects per pair of chunks (5.5 vector ops per
            // chunk that an f32 MFMA does not overlap; the empty asm keeps the compiler from turning it back into selects).  The accumulators
            // cross this merge untouched.  UP has 4 offsets and keeps the selects: with the branch its loop slowed down by a sixth.
            if constexpr (UP) {
#pragma unroll
                for (int k = 0; k < NG; ++k) voff[k] = last_pair ? voff_next[k] : voff[k];
            } else if (last_pair) {
                asm volatile("" ::: "memory");
#pragma unroll
                for (int k = 0; k < NG; ++k) voff[k] = voff_next[k];
            }
            chunk_body(std::integral_constant<int, 0>{}, F_{}, i, nk);
            if constexpr (UP) {          // a region's last chunk transforms the first planes of the NEXT item
                float nk2[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) nk2[k] = last_pair ? nkn[k] : nk[k];
                chunk_body(std::integral_constant<int, 1>{}, F_{}, i + 1, nk2);
            } else {
                chunk_body(std::integral_constant<int, 1>{}, F_{}, i + 1, nk);
            }
        }

        // ---- epilogue, in registers: output transform Y = A^T M A (A^T = [1,1,1,0; 0,1,-1,-1]) of one channel row at a time, then the
        // f32 kernel's epilogue element for element (out_scale, bias, noise, LeakyReLU, [y_pre], style, [accumulate]) on the lane's
        // 2 x 2 pixels, and two 8-byte stores: lanes 0-15 / 16-31 of a half-wave cover 32 consecutive pixels of two image rows --
        // whole 128-byte lines -- so the block needs no trip through LDS (which would also collide with the next region's operands).
        // Every stage runs unconditionally; an absent one has its neutral operand in the table.
        LAB_STAMP(2)
        smem[PRM_OFF + tid] = (tid & 3) == 2 ? prm_raw + 1.f : prm_raw;       // the table holds style scale + 1
        if constexpr (MOD) { if (tid < CO_T) smem[DEM_OFF + tid] = dem; }
        lds_barrier();
        unsigned hw_ = (unsigned)HW;                 // (opaque per region: the 16 rows' channel offsets must not be hoisted out of the region
        asm volatile("" : "+s"(hw_));                //  loop as 32 live registers)
        const size_t o0 = ((size_t)cur_b * p.Cy + (size_t)grp * p.Cout) * hw_ + pix + (size_t)(kb_cur / p.cps) * p.slice_floats;
        // LEAN: a store's address = wave-uniform row base (64 bits, scalar ALU) + this lane's byte offset within five channel planes
        // (32 bits, fixed for the region; host: 20 H W < 2^32)
        const size_t hw_bytes = (size_t)hw_ * 4, w_bytes = (size_t)p.W * 4;
        char* const y_rows = reinterpret_cast<char*>(p.y + ((size_t)cur_b * p.Cy + (size_t)grp * p.Cout + co0 + wm * 32) * hw_ +
                                                     (size_t)(kb_cur / p.cps) * p.slice_floats);
        const unsigned y_lane = ((unsigned)(4 * half) * hw_ + (unsigned)pix) * 4u;
        LAB_STAMP(3)
        // The accumulators are read out of the AGPR file one element at a time, by hand (v_accvgpr_read_b32 with an "a" operand):
        // left to the compiler, the first use of element r of a tile copies the whole 16-register tile to VGPRs, a row touches all
        // 16 tiles, and 256 VGPRs of copies push everything else that is alive into scratch -- whose reloads then queue, in
        // vmcnt order, behind the epilogue's own stores (25 000 cycles per region, measured).
        // A row's 16 reads and the 24 adds of Y = A^T M A are ONE asm statement (as up1d_): between dependent one-instruction statements
        // the compiler puts an s_nop or a v_mov.  Sums in the order of the scalar form: s0_i = (m0 + m1) + m2, s1_i = (m1 - m2) - m3 over
        // the tiles 4 i .. 4 i + 3, then top = (s_0 + s_1) + s_2, bot = (s_1 - s_2) - s_3.
#define WINO_ROW4(a_, b_, m0_, m1_, m2_, m3_)                                                                           \
    "v_accvgpr_read_b32 " a_ ", " m0_ "\n\tv_accvgpr_read_b32 " b_ ", " m1_ "\n\tv_accvgpr_read_b32 %4, " m2_ "\n\tv_accvgpr_read_b32 %5, " m3_ "\n\t" \
    "v_add_f32 " a_ ", " a_ ", " b_ "\n\tv_sub_f32 " b_ ", " b_ ", %4\n\tv_add_f32 " a_ ", " a_ ", %4\n\tv_sub_f32 " b_ ", " b_ ", %5\n\t"
#define WINO_ROW(r_, top_, bot_)                                                                                        \
    {                                                                                                                   \
        float tx_, ty_, bx_, by_, t0_, t1_, t2_, t3_;                                                                   \
        asm volatile(WINO_ROW4("%0", "%1", "%8", "%9", "%10", "%11")                                                    \
                     WINO_ROW4("%2", "%3", "%12", "%13", "%14", "%15")                                                  \
                     "v_add_f32 %0, %0, %2\n\tv_add_f32 %1, %1, %3\n\t"                                                \
                     WINO_ROW4("%6", "%7", "%16", "%17", "%18", "%19")                                                  \
                     "v_add_f32 %0, %0, %6\n\tv_sub_f32 %2, %2, %6\n\tv_add_f32 %1, %1, %7\n\tv_sub_f32 %3, %3, %7\n\t" \
                     WINO_ROW4("%6", "%7", "%20", "%21", "%22", "%23")                                                  \
                     "v_sub_f32 %2, %2, %6\n\tv_sub_f32 %3, %3, %7"                                                    \
                     : "=&v"(tx_), "=&v"(ty_), "=&v"(bx_), "=&v"(by_), "=&v"(t0_), "=&v"(t1_), "=&v"(t2_), "=&v"(t3_)    \
                     : "a"(acc[0][r_]), "a"(acc[1][r_]), "a"(acc[2][r_]), "a"(acc[3][r_]), "a"(acc[4][r_]), "a"(acc[5][r_]), \
                       "a"(acc[6][r_]), "a"(acc[7][r_]), "a"(acc[8][r_]), "a"(acc[9][r_]), "a"(acc[10][r_]), "a"(acc[11][r_]), \
                       "a"(acc[12][r_]), "a"(acc[13][r_]), "a"(acc[14][r_]), "a"(acc[15][r_]));                         \
        (top_).x = tx_; (top_).y = ty_; (bot_).x = bx_; (bot_).y = by_;                                                 \
    }
        float rgb[3][4];                                 // RGB: this lane's share (its 16 channel rows) of its tile's 2 x 2 pixels x 3 channels
#pragma unroll
        for (int o = 0; o < 3; ++o)
#pragma unroll
            for (int q = 0; q < 4; ++q) rgb[o][q] = 0.f;
        static_for<0, 16>([&](auto r_c) {
            constexpr int r = decltype(r_c)::value;
            const int row = row_lane + (r & 3) + 8 * (r >> 2);
            const float4 q_ = *reinterpret_cast<const float4*>(smem + PRM_OFF + 4 * row);
            f32x2 top, bot;
            WINO_ROW(r, top, bot)
            float osc_r = osc;
            if constexpr (MOD) osc_r = osc * smem[DEM_OFF + row];
            top.x = top.x * osc_r + q_.x; top.y = top.y * osc_r + q_.x; bot.x = bot.x * osc_r + q_.x; bot.y = bot.y * osc_r + q_.x;
            top.x += q_.y * nz0.x; top.y += q_.y * nz0.y; bot.x += q_.y * nz1.x; bot.y += q_.y * nz1.y;
            if constexpr (EPI != GENERIC) {
                // max(x, x slope) gain: what the select gives for every non-NaN x, +-0 included, while 0 < slope <= 1 (host)
                top.x = __builtin_fmaxf(top.x, top.x * slope_) * gain_; top.y = __builtin_fmaxf(top.y, top.y * slope_) * gain_;
                bot.x = __builtin_fmaxf(bot.x, bot.x * slope_) * gain_; bot.y = __builtin_fmaxf(bot.y, bot.y * slope_) * gain_;
                top.x = top.x * q_.z + q_.w; top.y = top.y * q_.z + q_.w; bot.x = bot.x * q_.z + q_.w; bot.y = bot.y * q_.z + q_.w;
                if constexpr (RGB) {
#pragma unroll
                    for (int o = 0; o < 3; ++o) {
                        const float w_ = smem[RGBW_OFF + o * CO_T + row];      // (rows past Cout: 0)
                        rgb[o][0] += w_ * top.x; rgb[o][1] += w_ * top.y; rgb[o][2] += w_ * bot.x; rgb[o][3] += w_ * bot.y;
                    }
                }
                if constexpr (EPI == LEAN) {
                    char* const yr = y_rows + (size_t)((r & 3) + 8 * (r >> 2)) * hw_bytes;       // the channel row's step: scalar
#ifdef SPK_WINO_NOSTORE   // LAB knock-out: everything but the stores themselves
                    if (top.x == 12345.678f)
#endif
                    {
                        *reinterpret_cast<f32x2*>(yr + y_lane) = top;
                        *reinterpret_cast<f32x2*>(yr + w_bytes + y_lane) = bot;
                    }
                }
                if constexpr (RGB) __builtin_amdgcn_sched_barrier(0);
            } else {
                top.x = (top.x > 0.f ? top.x : top.x * slope_) * gain_; top.y = (top.y > 0.f ? top.y : top.y * slope_) * gain_;
                bot.x = (bot.x > 0.f ? bot.x : bot.x * slope_) * gain_; bot.y = (bot.y > 0.f ? bot.y : bot.y * slope_) * gain_;
                const int co = co0 + row;
                if constexpr (RGB) {                     // (no y_pre / accumulate with a fused toRGB: host)
                    top.x = top.x * q_.z + q_.w; top.y = top.y * q_.z + q_.w; bot.x = bot.x * q_.z + q_.w; bot.y = bot.y * q_.z + q_.w;
#pragma unroll
                    for (int o = 0; o < 3; ++o) {
                        const float w_ = smem[RGBW_OFF + o * CO_T + row];      // (rows past Cout: 0)
                        rgb[o][0] += w_ * top.x; rgb[o][1] += w_ * top.y; rgb[o][2] += w_ * bot.x; rgb[o][3] += w_ * bot.y;
                    }
                    if (p.y && co < p.Cout) {        // (the lean rows' address: scalar row base + 32-bit lane offset)
                        char* const yr = y_rows + (size_t)((r & 3) + 8 * (r >> 2)) * hw_bytes;
                        *reinterpret_cast<f32x2*>(yr + y_lane) = top;
                        *reinterpret_cast<f32x2*>(yr + w_bytes + y_lane) = bot;
                    }
                    __builtin_amdgcn_sched_barrier(0);       // one channel row at a time: hoisted table reads of 16 rows would not fit the registers
                } else if (co < p.Cout) {
                    const size_t off = o0 + (size_t)co * hw_;
                    if (p.y_pre) {
                        *reinterpret_cast<f32x2*>(p.y_pre + off) = top;
                        *reinterpret_cast<f32x2*>(p.y_pre + off + p.W) = bot;
                    }
                    top.x = top.x * q_.z + q_.w; top.y = top.y * q_.z + q_.w; bot.x = bot.x * q_.z + q_.w; bot.y = bot.y * q_.z + q_.w;
                    if (f_accum) {
                        const f32x2 o_t = *reinterpret_cast<const f32x2*>(p.y + off), o_b = *reinterpret_cast<const f32x2*>(p.y + off + p.W);
                        top.x += o_t.x; top.y += o_t.y; bot.x += o_b.x; bot.y += o_b.y;
                    }
#ifdef SPK_WINO_NOSTORE   // LAB knock-out: everything but the stores themselves
                    if (top.x == 12345.678f)
#endif
                    {
                        *reinterpret_cast<f32x2*>(p.y + off) = top;
                        *reinterpret_cast<f32x2*>(p.y + off + p.W) = bot;
                    }
                }
            }
        });
#undef WINO_ROW
#undef WINO_ROW4
        if constexpr (RGB) {
            // the four channel groups of a tile: (wm, half) -> LDS [group][tile][3][4], summed in group order by thread (tile, channel)
            float* part = smem + RGB_PART_OFF + ((wm * 2 + half) * NTILE + tile) * 12;
#pragma unroll
            for (int o = 0; o < 3; ++o) *reinterpret_cast<float4*>(part + 4 * o) = make_float4(rgb[o][0], rgb[o][1], rgb[o][2], rgb[o][3]);
            lds_barrier();
            {
                // wave o finishes image channel o; wave 3 repeats channel 2 (the same values to the same addresses) rather than
                // stand behind a guard, which would be the only branch of the epilogue
                const int o = min(wave, 2), t = lane;
                const float* ps = smem + RGB_PART_OFF + t * 12 + 4 * o;
                float4 v = *reinterpret_cast<const float4*>(ps);
#pragma unroll
                for (int g = 1; g < 4; ++g) {
                    const float4 u = *reinterpret_cast<const float4*>(ps + g * NTILE * 12);
                    v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
                }
                // address = scalar base (image, channel, region origin) + the tile's 32-bit byte offset within the plane
                char* const yo = reinterpret_cast<char*>(p.rgb_y + ((size_t)cur_b * 3 + o) * hw_ + (size_t)cur_y0 * p.W + cur_x0);
                const unsigned t_off = ((unsigned)(2 * (t / TXN)) * (unsigned)p.W + (unsigned)(2 * (t % TXN))) * 4u;
                f32x2 a_, b_;
                a_.x = v.x + rgb_bo; a_.y = v.y + rgb_bo; b_.x = v.z + rgb_bo; b_.y = v.w + rgb_bo;
                *reinterpret_cast<f32x2*>(yo + t_off) = a_;
                *reinterpret_cast<f32x2*>(yo + (size_t)p.W * 4 + t_off) = b_;
            }
        }
        LAB_STAMP(4)
        lds_barrier();                               // (the table has been read: the next region may rewrite it)
#ifdef SPK_WINO_LAB
        if (lab_region == 1 && blockIdx.x == 8 && blockIdx.y == 0 && tid == 0)
            for (int k = 0; k < 5; ++k) p.y[k] = (float)(long long)(lab_t[k] - lab_t[0]);
        ++lab_region;
#endif
        if (!more) break;
    }
#undef WINO_FRAG
#undef WINO_T_WRITE_LOOP
#undef WINO_T_WRITE
#undef WINO_U_WRITE_LOOP
#undef WINO_U_WRITE
#undef WINO_U_WRITE2
#undef WINO_U_V
#undef WINO_U_H
#undef WINO_U_READ
#undef WINO_T_COLS
#undef WINO_T_SCALE
#undef WINO_T_ROWS
#undef WINO_T_READ
#undef WINO_DMA_U_BARE
#undef WINO_DMA_U
#undef WINO_DMA_RAW
#undef WINO_EDGE
}

}  // namespace spkwino

using namespace spkwino;

extern "C" {

int64_t spk_conv2d_packed_bytes_wino(int Cin, int Cout) {
    if (Cin <= 0 || Cout <= 0) return -1;
    return (int64_t)spk::ceil_div(Cout, CO_T) * spk::ceil_div(Cin, CI_T) * U_FLOATS * 4;
}

int spk_conv2d_pack_weights_wino(const float* w, float* w_packed, int Cin, int Cout, int transpose_flip, void* stream) {
    SPK_REQUIRE(w && w_packed && Cin > 0 && Cout > 0 && (transpose_flip == 0 || transpose_flip == 1), "pack_weights_wino: bad arguments");
    const int opCin = transpose_flip ? Cout : Cin, opCout = transpose_flip ? Cin : Cout;
    const int n_chunks = spk::ceil_div(opCin, CI_T);
    const long long total = (long long)spk::ceil_div(opCout, CO_T) * n_chunks * U_FLOATS;
    hipLaunchKernelGGL(pack_wino_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, w_packed, Cin, Cout,
                       opCin, opCout, transpose_flip, n_chunks, total);
    return spk::check_launch("pack_wino_kernel");
}

static int wino_shape(int H, int W) {         // -1: no region shape tiles the image
    if (H % region_h(WIDE) == 0 && W % region_w(WIDE) == 0) return WIDE;
    if (H % region_h(SQUARE) == 0 && W % region_w(SQUARE) == 0) return SQUARE;
    return -1;
}

int spk_conv2d_pack_weights_wino_list(const float* const* w, float* const* w_packed, const int* Cin, const int* Cout, const int* transpose_flip,
                                      int n, void* stream) {
    SPK_REQUIRE(w && w_packed && Cin && Cout && transpose_flip && n > 0 && n <= SPK_WINO_PACK_MAX, "pack_weights_wino_list: 1..%d items", SPK_WINO_PACK_MAX);
    PackWinoList a;
    long long most = 0;
    for (int i = 0; i < n; ++i) {
        SPK_REQUIRE(w[i] && w_packed[i] && Cin[i] > 0 && Cout[i] > 0 && (transpose_flip[i] == 0 || transpose_flip[i] == 1), "pack_weights_wino_list: item %d", i);
        a.w[i] = w[i]; a.out[i] = w_packed[i]; a.Cin[i] = Cin[i]; a.Cout[i] = Cout[i]; a.tf[i] = transpose_flip[i];
        most = std::max<long long>(most, (transpose_flip[i] ? spk_conv2d_packed_bytes_wino(Cout[i], Cin[i]) : spk_conv2d_packed_bytes_wino(Cin[i], Cout[i])) / 4);
    }
    dim3 grid((unsigned)std::min<long long>((most + 255) / 256, 2048), (unsigned)n);
    hipLaunchKernelGGL(pack_wino_list_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    return spk::check_launch("pack_wino_list_kernel");
}

static int wino_geometry_ok(int B, int Cin, int Cout, int H, int W) {        // everything but the size of the tensor the gathers read
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return 0;
    if (wino_shape(H, W) < 0) return 0;     // whole 32 x 8 or 16 x 16 pixel regions
    if (Cin % (2 * CI_T)) return 0; // whole chunks (the gathers of a ragged last chunk would reach past the tensor), an even number of them
    return 1;
}

int spk_conv2d_wino_supported(int B, int Cin, int Cout, int H, int W) {
    if (!wino_geometry_ok(B, Cin, Cout, H, W)) return 0;
    if ((long long)B * Cin * H * W * 4 >= (1ll << 31)) return 0;          // 32-bit buffer offsets, bit 31 = "out of range"
    return 1;
}

// SPK_CONV_WINOGRAD | SPK_CONV_UPSAMPLE2X: OUTPUT shape H x W of conv3x3(bilinear_x2(x)), x = [B, Cin, H/2, W/2]
int spk_conv2d_wino_up_supported(int B, int Cin, int Cout, int H, int W) {
    if (!wino_geometry_ok(B, Cin, Cout, H, W) || (H & 1) || (W & 1)) return 0;
    if ((long long)B * Cin * (H / 2) * (W / 2) * 4 >= (1ll << 31)) return 0;      // the 2 GB limit is the INPUT tensor's: the gathers read it
    return 1;
}

// Slices of the channel contraction (split-K) for a problem with too few (region, channel tile) pairs to fill the CUs: the smallest
// power of two that brings the grid to >= 3/4 of a workgroup per CU while a slice keeps >= 4 chunks (an even number); `want` > 0: that
// many if the chunk count allows.  1 = no split.  A split launch writes partial sums [ksplit][B][Cout][H][W] into the workspace and
// the direct kernels' split-K finisher applies the epilogue.
int spk_conv2d_wino_ksplit(int want, int B, int Cin, int Cout, int H, int W) {
    if (!wino_geometry_ok(B, Cin, Cout, H, W)) return -1;      // (the byte limit is the launch's: it knows which tensor the gathers read)
    const int shape = wino_shape(H, W), n_chunks = Cin / CI_T;
    const long long pairs = (long long)B * (H / region_h(shape)) * (W / region_w(shape)) * spk::ceil_div(Cout, CO_T);
    auto ok = [&](int ks) { return ks >= 1 && n_chunks % (2 * ks) == 0 && n_chunks / ks >= 4; };
    if (want > 0) {
        int ks = want;
        while (ks > 1 && !ok(ks)) --ks;
        return ks;
    }
    int ks = 1;
    while (pairs * ks < 192 && ok(2 * ks)) ks *= 2;
    return ks;
}

int64_t spk_conv2d_wino_workspace_bytes(int ksplit, int B, int Cin, int Cout, int H, int W) {
    const int ks = spk_conv2d_wino_ksplit(ksplit, B, Cin, Cout, H, W);
    if (ks < 0) return -1;
    return ks > 1 ? (int64_t)ks * B * Cout * H * W * 4 : 0;
}

}  // extern "C"

// The kernel choice of a Winograd launch as integers, and what its grid is derived from (the grid itself depends on the device)
struct WinoKernel {
    bool mod, rgb, up;
    int shape, epi_form;
    long long n_items;
    int co_tiles;
};

// every requirement and decision of a SPK_CONV_WINOGRAD launch, without a HIP call; `a`: the kernel's argument block
static int plan_args(const spk_conv2d_desc* d, spkconv::SlicedPlan& p, Args& a, WinoKernel& k) {
    using spkconv::aligned16;
    SPK_REQUIRE(d && d->x && d->w_packed, "conv2d winograd: null pointer");
    SPK_REQUIRE(d->kh == 3 && d->kw == 3 && d->stride == 1, "conv2d winograd: 3x3 stride-1 kernels only");
    const spkconv::Groups q = spkconv::groups_of(*d);
    const int G = q.G, gin = q.gin, Cx = (int)q.Cx, Cy = (int)q.Cy;
    const bool up = d->flags & SPK_CONV_UPSAMPLE2X;
    SPK_REQUIRE(!up || (G == 1 && !(d->flags & (SPK_CONV_IN_BATCH_SCALE | SPK_CONV_UP_FIR1331))),
                "conv2d winograd: SPK_CONV_UPSAMPLE2X is the bilinear x2 of a plain launch (no IN_BATCH_SCALE, no UP_FIR1331, no groups): "
                "pass the x2 image (spk_upsample2x_fwd)");
    SPK_REQUIRE(G == 1 || !(d->flags & ~(SPK_CONV_WINOGRAD | SPK_EPI_ACCUM)), "conv2d winograd: a grouped launch takes SPK_EPI_ACCUM only (the encoders' "
                "data gradients)");
    SPK_REQUIRE(G == 1 || gin >= d->Cin, "conv2d winograd: groups read disjoint channels");
    const unsigned epi = SPK_EPI_BIAS | SPK_EPI_NOISE | SPK_EPI_LRELU | SPK_EPI_STYLE | SPK_EPI_ACCUM;
    const unsigned allowed = SPK_CONV_WINOGRAD | epi | SPK_CONV_IN_BATCH_SCALE | SPK_EPI_TORGB | SPK_CONV_UPSAMPLE2X;
    SPK_REQUIRE(!(d->flags & ~allowed) && !d->stats && !d->accum_half,
                "conv2d winograd: plain, bilinear x2 or batch-scaled input; epilogue flags bias, noise, lrelu, style, accum, torgb");
    const bool mod = d->flags & SPK_CONV_IN_BATCH_SCALE, rgb = d->flags & SPK_EPI_TORGB;
    SPK_REQUIRE(d->y || rgb, "conv2d winograd: null pointer");
    if (rgb)
        SPK_REQUIRE(d->rgb_w && d->rgb_y && d->rgb_channels == 3 && d->Cout <= CO_T && !mod && !d->y_pre && !(d->flags & SPK_EPI_ACCUM) &&
                        (reinterpret_cast<uintptr_t>(d->rgb_y) & 7) == 0,
                    "conv2d winograd: SPK_EPI_TORGB needs rgb_w [3][Cout], rgb_y [B,3,H,W], Cout <= 64 (one channel tile), no y_pre / accumulate / modulation");
    SPK_REQUIRE(!mod || d->in_scale, "conv2d winograd: IN_BATCH_SCALE without in_scale[B,Cin]");
    SPK_REQUIRE(!d->out_scale_bc || mod, "conv2d winograd: out_scale_bc (demodulation) goes with SPK_CONV_IN_BATCH_SCALE");
    if (up)
        SPK_REQUIRE(d->H == 2 * d->Hin && d->W == 2 * d->Win && spk_conv2d_wino_up_supported(d->B, d->Cin, d->Cout, d->H, d->W),
                    "conv2d winograd: SPK_CONV_UPSAMPLE2X needs an output of twice the input size, %dx%d -> %dx%d", d->Hin, d->Win, d->H, d->W);
    else
        SPK_REQUIRE(d->H == d->Hin && d->W == d->Win, "conv2d winograd: output size must equal the input size");
    SPK_REQUIRE(wino_geometry_ok(d->B, d->Cin, d->Cout, d->H, d->W) && (long long)d->B * Cx * d->Hin * d->Win * 4 < (1ll << 31),
                "conv2d winograd: %dx%d is not a whole number of 32 x 8 or 16 x 16 regions (or the input exceeds 2 GB)", d->H, d->W);
    SPK_REQUIRE(!(d->flags & SPK_EPI_BIAS) || d->bias, "conv2d winograd: SPK_EPI_BIAS without bias");
    SPK_REQUIRE(!(d->flags & SPK_EPI_NOISE) || (d->noise && d->noise_w), "conv2d winograd: SPK_EPI_NOISE without noise");
    SPK_REQUIRE(!(d->flags & SPK_EPI_STYLE) || d->style, "conv2d winograd: SPK_EPI_STYLE without style");
    SPK_REQUIRE(aligned16(d->w_packed) && aligned16(d->y) && aligned16(d->y_pre) && aligned16(d->noise) && (reinterpret_cast<uintptr_t>(d->x) & 3) == 0,
                "conv2d winograd: tensors must be 16-byte aligned");
    const int shape = wino_shape(d->H, d->W);
    const int ks = spk_conv2d_wino_ksplit(d->ksplit, d->B, d->Cin, Cy, d->H, d->W);       // (the groups' channel tiles count towards the grid)
    const size_t out_floats = (size_t)d->B * Cy * d->H * d->W;
    if (ks > 1)
        SPK_REQUIRE(d->workspace && aligned16(d->workspace) && d->workspace_bytes >= (int64_t)ks * (int64_t)out_floats * 4,
                    "conv2d winograd: %d contraction slices need a workspace of %lld bytes (spk_conv2d_wino_workspace_bytes)", ks,
                    (long long)ks * (long long)out_floats * 4);
    a.x = d->x; a.wp = d->w_packed; a.bias = d->bias; a.noise_w = d->noise_w; a.noise = d->noise; a.style = d->style;
    a.y = d->y; a.y_pre = d->y_pre; a.out_scale_dev = d->out_scale_dev;
    a.in_scale = mod ? d->in_scale : nullptr; a.out_scale_bc = d->out_scale_bc;
    a.rgb_w = d->rgb_w; a.rgb_bias = d->rgb_bias; a.rgb_y = d->rgb_y;
    a.B = d->B; a.Cin = d->Cin; a.Cout = d->Cout; a.H = d->H; a.W = d->W;
    a.G = G; a.gin = gin; a.Cx = Cx; a.Cy = Cy; a.co_tiles_g = spk::ceil_div(d->Cout, CO_T);
    a.regions_x = d->W / region_w(shape); a.regions_y = d->H / region_h(shape);
    a.n_chunks = spk::ceil_div(d->Cin, CI_T);
    a.ksplit = ks; a.cps = a.n_chunks / ks; a.slice_floats = 0;
    a.style_stride = d->style_stride; a.flags = d->flags;
    a.x_bytes = (unsigned)((long long)d->B * Cx * d->Hin * d->Win * 4);
    const float up_scale = up ? 0.0625f : 1.f;      // UP: the input transform yields 16 V (up1d_)
    a.slope = d->lrelu_slope; a.out_scale = d->out_scale * up_scale; a.act_gain = spkconv::act_gain_of(*d);
    SPK_REQUIRE(!rgb || ks == 1, "conv2d winograd: SPK_EPI_TORGB with a sliced contraction (%d slices): pass ksplit = 1 or run the 1x1 separately", ks);
    if (ks > 1) {       // partial sums, raw: the whole epilogue (and the demodulation) belongs to the finisher
        a.y = static_cast<float*>(d->workspace); a.y_pre = nullptr; a.out_scale_dev = nullptr; a.out_scale_bc = nullptr;
        a.flags = d->flags & ~epi; a.out_scale = 1.f; a.slice_floats = out_floats;
    }
    p.config = -1;
    p.finish.args = spkconv::finisher_args(*d, q, d->flags & epi, d->out_scale * up_scale);
    p.finish.ws = static_cast<const float*>(d->workspace);
    p.finish.ksplit = ks;
    // the rows' form: LEAN for whole channel tiles without y_pre / accumulate (every inference launch of the decoder, and the sliced
    // launches' raw partial sums); everything else -- and a slope outside (0, 1], which the lean rows' max() does not cover -- GENERIC
    const bool lrelu_ok = !(a.flags & SPK_EPI_LRELU) || (a.slope > 0.f && a.slope <= 1.f);
    const bool lean_ok = !mod && lrelu_ok && !a.y_pre && !(a.flags & SPK_EPI_ACCUM) && 20ll * d->H * d->W < (1ll << 32);
    k.mod = mod; k.rgb = rgb; k.up = up; k.shape = shape;
    k.epi_form = !lean_ok ? GENERIC : rgb ? (!a.y ? LEAN_NOSTORE : d->Cout == CO_T ? LEAN : GENERIC) : (d->Cout % CO_T == 0 ? LEAN : GENERIC);
    k.n_items = (long long)a.regions_x * a.regions_y * d->B * ks;
    SPK_REQUIRE(k.n_items < (1ll << 31), "conv2d winograd: grid too large");
    k.co_tiles = G * spk::ceil_div(d->Cout, CO_T);
    return SPK_OK;
}

static const void* wino_kernel_of(const WinoKernel& k) {
    const int shape = k.shape, epi_form = k.epi_form;
    const auto pick = [&](auto rgb_c, auto up_c) -> void (*)(const Args) {
        constexpr bool R = decltype(rgb_c)::value, U = decltype(up_c)::value;
        if constexpr (R) {
            if (epi_form == LEAN_NOSTORE) return shape == SQUARE ? &wino_kernel<false, SQUARE, R, U, LEAN_NOSTORE> : &wino_kernel<false, WIDE, R, U, LEAN_NOSTORE>;
        }
        if (epi_form == LEAN) return shape == SQUARE ? &wino_kernel<false, SQUARE, R, U, LEAN> : &wino_kernel<false, WIDE, R, U, LEAN>;
        return shape == SQUARE ? &wino_kernel<false, SQUARE, R, U> : &wino_kernel<false, WIDE, R, U>;
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    void (*kern)(const Args) = k.mod ? (shape == SQUARE ? &wino_kernel<true, SQUARE> : &wino_kernel<true, WIDE>)
                               : k.rgb ? (k.up ? pick(T_{}, T_{}) : pick(T_{}, F_{})) : (k.up ? pick(F_{}, T_{}) : pick(F_{}, F_{}));
    return reinterpret_cast<const void*>(kern);
}

// gridDim.x of a launch, for the launch and for spk_conv2d_wino_form: persistent workgroups, one per CU over all channel tiles, a
// multiple of 8 per channel tile (the XCD shares), at most one per item
static long long wino_grid_x(int n_cu, int co_tiles, long long items) {
    return std::min(std::max(8ll, ((long long)n_cu / co_tiles) / 8 * 8), (items + 7) / 8 * 8);
}

int spkconv::plan_wino(const spk_conv2d_desc* d, SlicedPlan& p) {
    Args a;
    WinoKernel k;
    return plan_args(d, p, a, k);
}

extern "C" {

// entered from spk_conv2d_fwd when desc->flags has SPK_CONV_WINOGRAD
int spk_conv2d_wino_fwd(const spk_conv2d_desc* d, void* stream) {
    spkconv::SlicedPlan p;
    Args a;
    WinoKernel k;
    int rc = plan_args(d, p, a, k);
    if (rc != SPK_OK) return rc;
    const void* kern = wino_kernel_of(k);
    rc = spk::raise_dynamic_lds(kern, LDS_BYTES);
    if (rc != SPK_OK) return rc;
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return spk::fail(SPK_ELAUNCH, "conv2d winograd: no device properties");
        n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    long long gx = wino_grid_x(n_cu, k.co_tiles, k.n_items);
    static int lab_mult = -1;       // LAB: SPK_WINO_WGS = workgroups per CU slot (0: one workgroup per item)
    if (lab_mult < 0) { const char* e = getenv("SPK_WINO_WGS"); lab_mult = e ? atoi(e) : 1; }
    if (lab_mult != 1) {
        const long long every = (k.n_items + 7) / 8 * 8;
        gx = lab_mult == 0 ? every : std::min(wino_grid_x(n_cu, k.co_tiles, 1ll << 40) * lab_mult, every);
    }
    void* argv[1] = {&a};
    (void)hipLaunchKernel(kern, dim3((unsigned)gx, (unsigned)k.co_tiles), dim3(NT), argv, LDS_BYTES, (hipStream_t)stream);
    rc = spk::check_launch("wino_kernel");
    return rc != SPK_OK ? rc : spkconv::launch_finish(p.finish, (hipStream_t)stream);
}

int spk_conv2d_wino_form(const spk_conv2d_desc* d, int n_cu, spk_wino_form* out) {
    SPK_REQUIRE(d && out && n_cu > 0, "conv2d winograd form: null pointer or no CUs");
    SPK_REQUIRE(d->flags & SPK_CONV_WINOGRAD, "conv2d winograd form: serves SPK_CONV_WINOGRAD descriptors only");
    *out = spk_wino_form{};
    spkconv::SlicedPlan p;
    Args a;
    WinoKernel k;
    const int rc = plan_args(d, p, a, k);
    if (rc != SPK_OK) return rc;
    out->shape = k.shape; out->mod = k.mod; out->rgb = k.rgb; out->up = k.up; out->epi = k.epi_form;
    out->n_chunks = a.n_chunks; out->ksplit = a.ksplit; out->chunks_per_slice = a.cps; out->groups = a.G;
    out->co_tiles = k.co_tiles; out->items = (int32_t)k.n_items;
    const long long gx = wino_grid_x(n_cu, k.co_tiles, k.n_items);
    out->grid_x = (int32_t)gx;
    // the kernel's dealing: XCD share x of the item list has items / 8 (+ 1 for x < items % 8) items, its gx / 8 workgroups take
    // every (gx / 8)-th of them: the first of the largest share walks the most, the last of the smallest share the fewest
    const long long wpx = gx >> 3, share_q = k.n_items >> 3, share_r = k.n_items & 7;
    out->walk_max = (int32_t)((share_q + (share_r ? 1 : 0) + wpx - 1) / wpx);
    out->walk_min = (int32_t)(share_q / wpx);
    int seg = 0;
    out->finisher = a.ksplit > 1 ? spkconv::splitk_finisher(p.finish.args, p.finish.ws, &seg) : 0;
    out->finisher_seg = seg;
    out->lds_bytes = LDS_BYTES;
    return SPK_OK;
}

}  // extern "C"
