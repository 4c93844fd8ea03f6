// Shared by the weight-gradient units: the kernel argument block, the modes, the block shapes with the LDS sizes the planner needs,
// the plan a launch executes (wgrad_mfma_f32.hip builds it, the wgrad_inst_*.hip units launch their kernels from it) and the one
// launch helper.  Everything lives in namespace spkwg.
#pragma once
#include "spk_common.hpp"

#include <type_traits>

namespace spkwg {

typedef float f32x16 __attribute__((ext_vector_type(16)));
// LDS-typed fragment pointers: a volatile read stays ONE ds_read_b32 with a 16-bit immediate offset.  Left to itself the compiler
// merges neighbouring reads into ds_read2_b32 (1 KB reach) and pays a v_add_u32 per pair -- and on gfx950 every vector-ALU
// instruction of an f32-MFMA kernel is paid for in matrix time: 67 of the 183 per 288 MFMAs of the wide kernel.
typedef __attribute__((address_space(3))) float wg_lds_f32;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) f32x4 wg_lds_f32x4;
typedef __attribute__((address_space(3))) unsigned char wg_lds_u8;

template <int I, int N, class F>
__device__ __forceinline__ void wg_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        wg_static_for<I + 1, N>(f);
    }
}

// WG_BATCH_SCALE: the modulated convolution (StyleGAN2 variant): the forward input was x * s[b,ci] and the gradient reaching
// the conv output is g * d'[b,co] (demodulation x activation gain) -- both factors are applied while the tiles are staged, so
// neither rescaled tensor exists in HBM (in_scale = s [B][Cx], g_scale = d' [B][Cy])
enum { WG_PLAIN = 0, WG_UPSAMPLE = 1, WG_AFFINE_RELU = 2, WG_BATCH_SCALE = 3 };
constexpr int form_mode(int mode) { return mode == WG_AFFINE_RELU ? 1 : (mode == WG_BATCH_SCALE ? 2 : 0); }      // spk_wgrad_form.mode

struct WgradArgs {
    const float* g;        // [B,Cout,H,W]   output-side gradient
    const float* x;        // [B,Cin,Hs,Ws]  forward input
    const float* in_scale; // WG_AFFINE_RELU: [Cx]; WG_BATCH_SCALE: s [B][Cx]
    const float* in_shift;
    const float* g_scale;  // WG_BATCH_SCALE: d' [B][Cy]
    float* slabs;          // [n_slabs][Cout][TAPS][Cin]
    int B, Cin, Cout, H, W, Hs, Ws;   // Cin / Cout PER GROUP
    int lgTW, lgTH, lgTB;
    int tiles_x, tiles_y, n_tiles;
    // grouped form (G independent convs per launch): g has Cy = G*Cout channels, x has Cx, group q reads x channels
    // [q*gin, q*gin + Cin); Cout is a multiple of CO_T so that a workgroup's co block lies in one group
    int Cx, Cy, gin;
};

template <int KH, int KW, int S>
struct WShape {
    static constexpr int TAPS = KH * KW;
    // 7x7 (the ResNet stem, Cin = 3): the 32 lanes of the B fragment are (kx, ci) pairs instead of 32 input channels --
    // 7*3 = 21 of 32 lanes do work, where one-channel-per-lane would use 3 -- and there is one accumulator tile per tap
    // ROW (ky); needs KW * Cin <= 32.
    static constexpr bool PACK = KH == 7;
    // 4x4 (the weight gradient of ConvTranspose2d(4, s2, p1), styleganv1.py:231): 16 accumulator tiles would be 256 registers
    // on top of the staging state, so a workgroup owns ONE tap row (blockIdx.y carries the row) and holds KW tiles
    static constexpr bool ROWPASS = KH == 4;
    static constexpr int TP = PACK ? KH : (ROWPASS ? KW : TAPS);     // accumulator tiles per wave
    static constexpr int CI_T = PACK ? 4 : (S == 2 ? 32 : 64);
    static constexpr int WCI = PACK ? 1 : CI_T / 32, WPX = 2 / WCI;    // 4 waves = 2 (co) x WCI x WPX
    static constexpr int CO_T = 64, PIX_T = 64, PAD = (KH - 1) / 2;
    // Staging of the input tile: a thread owns KX plane positions and, of the CI_T channels, one of CS slices -- with
    // CS = 2 (the 64-channel 3x3 stride-1 form, whose tile has <= 128 positions) all 256 threads work on 32 channels
    // each instead of half of them on 64.
    static constexpr int CS = (!PACK && S == 1 && CI_T == 64) ? 2 : 1;
    static constexpr int NPT = 256 / CS;                        // threads per channel slice = positions per round
    static constexpr int CPT = CI_T / CS;                       // channels a thread stages
    static constexpr int KX = KH == 7 ? 3 : (S == 2 ? 2 : 1);   // plane positions (x NPT) a thread stages
};

// wgrad3x3_wide_kernel (and, at TW = 16, the tile of wgrad3x3_pipe_kernel and wgrad3x3_up_kernel)
template <int TW_>
struct WideShapeT {
    static constexpr int CO_T = 64, CI_T = 64, NT = 256;
    static constexpr int TW = TW_, TH = 64 / TW, PW = TW + 2, PH = TH + 2, PLANE = PH * PW;
    static constexpr int GPITCH = TW * TH + 1, XPITCH = PLANE | 1;
    static constexpr int BUF = (CO_T * GPITCH + CI_T * XPITCH + 1 + 3) & ~3;       // floats per buffer (+ a dump slot: BUF - 1)
    static constexpr int NG4 = CO_T / 16;            // float4 pieces of the gradient tile per thread (16 channels per piece)
    static constexpr int NXK = TW / 4;               // float4 per plane row (the aligned columns 0 .. TW-1)
    static constexpr int RS = 256 / (CI_T * NXK);    // plane rows covered by one float4 piece (1 or 2)
    static constexpr int NX4 = (PH + RS - 1) / RS;   // float4 pieces of the input tile
    static constexpr int NXH = (PH + 1) / 2;         // halo-dword pieces (piece = two plane rows x 2 sides of 64 channels)
    static constexpr int NL = NG4 + NX4 + NXH, NS = 4 * NG4 + 4 * NX4 + NXH;
    static constexpr int STEPS = 32, HS = STEPS / 2;
    static constexpr int PL = (NL + HS - 1) / HS, PS = (NS + HS - 1) / HS;
    static_assert(XPITCH % 2 == 1, "odd pitch");
};

// wgrad3x3_pipe_kernel: the tile images of the wide form at TW = 16, two LDS buffers
constexpr int WP_BUF = WideShapeT<16>::BUF;
static_assert(WP_BUF == 64 * 65 + 64 * 109 + 4, "floats per buffer (+ a dump slot for idle lanes)");

// wgrad3x3_s2_kernel
template <int TW_>
struct S2Shape {
    static constexpr int CO_T = 128, CI_T = 32, TW = TW_, TH = 64 / TW, PW = 2 * TW + 1, PH = 2 * TH + 1, PLANE = PH * PW;
    static constexpr int GPITCH = 65, XPITCH = PLANE | 1;
    static constexpr int BUF = (CO_T * GPITCH + CI_T * XPITCH + 1 + 3) & ~3;        // floats per buffer (+ a dump slot: BUF - 1)
    static constexpr int NG4 = CO_T / 16;                 // float4 pieces of the gradient tile per thread (16 channels per piece)
    static constexpr int NXK = 2 * TW / 4;                // float4 per plane row
    static constexpr int RS = 256 / (CI_T * NXK);         // plane rows covered by one piece (1 or 2)
    static constexpr int NX4 = (PH + RS - 1) / RS;        // float4 pieces of the input tile
    static constexpr int NXH = (PH + 7) / 8;              // halo-dword pieces (piece = 8 plane rows x 32 channels)
    static constexpr int NL = NG4 + NX4 + NXH, NS = 4 * NG4 + 4 * NX4 + NXH;
    static constexpr int STEPS = 32, HS = STEPS / 2;
    static constexpr int PL = (NL + HS - 1) / HS, PS = (NS + HS - 1) / HS;
    static_assert(XPITCH % 2 == 1, "odd pitch: the 32 channels of a fragment hit 32 banks");
};

// wgrad3x3_up_kernel: the low-resolution source patch of a 16 x 4 tile
constexpr int US_PW = 10, US_PH = 4, US_PITCH = US_PW * US_PH + 1, US_FLOATS = 64 * US_PITCH;

// wgrad1x1_kernel / wgrad1x1_dma_kernel: 32-pixel k-tiles
constexpr int G1_KT = 32, G1_PITCH = G1_KT + 1;

// wgrad_stem_kernel
constexpr int SW_TH = 4, SW_TW = 32, SW_PR = 2 * SW_TH + 5, SW_PC = 2 * SW_TW + 5, SW_PH = SW_TW + 3, SW_PROW = 2 * SW_PH;
constexpr int SW_K = 147, SW_NT = 5;
constexpr int SW_GP = SW_TH * SW_TW + 1;                       // pitch of a channel's gradients (odd: 32 channels, 32 banks)
constexpr int SW_G_FL = 64 * SW_GP, SW_P_FL = 3 * SW_PR * SW_PROW;
constexpr int SW_LDS_FL = SW_G_FL + SW_P_FL;                   // 8256 + 2730 floats = 43.9 KB: two workgroups per CU
constexpr int SW_TASKS = 3 * SW_PR, SW_TPW = (SW_TASKS + 3) / 4;
static_assert(SW_LDS_FL * 4 >= 4 * 2 * 16 * 64 * 4, "the final cross-wave sum of one n-tile fits the same LDS");

// Everything one launch needs, stated by plan_wgrad (wgrad_mfma_f32.hip) from a spk_wgrad_desc without a HIP call.
struct WgradPlan {
    int form, mode;                         // SPK_WGRAD_*; the kernel's WG_* mode (form_mode(mode) is spk_wgrad_form.mode)
    int kh, kw, stride;
    int TW, TH, TB, MT, NT;                 // pixel tile; MFMA tiles per wave of the 1x1 GEMM forms (else 0)
    int n_tiles, splits, tiles_per_split;
    int n_slabs, ws_slabs;                  // slabs the reducer sums; slabs the workspace check asks for
    size_t slab_floats;
    dim3 grid;
    size_t lds_bytes;
    // the reduce: dw[red_cout / fold][red_cin][taps] from n_slabs slabs [red_cout][taps][red_cin]
    int reducer, fold, taps, red_cout, red_cin, accumulate;
    float scale;
    float* dw;
    WgradArgs args;
};

// which of wgrad_reduce_kernel (0) / _vec_ (1) / _deep_ (2) sums n_slabs slabs of slab_floats floats into dw
inline int pick_reducer(const float* slabs, const float* dw, int n_slabs, size_t slab_floats, int Cin, int fold) {
    const bool vec = Cin % 4 == 0 && (reinterpret_cast<uintptr_t>(slabs) & 15) == 0 && (reinterpret_cast<uintptr_t>(dw) & 15) == 0;
    const bool deep = vec && n_slabs >= 32 && slab_floats / fold / 4 / 256 < 512;
    return deep ? 2 : (vec ? 1 : 0);
}

// raise the LDS limit if need be, launch `kernel` on the plan's grid, check under `name`.  The kernels take (WgradArgs) or
// (WgradArgs, int tiles_per_split): the runtime reads as many arguments as the kernel declares.
inline int launch_planned(const void* kernel, const char* name, const WgradPlan& p, hipStream_t stream) {
    int rc = spk::raise_dynamic_lds(kernel, p.lds_bytes);
    if (rc != SPK_OK) return rc;
    void* argv[2] = {const_cast<WgradArgs*>(&p.args), const_cast<int*>(&p.tiles_per_split)};
    (void)hipLaunchKernel(kernel, p.grid, dim3(256), argv, p.lds_bytes, stream);
    return spk::check_launch(name);
}

// one per kernel unit: (form, mode, shape) of the plan -> the template instantiation, launched
int launch_tap3x3s1(const WgradPlan& p, hipStream_t stream);   // wgrad_inst_tap3x3s1.hip: TAP, TAP_FIXED of a 3x3 stride 1
int launch_tap(const WgradPlan& p, hipStream_t stream);        // wgrad_inst_tap.hip: TAP of every other shape
int launch_pipe_up(const WgradPlan& p, hipStream_t stream);    // wgrad_inst_pipe_up.hip: PIPE, UP
int launch_wide(const WgradPlan& p, hipStream_t stream);       // wgrad_inst_wide.hip: WIDE16, WIDE8
int launch_s2_stem(const WgradPlan& p, hipStream_t stream);    // wgrad_inst_s2_stem.hip: S2_16, S2_8, STEM
int launch_gemm1x1(const WgradPlan& p, hipStream_t stream);    // wgrad_inst_gemm1x1.hip: GEMM1X1, GEMM1X1_DMA

// wgrad3x3_wino_f32.hip: the plan of spk_conv2d_wgrad_wino(d), less its kernel's own argument block (form SPK_WGRAD_WINO)
int plan_wino(const spk_wgrad_desc* d, WgradPlan& p);

}  // namespace spkwg
