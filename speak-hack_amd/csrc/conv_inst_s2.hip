// stride-2 instantiations: 3x3 s2 (bottleneck conv2 of the first block of layer2-4), the 7x7 s2 stem, and 4x4 s2 pad 1 --
// the data gradient of nn.ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1), the fused upscale of the legacy GBlock
// (styleganv1.py:231): dx = conv2d(dy, weight, stride 2, pad 1) with the module's [Cin,Cout,4,4] parameter read as a conv
// weight [out = Cin][in = Cout].
#include "conv_plan.hpp"

namespace spkconv {

template <int ID, class C, int K, bool FG>
static const void* by_mode(int mode) {
    if constexpr (K == 7 || K == 4) {   // the stem reads the raw image, the 4x4 a gradient: no producer BatchNorm to fold in
        return !FG && mode == MODE_PLAIN ? tap_kernel_ptr<ID, C, K, K, 2, MODE_PLAIN>() : nullptr;
    } else if constexpr (FG && C::PIX_T < 64) {
        return nullptr;
    } else {      // 3x3 stride 2: also in the fixed-geometry build (32-wide output tiles; conv_mfma_f32.hpp, FG)
        if (mode == MODE_AFFINE_RELU) return tap_kernel_ptr<ID, C, K, K, 2, MODE_AFFINE_RELU, FG>();
        return mode == MODE_PLAIN ? tap_kernel_ptr<ID, C, K, K, 2, MODE_PLAIN, FG>() : nullptr;
    }
}

template <int K, bool FG>
static const void* by_cfg(int cfg, int mode) {
    switch (cfg) {
        case 4: return by_mode<SPK_TAP_CFG(4), K, FG>(mode);
        case 5: return by_mode<SPK_TAP_CFG(5), K, FG>(mode);
        case 6: return by_mode<SPK_TAP_CFG(6), K, FG>(mode);
        case 7: return by_mode<SPK_TAP_CFG(7), K, FG>(mode);
        default: return nullptr;
    }
}

const void* tap_kernel_s2(int kh, int cfg, int mode, bool fg) {
    if (kh == 7) return fg ? nullptr : by_cfg<7, false>(cfg, mode);
    if (kh == 4) return fg ? nullptr : by_cfg<4, false>(cfg, mode);
    return fg ? by_cfg<3, true>(cfg, mode) : by_cfg<3, false>(cfg, mode);
}

}  // namespace spkconv
