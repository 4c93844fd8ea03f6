// 3x3 stride-1 instantiations, half-depth chunk configs (CI_T = 4): ids 4-7.
#include "conv_plan.hpp"

namespace spkconv {

// (every mode also exists with the fixed 32-wide tile geometry -- conv_kernel<..., FG = true> -- for the 64-, 128- and 256-pixel
// tiles: the layers from 32^2 up)
template <int ID, class C, bool FG>
static const void* by_mode(int mode) {
    if constexpr (FG && C::PIX_T < 64) return nullptr;
    else switch (mode) {
        case MODE_PLAIN: return tap_kernel_ptr<ID, C, 3, 3, 1, MODE_PLAIN, FG>();
        case MODE_UPSAMPLE: return tap_kernel_ptr<ID, C, 3, 3, 1, MODE_UPSAMPLE, FG>();
        case MODE_BATCH_SCALE: return tap_kernel_ptr<ID, C, 3, 3, 1, MODE_BATCH_SCALE, FG>();
        case MODE_UPSAMPLE_BATCH_SCALE: return tap_kernel_ptr<ID, C, 3, 3, 1, MODE_UPSAMPLE_BATCH_SCALE, FG>();
        case MODE_AFFINE_RELU: return tap_kernel_ptr<ID, C, 3, 3, 1, MODE_AFFINE_RELU, FG>();
        default: return nullptr;
    }
}

const void* tap_kernel_3x3s1_b(int cfg, int mode, bool fg) {
    switch (cfg) {
        case 4: return fg ? by_mode<SPK_TAP_CFG(4), true>(mode) : by_mode<SPK_TAP_CFG(4), false>(mode);
        case 5: return fg ? by_mode<SPK_TAP_CFG(5), true>(mode) : by_mode<SPK_TAP_CFG(5), false>(mode);
        case 6: return fg ? by_mode<SPK_TAP_CFG(6), true>(mode) : by_mode<SPK_TAP_CFG(6), false>(mode);
        case 7: return fg ? by_mode<SPK_TAP_CFG(7), true>(mode) : by_mode<SPK_TAP_CFG(7), false>(mode);
        default: return nullptr;
    }
}

}  // namespace spkconv
