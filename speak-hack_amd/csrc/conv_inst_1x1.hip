// 1x1 instantiations (stride 1 and 2): deep chunks (CI_T = 32 / 16) since a chunk has only CI_T/2 k-steps.
#include "conv_plan.hpp"

namespace spkconv {

template <int ID, class C, int S>
static const void* by_mode(int mode) {
    if constexpr (S == 1) {
        if (mode == MODE_PLAIN_RESIDUAL) return tap_kernel_ptr<ID, C, 1, 1, 1, MODE_PLAIN_RESIDUAL>();
    }
    if (mode == MODE_AFFINE_RELU) return tap_kernel_ptr<ID, C, 1, 1, S, MODE_AFFINE_RELU>();
    return mode == MODE_PLAIN ? tap_kernel_ptr<ID, C, 1, 1, S, MODE_PLAIN>() : nullptr;
}

template <int S>
static const void* by_cfg(int cfg, int mode) {
    switch (cfg) {
        case 8: return by_mode<SPK_TAP_CFG(8), S>(mode);
        case 9: return by_mode<SPK_TAP_CFG(9), S>(mode);
        case 10: return by_mode<SPK_TAP_CFG(10), S>(mode);
        case 11: return by_mode<SPK_TAP_CFG(11), S>(mode);
        default: return nullptr;
    }
}

const void* tap_kernel_1x1(int stride, int cfg, int mode, bool fg) {
    if (fg) return nullptr;
    return stride == 2 ? by_cfg<2>(cfg, mode) : by_cfg<1>(cfg, mode);
}

}  // namespace spkconv
