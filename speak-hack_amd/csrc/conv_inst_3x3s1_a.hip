// 3x3 stride-1 instantiations, full-depth chunk configs (CI_T = 8): ids 0-3.
#include "conv_plan.hpp"

namespace spkconv {

template <int ID, class C>
static const void* by_mode(int mode) {
    switch (mode) {
        case MODE_PLAIN: return tap_kernel_ptr<ID, C, 3, 3, 1, MODE_PLAIN>();
        case MODE_UPSAMPLE: return tap_kernel_ptr<ID, C, 3, 3, 1, MODE_UPSAMPLE>();
        case MODE_AFFINE_RELU: return tap_kernel_ptr<ID, C, 3, 3, 1, MODE_AFFINE_RELU>();
        default: return nullptr;
    }
}

const void* tap_kernel_3x3s1_a(int cfg, int mode, bool fg) {
    if (fg) return nullptr;
    switch (cfg) {
        case 0: return by_mode<SPK_TAP_CFG(0)>(mode);
        case 1: return by_mode<SPK_TAP_CFG(1)>(mode);
        case 2: return by_mode<SPK_TAP_CFG(2)>(mode);
        case 3: return by_mode<SPK_TAP_CFG(3)>(mode);
        default: return nullptr;
    }
}

}  // namespace spkconv
