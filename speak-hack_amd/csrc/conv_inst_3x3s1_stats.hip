// 3x3 stride-1 instantiations with the BatchNorm-statistics epilogue on a plain input (MODE_PLAIN_STATS), ids 0-7: kept apart
// from the decoders' hot instantiations, whose code generation the statistics epilogue measurably disturbs
// (conv_mfma_f32.hpp, HAS_STATS).
#include "conv_plan.hpp"

namespace spkconv {

const void* tap_kernel_3x3s1_stats(int cfg, int mode, bool fg) {
    if (fg || mode != MODE_PLAIN_STATS) return nullptr;
    switch (cfg) {
        case 0: return tap_kernel_ptr<SPK_TAP_CFG(0), 3, 3, 1, MODE_PLAIN_STATS>();
        case 1: return tap_kernel_ptr<SPK_TAP_CFG(1), 3, 3, 1, MODE_PLAIN_STATS>();
        case 2: return tap_kernel_ptr<SPK_TAP_CFG(2), 3, 3, 1, MODE_PLAIN_STATS>();
        case 3: return tap_kernel_ptr<SPK_TAP_CFG(3), 3, 3, 1, MODE_PLAIN_STATS>();
        case 4: return tap_kernel_ptr<SPK_TAP_CFG(4), 3, 3, 1, MODE_PLAIN_STATS>();
        case 5: return tap_kernel_ptr<SPK_TAP_CFG(5), 3, 3, 1, MODE_PLAIN_STATS>();
        case 6: return tap_kernel_ptr<SPK_TAP_CFG(6), 3, 3, 1, MODE_PLAIN_STATS>();
        case 7: return tap_kernel_ptr<SPK_TAP_CFG(7), 3, 3, 1, MODE_PLAIN_STATS>();
        default: return nullptr;
    }
}

}  // namespace spkconv
