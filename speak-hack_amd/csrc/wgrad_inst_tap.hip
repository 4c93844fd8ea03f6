// Weight gradient, one accumulator tile per tap, of a 1x1, a 3x3 stride 2, a 4x4 stride 2 (in row passes) and a 7x7 stride 2 (packed)
// (SPK_WGRAD_TAP).
#include "wgrad_tap_kernel.hpp"

int spkwg::launch_tap(const WgradPlan& p, hipStream_t stream) {
    const void* k = p.kh == 1 ? (p.stride == 1 ? tap_kernel<1, 1, 1>(p) : tap_kernel<1, 1, 2>(p))
                  : p.kh == 3 ? tap_kernel<3, 3, 2>(p) : p.kh == 4 ? tap_kernel<4, 4, 2>(p) : tap_kernel<7, 7, 2>(p);
    return launch_planned(k, "wgrad_kernel", p, stream);
}
