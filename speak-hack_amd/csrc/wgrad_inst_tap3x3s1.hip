// Weight gradient, one accumulator tile per tap, of a 3x3 stride 1 (SPK_WGRAD_TAP, SPK_WGRAD_TAP_FIXED).
#include "wgrad_tap_kernel.hpp"

int spkwg::launch_tap3x3s1(const WgradPlan& p, hipStream_t stream) { return launch_planned(tap_kernel<3, 3, 1>(p), "wgrad_kernel", p, stream); }
