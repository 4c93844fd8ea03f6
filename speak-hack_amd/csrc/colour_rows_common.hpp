// What the makers of colour rows share (csrc/frame_blend_common.hpp: a row per frame from the frame's own sums;
// csrc/colour_window.hip: from sums pooled over a window of frames): the layout of the 13 sums and the check of the row formula's
// three parameters.  Kept apart from the statistics' kernels so that a file which only reads sums does not carry a copy of them.
#pragma once

#include "spk_common.hpp"
#include <cmath>

namespace spk::frame {

constexpr int SUMS = 13;                // S0, then (Sq, Sqq, Sb, Sbb) for each of the three channels

// the three parameters of the row formula, alike wherever rows are made from sums
inline int check_match_params(const char* who, double max_gain, double min_sigma, double min_weight) {
    SPK_REQUIRE(std::isfinite(max_gain) && max_gain >= 1.0, "%s: max_gain must be a finite number >= 1 (got %g)", who, max_gain);
    SPK_REQUIRE(std::isfinite(min_sigma) && min_sigma >= 0.0, "%s: min_sigma must be a finite number >= 0 (got %g)", who, min_sigma);
    SPK_REQUIRE(std::isfinite(min_weight) && min_weight >= 0.0, "%s: min_weight must be a finite number >= 0 (got %g)", who, min_weight);
    return SPK_OK;
}

// THE ROW FORMULA (include/spk.h, spk_paste_colour_match_sim): the (gain, offset) of one channel from its five sums, fp64, each
// rounded to fp32 once; (1, 0) when `ok` does not hold.  min_var = min_sigma^2.  Every maker of rows calls this one function.
__device__ __forceinline__ void colour_row(double S0, double Sq, double Sqq, double Sb, double Sbb, bool ok, double max_gain, double min_var,
                                           float& g, float& o) {
    g = 1.f, o = 0.f;
    if (ok) {
        const double mu_q = Sq / S0, var_q = fmax(Sqq / S0 - mu_q * mu_q, 0.0);
        const double mu_b = Sb / S0, var_b = fmax(Sbb / S0 - mu_b * mu_b, 0.0);
        const double gain = var_q <= min_var ? 1.0 : fmin(fmax(sqrt(var_b / var_q), 1.0 / max_gain), max_gain);
        g = (float)gain, o = (float)(mu_b - gain * mu_q);
    }
}

}  // namespace spk::frame
