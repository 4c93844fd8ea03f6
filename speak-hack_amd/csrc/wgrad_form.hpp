// spk_conv2d_wgrad_launch_form: while `form_probe` is set (on the calling thread), the weight-gradient launchers answer here at the
// point where they would raise the LDS attribute and launch, and launch_wgrad_reduce answers which reducer it would run -- the
// launch path's own statements, no device call.  Host code only.
#pragma once
#include "spk_common.hpp"

namespace spkwg {

extern thread_local spk_wgrad_form* form_probe;       // (defined in wgrad_mfma_f32.hip)

// mode: the WG_* / wino MODE of the kernel as spk_wgrad_form states it (0 plain, 1 affine + ReLU, 2 batch scale)
// ws_slabs: the slabs the launcher's workspace check asks for (the stem form asks for more than it sums when tiles are few)
inline void report_form(int kernel, int mode, int TW, int TH, int TB, int MT, int NT, int n_tiles, int splits, int tiles_per_split,
                        dim3 grid, size_t lds_bytes, size_t slab_floats, size_t ws_slabs) {
    spk_wgrad_form& f = *form_probe;
    f.kernel = kernel; f.mode = mode; f.TW = TW; f.TH = TH; f.TB = TB; f.MT = MT; f.NT = NT;
    f.n_tiles = n_tiles; f.splits = splits; f.tiles_per_split = tiles_per_split;
    f.grid_x = (int)grid.x; f.grid_y = (int)grid.y; f.grid_z = (int)grid.z;
    f.lds_bytes = (int64_t)lds_bytes; f.slab_floats = (int64_t)slab_floats;
    f.workspace_bytes = (int64_t)(ws_slabs * slab_floats * sizeof(float));
}

}  // namespace spkwg
