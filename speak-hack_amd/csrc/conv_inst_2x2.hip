// 2x2 stride-1 instantiations (window rows y, y+1 / columns x, x+1, zeros beyond the input): the four output-parity
// classes of the data gradient of a 3x3 stride-2 pad-1 conv (the bottleneck conv2 of the first block of layer2-4 of the
// trunk; every block's conv2 of StyleDiscriminator, styleganv1.py:644-657), written interleaved into the full-size
// gradient by the kernel's epilogue.  dx[2m+py, 2n+px] needs 1 / 2 / 2 / 4 of the 9 taps; the zero-dilated form ran all
// 9 at four times the pixels.  The same four-class launch, anchored one pixel up / left (pshift = 1), is the forward of
// nn.ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1), the fused upscale of the legacy GBlock (styleganv1.py:231): every
// output pixel (2m+py, 2n+px) takes exactly 2x2 of the 16 taps.
#include "conv_plan.hpp"

namespace spkconv {

const void* tap_kernel_2x2(int cfg, int mode, bool fg) {
    if (fg || mode != MODE_PLAIN) return nullptr;
    switch (cfg) {
        case 0: return tap_kernel_ptr<SPK_TAP_CFG(0), 2, 2, 1, MODE_PLAIN>();
        case 1: return tap_kernel_ptr<SPK_TAP_CFG(1), 2, 2, 1, MODE_PLAIN>();
        case 2: return tap_kernel_ptr<SPK_TAP_CFG(2), 2, 2, 1, MODE_PLAIN>();
        case 3: return tap_kernel_ptr<SPK_TAP_CFG(3), 2, 2, 1, MODE_PLAIN>();
        default: return nullptr;
    }
}

}  // namespace spkconv
