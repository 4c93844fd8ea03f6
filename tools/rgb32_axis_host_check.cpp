// Host-side check of the axis-aligned RGB32 edge (csrc/frame_rgb32.hip) under AddressSanitizer / UBSan: every refusal of
// spk_frames_rgb32_to_f32, spk_frames_rgb32_to_f32_boxes, spk_frames_paste_rgb32 and spk_frames_f32_to_rgb32 -- null pointers, sizes
// below 1, a box larger than the frame, a row stride below 4 W, each misalignment (the base, the row stride, the image stride),
// alpha_first and alpha out of range, overlapping written frames and negative strides of read ones, the feather-table pairing, the
// value range, and the strides whose extents leave 32 bits (the arithmetic is 64-bit: nothing wraps) -- and the frames that must
// PASS: a region-of-interest view that is 4-aligned and not 16-aligned, frames that touch, the smallest frame, one frame with any
// image stride.  Every refusal happens before a launch and before anything is dereferenced, so no device is needed.  A frame that
// passes is shown twice: by the refusal of the argument that is checked BEHIND the frames (the paste and the way out: the value
// range; the way out also: alpha), by its message; and, on a machine WITHOUT a device only, by running accepted argument sets up to
// the launch, which then fails with SPK_ELAUNCH and not SPK_EINVAL (with a device the launch would run on host pointers: skipped,
// and said so).  The file is linked with nothing else: what it shares with csrc/frame_io.hip lives in headers.  Build and run from
// the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/frame_rgb32.hip tools/rgb32_axis_host_check.cpp -o tools/_bin/rgb32_axis_host_check
//   tools/_bin/rgb32_axis_host_check
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    alignas(16) static uint8_t raw[8192];
    alignas(16) static float fl[3 * 8 * 8 * 2];                           // a source / an output of two 8 x 8 images
    alignas(16) static int32_t tab[8];                                     // first / count rows: zeros
    alignas(16) static float wt[16];                                       // weights
    int refusals = 0, passes = 0, launched = 0;

    // Two 8 x 8 frames at pitch 48 (4 W = 32), 384 bytes per frame, from raw + 64
    struct Frames { uint8_t* px; int64_t img, row; int N, H, W, swap_rb, alpha_first; };
    const Frames okf = {raw + 64, 384, 48, 1, 8, 8, 1, 0};
    struct InArgs { Frames f; float* dst; const int32_t* tab; const float* w; const int32_t* boxes; int Hin, Win, taps, Hout, Wout; };
    const InArgs oki = {okf, fl, tab, wt, tab, 4, 4, 2, 2, 2};
    auto in = [&](const InArgs& a) {                                       // the box is the frame
        return spk_frames_rgb32_to_f32(a.f.px, a.f.img, a.f.row, a.f.N, a.f.H, a.f.W, a.f.swap_rb, a.f.alpha_first, a.tab, a.tab, a.w, a.taps, a.tab,
                                       a.tab, a.w, a.taps, a.dst, a.Hout, a.Wout, 1.f, 1.f, 1.f, 0.f, 0.f, 0.f, nullptr);
    };
    auto boxes = [&](const InArgs& a) {
        return spk_frames_rgb32_to_f32_boxes(a.f.px, a.f.img, a.f.row, a.f.N, a.f.H, a.f.W, a.boxes, a.Hin, a.Win, a.f.swap_rb, a.f.alpha_first, a.tab,
                                             a.tab, a.w, a.taps, a.tab, a.tab, a.w, a.taps, a.dst, a.Hout, a.Wout, 1.f, 1.f, 1.f, 0.f, 0.f, 0.f,
                                             nullptr);
    };
    struct PasteArgs { Frames f; const float* src; const int32_t* tab; const float* w; const float* ay; const float* ax; int Hs, Ws, h, w_, taps; float lo, k; };
    const PasteArgs okp = {okf, fl, tab, wt, nullptr, nullptr, 4, 4, 4, 4, 2, -1.f, 127.5f};
    auto paste = [&](const PasteArgs& a) {
        return spk_frames_paste_rgb32(a.src, a.f.N, a.Hs, a.Ws, a.f.px, a.f.img, a.f.row, a.f.H, a.f.W, a.h, a.w_, 1, 1, nullptr, a.f.swap_rb,
                                      a.f.alpha_first, a.tab, a.tab, a.w, a.taps, a.tab, a.tab, a.w, a.taps, a.ay, a.ax, a.lo, a.k, nullptr);
    };
    struct OutArgs { Frames f; const float* src; int alpha; float lo, k; };
    const OutArgs oko = {okf, fl, 255, -1.f, 127.5f};
    auto out = [&](const OutArgs& a) {
        return spk_frames_f32_to_rgb32(a.src, a.f.px, a.f.img, a.f.row, a.f.N, a.f.H, a.f.W, a.f.swap_rb, a.f.alpha_first, a.alpha, a.lo, a.k, nullptr);
    };
    InArgs a;
    PasteArgs p;
    OutArgs o;

    // ---- what every frames argument gets, through each of the four entry points
#define FRAMES_REFUSED(stmt, word)                                                                                  \
    a = oki; { Frames& f = a.f; stmt; } CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));         \
    a = oki; { Frames& f = a.f; stmt; } CHECK(boxes(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));      \
    p = okp; { Frames& f = p.f; stmt; } CHECK(paste(p) == SPK_EINVAL && std::strstr(spk_last_error(), word));      \
    o = oko; { Frames& f = o.f; stmt; } CHECK(out(o) == SPK_EINVAL && std::strstr(spk_last_error(), word));        \
    refusals += 4
    FRAMES_REFUSED(f.px = nullptr, "null frame pointer");
    FRAMES_REFUSED(f.N = 0, "N / H / W");
    FRAMES_REFUSED(f.N = -3, "N / H / W");
    FRAMES_REFUSED(f.row = 31, "smaller than 4 * W");
    FRAMES_REFUSED(f.row = 24, "smaller than 4 * W");                      // the packed pitch 3 W
    FRAMES_REFUSED(f.row = 28, "smaller than 4 * W");                      // a multiple of 4 below 4 W
    FRAMES_REFUSED(f.row = -48, "smaller than 4 * W");
    FRAMES_REFUSED(f.W = 0x7fffffff, "smaller than 4 * W");                // 4 W is formed in 64 bits: 2^33 - 4 against the pitch 48
    FRAMES_REFUSED(f.row = 49, "row stride 49 is not a multiple of 4");
    FRAMES_REFUSED(f.row = 50, "row stride 50 is not a multiple of 4");
    FRAMES_REFUSED(f.row = 51, "row stride 51 is not a multiple of 4");
    FRAMES_REFUSED((f.N = 2, f.img = 385), "image stride 385 is not a multiple of 4");
    FRAMES_REFUSED((f.N = 2, f.img = 386), "image stride 386 is not a multiple of 4");
    FRAMES_REFUSED(f.px = raw + 65, "aligned to 4 bytes");
    FRAMES_REFUSED(f.px = raw + 66, "aligned to 4 bytes");
    FRAMES_REFUSED(f.px = raw + 67, "aligned to 4 bytes");
    FRAMES_REFUSED(f.alpha_first = 2, "alpha_first");
    FRAMES_REFUSED(f.alpha_first = -1, "alpha_first");
    FRAMES_REFUSED(f.alpha_first = 8, "alpha_first");                      // (the shift it stands for is no valid value of it)
#undef FRAMES_REFUSED
    // H and W below 1: the way in takes its box for the frame, the other three name the frame
    a = oki; a.f.H = 0; CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), "N / H / W")); ++refusals;
    a = oki; a.f.W = -8; CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), "N / H / W")); ++refusals;
    a = oki; a.f.H = 0; CHECK(boxes(a) == SPK_EINVAL && std::strstr(spk_last_error(), "does not fit")); ++refusals;      // no box fits a frame without rows
    p = okp; p.f.H = 0; CHECK(paste(p) == SPK_EINVAL && std::strstr(spk_last_error(), "N / H / W")); ++refusals;
    p = okp; p.f.W = -8; CHECK(paste(p) == SPK_EINVAL && std::strstr(spk_last_error(), "N / H / W")); ++refusals;
    o = oko; o.f.H = 0; CHECK(out(o) == SPK_EINVAL && std::strstr(spk_last_error(), "N / H / W")); ++refusals;
    o = oko; o.f.W = -8; CHECK(out(o) == SPK_EINVAL && std::strstr(spk_last_error(), "N / H / W")); ++refusals;

    // ---- two frames: a negative stride for the two that read; frames that overlap for the two that write
#define READ_REFUSED(stmt, word)                                                                                              \
    a = oki; a.f.N = 2; { Frames& f = a.f; stmt; } CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));        \
    a = oki; a.f.N = 2; { Frames& f = a.f; stmt; } CHECK(boxes(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));     \
    refusals += 2
    READ_REFUSED(f.img = -384, "negative");
    READ_REFUSED(f.img = -4, "negative");
#undef READ_REFUSED
#define WRITTEN_REFUSED(stmt, word)                                                                                           \
    p = okp; p.f.N = 2; { Frames& f = p.f; stmt; } CHECK(paste(p) == SPK_EINVAL && std::strstr(spk_last_error(), word));     \
    o = oko; o.f.N = 2; { Frames& f = o.f; stmt; } CHECK(out(o) == SPK_EINVAL && std::strstr(spk_last_error(), word));       \
    refusals += 2
    WRITTEN_REFUSED(f.img = 364, "overlap");                               // 8 rows of pitch 48 end at 7 * 48 + 32 = 368
    WRITTEN_REFUSED(f.img = 48, "overlap");
    WRITTEN_REFUSED(f.img = 0, "overlap");
    WRITTEN_REFUSED(f.img = -384, "overlap");
    // extents that leave 32 bits: (H - 1) * row stride + 4 W is formed in 64 bits, so a stride that a wrapped extent would let
    // through is refused
    WRITTEN_REFUSED((f.H = 0x7ffffffe, f.img = 384), "overlap");           // the extent is 48 * (2^31 - 3) + 32: about 2^36.6
    WRITTEN_REFUSED((f.row = (int64_t)1 << 32, f.img = 384), "overlap");   // 7 * 2^32 + 32: 32 if the pitch wrapped
    WRITTEN_REFUSED((f.row = ((int64_t)1 << 32) + 48, f.img = 368), "overlap");       // the pitch 48 if it wrapped, whose extent 368 would pass
    WRITTEN_REFUSED((f.W = 0x40000008, f.row = ((int64_t)1 << 32) + 32, f.img = (int64_t)1 << 32), "overlap");      // 4 W = 2^32 + 32: 32 if it wrapped
#undef WRITTEN_REFUSED

    // ---- each entry point's own arguments
#define REFUSED(var, ok, call, field, value, word) var = ok; var.field = value; CHECK(call(var) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED(a, oki, in, dst, nullptr, "null frame pointer");
    REFUSED(a, oki, in, tab, nullptr, "table");
    REFUSED(a, oki, in, w, nullptr, "table");
    REFUSED(a, oki, in, taps, 0, "tap count");
    REFUSED(a, oki, in, Hout, 0, "N / H / W");
    REFUSED(a, oki, in, Wout, -1, "N / H / W");
    REFUSED(a, oki, boxes, dst, nullptr, "null frame pointer");
    REFUSED(a, oki, boxes, boxes, nullptr, "null box origin");
    REFUSED(a, oki, boxes, tab, nullptr, "table");
    REFUSED(a, oki, boxes, w, nullptr, "table");
    REFUSED(a, oki, boxes, taps, -2, "tap count");
    REFUSED(a, oki, boxes, Hin, 0, "N / H / W");
    REFUSED(a, oki, boxes, Win, -1, "N / H / W");
    REFUSED(a, oki, boxes, Hin, 9, "does not fit");                        // the box is larger than the frame
    REFUSED(a, oki, boxes, Win, 9, "does not fit");
    REFUSED(a, oki, boxes, Hout, 0, "N / H / W");
    REFUSED(a, oki, boxes, Wout, -1, "N / H / W");

    REFUSED(p, okp, paste, src, nullptr, "null frame pointer");
    REFUSED(p, okp, paste, tab, nullptr, "table");
    REFUSED(p, okp, paste, w, nullptr, "table");
    REFUSED(p, okp, paste, ay, wt, "feather");                             // one feather table without the other
    REFUSED(p, okp, paste, ax, wt, "feather");
    REFUSED(p, okp, paste, Hs, 0, "N / H / W");
    REFUSED(p, okp, paste, Ws, -1, "N / H / W");
    REFUSED(p, okp, paste, h, 0, "N / H / W");
    REFUSED(p, okp, paste, w_, 0, "N / H / W");
    REFUSED(p, okp, paste, taps, 0, "tap count");
    REFUSED(p, okp, paste, lo, NAN, "value range");
    REFUSED(p, okp, paste, k, 0.f, "value range");
    REFUSED(p, okp, paste, k, INFINITY, "value range");

    REFUSED(o, oko, out, src, nullptr, "null frame pointer");
    REFUSED(o, oko, out, alpha, 256, "alpha must be");
    REFUSED(o, oko, out, alpha, -2, "alpha must be");
    REFUSED(o, oko, out, alpha, 0x7fffffff, "alpha must be");
    REFUSED(o, oko, out, lo, INFINITY, "value range");
    REFUSED(o, oko, out, k, -1.f, "value range");
    REFUSED(o, oko, out, k, NAN, "value range");
#undef REFUSED

    // ---- the frames that must pass: each is let through by the frames check of the two that write, which shows in the refusal
    // BEHIND it (the value range; for the way out alpha too)
#define PASSES(stmt)                                                                                                                   \
    p = okp; p.k = 0.f; { Frames& f = p.f; stmt; } CHECK(paste(p) == SPK_EINVAL && std::strstr(spk_last_error(), "value range"));      \
    o = oko; o.k = 0.f; { Frames& f = o.f; stmt; } CHECK(out(o) == SPK_EINVAL && std::strstr(spk_last_error(), "value range"));        \
    o = oko; o.alpha = 300; { Frames& f = o.f; stmt; } CHECK(out(o) == SPK_EINVAL && std::strstr(spk_last_error(), "alpha must be"));   \
    passes += 3
    PASSES((void)f);                                                       // as it is
    PASSES(f.px = raw + 64 + 48 * 3 + 4 * 5);                              // a view at pixel offset (3, 5): 4-aligned, not 16-aligned
    PASSES((f.px = raw + 64 + 48 + 4, f.H = 5, f.W = 7));                  // odd sizes inside the same pitch
    PASSES((f.N = 2, f.img = 368));                                        // two frames that touch: the extent itself
    PASSES((f.N = 2, f.img = 372));                                        // an image stride that is a multiple of 4 and of nothing more
    PASSES((f.H = 1, f.W = 1, f.row = 4));                                 // the smallest frame
    PASSES((f.img = 3));                                                   // one frame: its image stride is not looked at
    PASSES((f.img = -384));
    PASSES((f.alpha_first = 1, f.swap_rb = 0));                            // argb
    PASSES((f.H = 1, f.row = ((int64_t)1 << 40), f.N = 2, f.img = 32));    // one row: its stride does not count towards the extent
#undef PASSES

    // ---- accepted argument sets up to the launch, where there is no device to run them on host memory
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess) devices = 0;
    (void)hipGetLastError();
    if (devices == 0) {
#define LAUNCHED(call) { const int rc = (call); CHECK(rc != SPK_EINVAL && rc != SPK_OK); ++launched; }
        a = oki; LAUNCHED(in(a));
        a = oki; a.f.N = 2; a.f.alpha_first = 1; LAUNCHED(in(a));
        a = oki; a.f.px = raw + 64 + 48 * 3 + 4 * 5; a.f.H = 4; a.f.W = 3; LAUNCHED(in(a));
        a = oki; LAUNCHED(boxes(a));
        a = oki; a.f.N = 2; a.Hin = 8; a.Win = 8; LAUNCHED(boxes(a));       // the box is the whole frame
        p = okp; LAUNCHED(paste(p));
        p = okp; p.f.N = 2; p.ay = wt; p.ax = wt; LAUNCHED(paste(p));
        o = oko; LAUNCHED(out(o));                                          // the vector form
        o = oko; o.alpha = -1; o.f.N = 2; LAUNCHED(out(o));                 // keep
        o = oko; o.alpha = 0; o.f.px = raw + 64 + 4; o.f.W = 4; LAUNCHED(out(o));        // the vector form behind a 4-aligned pixel
        o = oko; o.f.W = 7; LAUNCHED(out(o));                               // the tail form
        o = oko; o.src = fl + 1; o.f.H = 4; LAUNCHED(out(o));               // an unaligned source
#undef LAUNCHED
    } else {
        std::printf("rgb32 axis host check: %d device(s) present: the accepted sets are not launched on host memory\n", devices);
    }
    std::printf("rgb32 axis host check: %d refusals and %d passes of the four entry points of the axis-aligned RGB32 edge, %d accepted sets up to the launch\n",
                refusals, passes, launched);
    return 0;
}
