// Host-side check of the axis-aligned I420 edge (csrc/frame_i420.hip) under AddressSanitizer / UBSan: every refusal of
// spk_frames_i420_to_f32, spk_frames_paste_i420 and spk_frames_f32_to_i420 -- the surface checks through each of the three (null
// planes, N, odd or small H / W, row strides below the row, a W no stride holds), the strides whose extents leave 32 bits (the
// arithmetic is 64-bit: nothing wraps), overlapping written frames, negative strides of read ones, and each entry point's own
// arguments -- and the surfaces that must PASS the surface check: an odd chroma pitch, an odd chroma base, an odd image stride, V
// before U in memory, planes in separate allocations, frames that touch.  Every refusal happens before a launch and before anything
// is dereferenced, so no device is needed; a surface that passes would be launched, so a pass is shown by the refusal of the
// argument that is checked BEHIND the surface (the way in: the output pointer; the two ways out: the value range), by its message.
// The file is linked with nothing else: what it shares with csrc/frame_nv12.hip lives in headers, and the colour maps come from the
// inline routine of csrc/frame_nv12_common.hpp.  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/frame_i420.hip tools/i420_axis_host_check.cpp -o tools/_bin/i420_axis_host_check
//   tools/_bin/i420_axis_host_check
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    alignas(16) static uint8_t raw[4096];
    alignas(16) static uint8_t apart[64];                                 // a second allocation
    float fl[4];
    int32_t i4[4];
    int refusals = 0, passes = 0;

    // One 8 x 8 surface: Y 8 rows of 8 bytes; U 4 rows of 4 bytes at the ODD pitch 5 from the ODD address raw + 129, its frames an
    // odd 21 bytes apart; V 4 rows at pitch 4
    struct Surface { uint8_t* y; uint8_t* u; uint8_t* v; int N, H, W; int64_t yi, yr, ui, ur, vi, vr; int standard, full; };
    const Surface oks = {raw, raw + 129, raw + 256, 1, 8, 8, 96, 8, 21, 5, 16, 4, 601, 0};
    struct InArgs { Surface s; float* dst; const int32_t* tab; const float* w; int Hin, Win, taps, Hout, Wout; };
    const InArgs oki = {oks, fl, i4, fl, 4, 4, 2, 2, 2};
    auto in = [&](const InArgs& a) {
        return spk_frames_i420_to_f32(a.s.y, a.s.yi, a.s.yr, a.s.u, a.s.ui, a.s.ur, a.s.v, a.s.vi, a.s.vr, a.s.N, a.s.H, a.s.W, nullptr, 1, 1, a.Hin, a.Win,
                                      0, a.s.standard, a.s.full, a.tab, a.tab, a.w, a.taps, a.tab, a.tab, a.w, a.taps, a.dst, a.Hout, a.Wout, 1.f, 1.f,
                                      1.f, 0.f, 0.f, 0.f, nullptr);
    };
    struct PasteArgs { Surface s; const float* src; const int32_t* tab; const float* w; const float* ay; const float* ax; int Hs, Ws, h, w_, taps; float lo, k; };
    const PasteArgs okp = {oks, fl, i4, fl, nullptr, nullptr, 4, 4, 4, 4, 2, -1.f, 127.5f};
    auto paste = [&](const PasteArgs& a) {
        return spk_frames_paste_i420(a.src, a.s.N, a.Hs, a.Ws, a.s.y, a.s.yi, a.s.yr, a.s.u, a.s.ui, a.s.ur, a.s.v, a.s.vi, a.s.vr, a.s.H, a.s.W, a.h,
                                     a.w_, 1, 1, nullptr, a.s.standard, a.s.full, a.tab, a.tab, a.w, a.taps, a.tab, a.tab, a.w, a.taps, a.ay, a.ax, a.lo,
                                     a.k, nullptr);
    };
    struct OutArgs { Surface s; const float* src; float lo, k; };
    const OutArgs oko = {oks, fl, -1.f, 127.5f};
    auto out = [&](const OutArgs& a) {
        return spk_frames_f32_to_i420(a.src, a.s.N, a.s.H, a.s.W, a.s.y, a.s.yi, a.s.yr, a.s.u, a.s.ui, a.s.ur, a.s.v, a.s.vi, a.s.vr, a.s.standard,
                                      a.s.full, a.lo, a.k, nullptr);
    };
    InArgs a;
    PasteArgs p;
    OutArgs o;

    // ---- what every surface argument gets, through each of the three entry points
#define SURFACE_REFUSED(stmt, word)                                                                                \
    a = oki; { Surface& s = a.s; stmt; } CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));       \
    p = okp; { Surface& s = p.s; stmt; } CHECK(paste(p) == SPK_EINVAL && std::strstr(spk_last_error(), word));    \
    o = oko; { Surface& s = o.s; stmt; } CHECK(out(o) == SPK_EINVAL && std::strstr(spk_last_error(), word));      \
    refusals += 3
    SURFACE_REFUSED(s.y = nullptr, "plane pointer");
    SURFACE_REFUSED(s.u = nullptr, "plane pointer");
    SURFACE_REFUSED(s.v = nullptr, "plane pointer");
    SURFACE_REFUSED(s.N = 0, "N must");
    SURFACE_REFUSED(s.N = -3, "N must");
    SURFACE_REFUSED(s.H = 0, "N must");
    SURFACE_REFUSED(s.W = -8, "N must");
    SURFACE_REFUSED(s.H = 7, "even");                                     // odd H
    SURFACE_REFUSED(s.W = 9, "even");                                     // odd W
    SURFACE_REFUSED(s.yr = 7, "Y row stride");
    SURFACE_REFUSED(s.ur = 3, "U row stride");
    SURFACE_REFUSED(s.vr = 3, "V row stride");
    SURFACE_REFUSED(s.vr = -4, "V row stride");
    SURFACE_REFUSED(s.W = 0x7ffffffe, "Y row stride");                    // an even W that no stride holds
    SURFACE_REFUSED((s.W = 0x7ffffffe, s.yr = 0x7ffffffe), "U row stride");      // W / 2 = 2^30 - 1 against the pitch 5
    SURFACE_REFUSED(s.standard = 2020, "standard");
    SURFACE_REFUSED(s.standard = 0, "standard");
    SURFACE_REFUSED(s.full = 2, "full_range");
    SURFACE_REFUSED(s.full = -1, "full_range");
#undef SURFACE_REFUSED

    // ---- two frames: a negative stride for the one that reads; frames that overlap for the two that write
#define READ_REFUSED(stmt, word) a = oki; a.s.N = 2; { Surface& s = a.s; stmt; } CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    READ_REFUSED(s.yi = -96, "negative");
    READ_REFUSED(s.ui = -21, "negative");
    READ_REFUSED(s.vi = -1, "negative");
#undef READ_REFUSED
#define WRITTEN_REFUSED(stmt, word)                                                                                              \
    p = okp; p.s.N = 2; { Surface& s = p.s; stmt; } CHECK(paste(p) == SPK_EINVAL && std::strstr(spk_last_error(), word));       \
    o = oko; o.s.N = 2; { Surface& s = o.s; stmt; } CHECK(out(o) == SPK_EINVAL && std::strstr(spk_last_error(), word));         \
    refusals += 2
    WRITTEN_REFUSED(s.yi = 63, "overlap");                                // two Y planes of 8 rows of 8 bytes overlap below 64
    WRITTEN_REFUSED(s.ui = 18, "overlap");                                // a U plane of 4 rows at pitch 5 ends at 19
    WRITTEN_REFUSED(s.vi = 15, "overlap");                                // a V plane of 4 rows at pitch 4 ends at 16
    WRITTEN_REFUSED(s.yi = 0, "overlap");
    WRITTEN_REFUSED(s.vi = 0, "overlap");
    WRITTEN_REFUSED(s.ui = -21, "overlap");
    // extents that leave 32 bits: (rows - 1) * row stride + width is formed in 64 bits, so a stride that a wrapped extent would let
    // through is refused
    WRITTEN_REFUSED((s.H = 0x7ffffffe, s.yi = 64), "overlap");            // the Y extent is 2^34 - 16, which 32 bits do not hold
    WRITTEN_REFUSED((s.H = 0x7ffffffe, s.yi = ((int64_t)1 << 34) - 16, s.ui = (int64_t)1 << 32), "overlap");     // Y fits; the U extent 5 * 2^30 - 6 > 2^32
    WRITTEN_REFUSED((s.H = 0x7ffffffe, s.yi = ((int64_t)1 << 34) - 16, s.ui = (int64_t)1 << 33, s.vi = (int64_t)1 << 31), "overlap");   // the V extent 2^32 - 4
    WRITTEN_REFUSED((s.yr = (int64_t)1 << 31, s.yi = (int64_t)1 << 31), "overlap");                              // 7 * 2^31 + 8
    WRITTEN_REFUSED((s.ur = ((int64_t)1 << 32) + 1, s.ui = 19), "overlap");                                      // 3 * (2^32 + 1) + 4: 19 if the pitch wrapped
#undef WRITTEN_REFUSED

    // ---- each entry point's own arguments
#define REFUSED(var, ok, call, field, value, word) var = ok; var.field = value; CHECK(call(var) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED(a, oki, in, dst, nullptr, "null frame pointer");
    REFUSED(a, oki, in, tab, nullptr, "table");
    REFUSED(a, oki, in, w, nullptr, "table");
    REFUSED(a, oki, in, Hin, 0, "sizes must be");
    REFUSED(a, oki, in, Win, -1, "sizes must be");
    REFUSED(a, oki, in, Hin, 9, "does not fit");                          // the box does not fit the frame
    REFUSED(a, oki, in, Win, 9, "does not fit");
    REFUSED(a, oki, in, taps, 0, "tap count");
    REFUSED(a, oki, in, Hout, 0, "sizes must be");
    REFUSED(a, oki, in, Wout, -1, "sizes must be");

    REFUSED(p, okp, paste, src, nullptr, "null frame pointer");
    REFUSED(p, okp, paste, tab, nullptr, "table");
    REFUSED(p, okp, paste, w, nullptr, "table");
    REFUSED(p, okp, paste, ay, fl, "feather");                            // one feather table without the other
    REFUSED(p, okp, paste, ax, fl, "feather");
    REFUSED(p, okp, paste, Hs, 0, "sizes must be");
    REFUSED(p, okp, paste, Ws, -1, "sizes must be");
    REFUSED(p, okp, paste, h, 0, "sizes must be");
    REFUSED(p, okp, paste, w_, 0, "sizes must be");
    REFUSED(p, okp, paste, taps, 0, "tap count");
    REFUSED(p, okp, paste, lo, NAN, "value range");
    REFUSED(p, okp, paste, k, 0.f, "value range");
    REFUSED(p, okp, paste, k, INFINITY, "value range");

    REFUSED(o, oko, out, src, nullptr, "null frame pointer");
    REFUSED(o, oko, out, lo, INFINITY, "value range");
    REFUSED(o, oko, out, k, -1.f, "value range");
    REFUSED(o, oko, out, k, NAN, "value range");
#undef REFUSED

    // ---- the surfaces that must pass: each is let through by the surface check of all three, which shows in the refusal BEHIND it
#define PASSES(stmt)                                                                                                                      \
    a = oki; a.dst = nullptr; { Surface& s = a.s; stmt; } CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), "null frame pointer")); \
    p = okp; p.k = 0.f; { Surface& s = p.s; stmt; } CHECK(paste(p) == SPK_EINVAL && std::strstr(spk_last_error(), "value range"));           \
    o = oko; o.k = 0.f; { Surface& s = o.s; stmt; } CHECK(out(o) == SPK_EINVAL && std::strstr(spk_last_error(), "value range"));             \
    passes += 3
    PASSES((void)s);                                                      // as it is: U at an odd pitch from an odd address
    PASSES((s.u = raw + 301, s.ur = 7, s.v = raw + 131, s.vr = 5));       // V BEFORE U, both odd, pitches that differ
    PASSES((s.u = raw + 256, s.v = raw + 129, s.ur = 4, s.vr = 4));       // YV12: the planes swapped
    PASSES((s.u = apart + 1, s.v = apart + 33, s.ur = 4, s.vr = 4));      // chroma in a separate allocation
    PASSES((s.H = 2, s.W = 2, s.yr = 2, s.ur = 1, s.vr = 1));             // the smallest surface: one chroma sample at pitch 1
    PASSES((s.H = 4, s.W = 6, s.yr = 6, s.ur = 3, s.vr = 3));             // W / 2 odd, packed: the odd pitch 3
    PASSES((s.N = 2, s.yi = 64, s.ui = 19, s.vi = 16));                   // two frames that touch: the extents themselves, U's odd
    PASSES((s.N = 2, s.yi = 97, s.ui = 21, s.vi = 17));                   // odd image strides
#undef PASSES
    std::printf("i420 axis host check: %d refusals and %d passes of the three entry points of the axis-aligned I420 edge\n", refusals, passes);
    return 0;
}
