// Host-side check of the NV12 video edge (csrc/frame_nv12.hip) under AddressSanitizer / UBSan: the colour matrices of
// spk_yuv_coeffs against their known answers, to_rgb o from_rgb = identity to 1e-12 for the four standard / range pairs (the
// matrices are written into arrays sized exactly, so a write past one is caught), and the argument validation of
// spk_frames_nv12_to_f32, spk_frames_f32_to_nv12 and spk_frames_paste_nv12 (every refusal happens before a launch, so no device is
// needed; the pointers are host buffers that are never dereferenced).  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/frame_nv12.hip tools/nv12_host_check.cpp -o tools/_bin/nv12_host_check
//   tools/_bin/nv12_host_check
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_check.hpp"

static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }

int main() {
    // ---- the colour matrices ----
    int matrices = 0;
    for (const int standard : {601, 709})
        for (const int full : {0, 1}) {
            std::vector<double> t(12), f(12);
            CHECK(spk_yuv_coeffs(standard, full, t.data(), f.data()) == SPK_OK);
            // 4 x 4 products of the affine maps, both ways
            for (int dir = 0; dir < 2; ++dir) {
                const double* A = dir ? f.data() : t.data();
                const double* B = dir ? t.data() : f.data();
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 4; ++c) {
                        double s = c == 3 ? A[4 * r + 3] : 0.0;
                        for (int k = 0; k < 3; ++k) s += A[4 * r + k] * B[4 * k + c];
                        CHECK(near(s, r == c ? 1.0 : 0.0, 1e-12));
                    }
            }
            const double kr = standard == 601 ? 0.299 : 0.2126, kb = standard == 601 ? 0.114 : 0.0722;
            const double sy = full ? 1.0 : 219.0 / 255.0;
            CHECK(near(f[0], sy * kr, 1e-15) && near(f[1], sy * (1.0 - kr - kb), 1e-15) && near(f[2], sy * kb, 1e-15));
            CHECK(f[3] == (full ? 0.0 : 16.0) && f[7] == 128.0 && f[11] == 128.0);
            CHECK(near(f[4] + f[5] + f[6], 0.0, 1e-15) && near(f[8] + f[9] + f[10], 0.0, 1e-15));      // grey has no chroma
            CHECK(near(f[6], full ? 0.5 : 112.0 / 255.0, 1e-15) && near(f[8], full ? 0.5 : 112.0 / 255.0, 1e-15));
            CHECK(t[1] == 0.0 && t[10] == 0.0 && t[0] == t[4] && t[4] == t[8]);
            // one pointer may be null
            std::vector<double> only(12);
            CHECK(spk_yuv_coeffs(standard, full, only.data(), nullptr) == SPK_OK && std::memcmp(only.data(), t.data(), 96) == 0);
            CHECK(spk_yuv_coeffs(standard, full, nullptr, only.data()) == SPK_OK && std::memcmp(only.data(), f.data(), 96) == 0);
            ++matrices;
        }
    double t[12], f[12];
    CHECK(spk_yuv_coeffs(601, 0, t, f) == SPK_OK);
    CHECK(near(t[0], 255.0 / 219.0, 1e-15) && near(t[2], 1.596027, 5e-7) && near(t[5], -0.391762, 5e-7) && near(t[6], -0.812968, 5e-7) &&
          near(t[9], 2.017232, 5e-7));
    CHECK(spk_yuv_coeffs(709, 0, t, f) == SPK_OK);
    CHECK(near(t[0], 255.0 / 219.0, 1e-15) && near(t[2], 1.792741, 5e-7) && near(t[5], -0.213249, 5e-7) && near(t[6], -0.532909, 5e-7) &&
          near(t[9], 2.112402, 5e-7));
    CHECK(spk_yuv_coeffs(2020, 0, t, f) == SPK_EINVAL && std::strstr(spk_last_error(), "601"));
    CHECK(spk_yuv_coeffs(0, 0, t, f) == SPK_EINVAL);
    CHECK(spk_yuv_coeffs(601, 2, t, f) == SPK_EINVAL && std::strstr(spk_last_error(), "full_range"));
    CHECK(spk_yuv_coeffs(601, -1, t, f) == SPK_EINVAL);
    CHECK(spk_yuv_coeffs(601, 0, nullptr, nullptr) == SPK_EINVAL);

    // ---- the three launchers: every bad argument is refused before anything is dereferenced or launched ----
    alignas(4) uint8_t u8[8];
    float fl[4];
    int32_t i4[4];
    struct Surface { uint8_t* y; uint8_t* uv; int N, H, W; int64_t yi, yr, ui, ur; int standard, full; };
    const Surface oks = {u8, u8 + 4, 1, 8, 8, 96, 8, 96, 8, 601, 0};

    struct InArgs { Surface s; float* dst; const int32_t* tab; const float* w; int Hin, Win, taps, Hout, Wout; };
    const InArgs oki = {oks, fl, i4, fl, 4, 4, 2, 2, 2};
    auto in = [&](const InArgs& a) {
        return spk_frames_nv12_to_f32(a.s.y, a.s.yi, a.s.yr, a.s.uv, a.s.ui, a.s.ur, a.s.N, a.s.H, a.s.W, nullptr, 1, 1, a.Hin, a.Win, 0, a.s.standard,
                                      a.s.full, a.tab, a.tab, a.w, a.taps, a.tab, a.tab, a.w, a.taps, a.dst, a.Hout, a.Wout, 1.f, 1.f, 1.f, 0.f, 0.f,
                                      0.f, nullptr);
    };
    struct PasteArgs { Surface s; const float* src; const int32_t* tab; const float* w; const float* ay; const float* ax; int Hs, Ws, h, w_, taps; float lo, k; };
    const PasteArgs okp = {oks, fl, i4, fl, nullptr, nullptr, 4, 4, 4, 4, 2, -1.f, 127.5f};
    auto paste = [&](const PasteArgs& a) {
        return spk_frames_paste_nv12(a.src, a.s.N, a.Hs, a.Ws, a.s.y, a.s.yi, a.s.yr, a.s.uv, a.s.ui, a.s.ur, a.s.H, a.s.W, a.h, a.w_, 1, 1, nullptr,
                                     a.s.standard, a.s.full, a.tab, a.tab, a.w, a.taps, a.tab, a.tab, a.w, a.taps, a.ay, a.ax, a.lo, a.k, nullptr);
    };
    struct OutArgs { Surface s; const float* src; float lo, k; };
    const OutArgs oko = {oks, fl, -1.f, 127.5f};
    auto out = [&](const OutArgs& a) {
        return spk_frames_f32_to_nv12(a.src, a.s.N, a.s.H, a.s.W, a.s.y, a.s.yi, a.s.yr, a.s.uv, a.s.ui, a.s.ur, a.s.standard, a.s.full, a.lo, a.k, nullptr);
    };
    InArgs a;
    PasteArgs p;
    OutArgs o;
    int refusals = 0;
    // what every surface argument gets, through each of the three entry points
#define SURFACE_REFUSED(field, value, word)                                                                  \
    a = oki; a.s.field = value; CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));           \
    p = okp; p.s.field = value; CHECK(paste(p) == SPK_EINVAL && std::strstr(spk_last_error(), word));        \
    o = oko; o.s.field = value; CHECK(out(o) == SPK_EINVAL && std::strstr(spk_last_error(), word));          \
    refusals += 3
    SURFACE_REFUSED(y, nullptr, "null");
    SURFACE_REFUSED(uv, nullptr, "null");
    SURFACE_REFUSED(N, 0, "N must be");
    SURFACE_REFUSED(N, -2, "N must be");
    SURFACE_REFUSED(H, 0, "N must be");
    SURFACE_REFUSED(W, -8, "N must be");
    SURFACE_REFUSED(H, 7, "even");
    SURFACE_REFUSED(W, 9, "even");
    SURFACE_REFUSED(uv, u8 + 5, "aligned");
    SURFACE_REFUSED(ur, 9, "UV strides");
    SURFACE_REFUSED(ui, 97, "UV strides");
    SURFACE_REFUSED(yr, 7, "row stride");
    SURFACE_REFUSED(ur, 6, "row stride");
    SURFACE_REFUSED(W, 0x7ffffffe, "row stride");              // (an even W that no stride holds)
    SURFACE_REFUSED(standard, 2020, "standard");
    SURFACE_REFUSED(full, 2, "full_range");
#undef SURFACE_REFUSED

#define REFUSED(var, ok, call, field, value) var = ok; var.field = value; CHECK(call(var) == SPK_EINVAL); ++refusals
    REFUSED(a, oki, in, dst, nullptr);
    REFUSED(a, oki, in, tab, nullptr);
    REFUSED(a, oki, in, w, nullptr);
    REFUSED(a, oki, in, Hin, 0);
    REFUSED(a, oki, in, Win, -1);
    REFUSED(a, oki, in, Hin, 9);                                // the box does not fit the frame
    CHECK(std::strstr(spk_last_error(), "does not fit"));
    REFUSED(a, oki, in, Win, 9);
    REFUSED(a, oki, in, taps, 0);
    REFUSED(a, oki, in, Hout, 0);
    REFUSED(a, oki, in, Wout, -1);
    REFUSED(a, oki, in, s.yi, -1);
    REFUSED(a, oki, in, s.ui, -2);

    REFUSED(p, okp, paste, src, nullptr);
    REFUSED(p, okp, paste, tab, nullptr);
    REFUSED(p, okp, paste, w, nullptr);
    REFUSED(p, okp, paste, ay, fl);                             // one feather table without the other
    CHECK(std::strstr(spk_last_error(), "feather"));
    REFUSED(p, okp, paste, ax, fl);
    REFUSED(p, okp, paste, Hs, 0);
    REFUSED(p, okp, paste, Ws, -1);
    REFUSED(p, okp, paste, h, 0);
    REFUSED(p, okp, paste, w_, 0);
    REFUSED(p, okp, paste, taps, 0);
    REFUSED(p, okp, paste, lo, NAN);
    REFUSED(p, okp, paste, k, 0.f);
    REFUSED(p, okp, paste, k, INFINITY);
    p = okp; p.s.N = 2; p.s.yi = 63;                            // two Y planes of 8 rows of 8 bytes overlap below 64
    CHECK(paste(p) == SPK_EINVAL && std::strstr(spk_last_error(), "overlap"));
    p = okp; p.s.N = 2; p.s.ui = 30;                            // two UV planes of 4 rows of 8 bytes overlap below 32
    CHECK(paste(p) == SPK_EINVAL && std::strstr(spk_last_error(), "overlap"));
    p = okp; p.s.N = 2; p.s.yi = 0;
    CHECK(paste(p) == SPK_EINVAL);
    p = okp; p.s.N = 2; p.s.yi = -96;
    CHECK(paste(p) == SPK_EINVAL);
    refusals += 4;

    REFUSED(o, oko, out, src, nullptr);
    REFUSED(o, oko, out, lo, INFINITY);
    REFUSED(o, oko, out, k, -1.f);
    REFUSED(o, oko, out, k, NAN);
    o = oko; o.s.N = 2; o.s.yi = 63;
    CHECK(out(o) == SPK_EINVAL && std::strstr(spk_last_error(), "overlap"));
    o = oko; o.s.N = 2; o.s.ui = 30;
    CHECK(out(o) == SPK_EINVAL);
    refusals += 2;
#undef REFUSED
    std::printf("nv12 host check: %d colour matrices, the known answers and %d argument refusals of the three entry points passed\n", matrices,
                refusals);
    return 0;
}
