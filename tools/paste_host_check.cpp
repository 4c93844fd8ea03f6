// Host-side check of the full-frame way out of csrc/frame_io.hip under AddressSanitizer / UBSan: the feather table at the sizes
// the tests and the benchmark use (tables sized exactly, so a write past one is caught; n = 1, n = 2, feather = 0 and
// feather >= n among them) and the argument validation of spk_frames_paste_u8 and spk_frames_u8_to_f32_boxes (every refusal
// happens before a launch, so no device is needed).  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/frame_io.hip tools/paste_host_check.cpp -o tools/_bin/paste_host_check
//   tools/_bin/paste_host_check
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_check.hpp"

int main() {
    const int sizes[] = {1, 2, 3, 9, 11, 20, 24, 32, 37, 53, 256, 264, 400, 1080, 1920};
    const double feathers[] = {0.0, 0.5, 2.0, 3.0, 4.0, 16.0, 40.0, 1000.0, 5000.0};
    int tables = 0;
    for (const int n : sizes)
        for (const double f : feathers) {
            std::vector<float> a(n);
            CHECK(spk_feather_table(n, f, a.data()) == SPK_OK);
            for (int i = 0; i < n; ++i) {
                const double want = std::min(1.0, (double)(std::min(i, n - 1 - i) + 1) / (f + 1.0));
                CHECK(a[i] == (float)want && a[i] == a[n - 1 - i] && a[i] > 0.f && a[i] <= 1.f);
                if (f == 0.0) CHECK(a[i] == 1.f);
                if (f >= n) CHECK(a[i] < 1.f);
            }
            ++tables;
        }
    float one;
    CHECK(spk_feather_table(0, 1.0, &one) == SPK_EINVAL);
    CHECK(spk_feather_table(-3, 1.0, &one) == SPK_EINVAL);
    CHECK(spk_feather_table(1, -0.5, &one) == SPK_EINVAL && std::strstr(spk_last_error(), "feather"));
    CHECK(spk_feather_table(1, NAN, &one) == SPK_EINVAL);
    CHECK(spk_feather_table(1, INFINITY, &one) == SPK_EINVAL);
    CHECK(spk_feather_table(1, 1.0, nullptr) == SPK_EINVAL);

    // the two launchers: every bad argument is refused before anything is dereferenced or launched
    uint8_t u8[4];
    float f[4];
    int32_t i4[4];
    struct PasteArgs {
        const float* src; uint8_t* dst; const int32_t* tab; const float* w; const float* ay; const float* ax;
        int N, Hs, Ws, H, W, h, w_, taps; int64_t img, row; float lo, k;
    };
    const PasteArgs ok = {f, u8, i4, f, nullptr, nullptr, 1, 4, 4, 8, 8, 4, 4, 2, 192, 24, -1.f, 127.5f};
    auto paste = [&](const PasteArgs& a) {
        return spk_frames_paste_u8(a.src, a.N, a.Hs, a.Ws, a.dst, a.img, a.row, a.H, a.W, a.h, a.w_, 0, 0, nullptr, 0, a.tab, a.tab, a.w,
                                   a.taps, a.tab, a.tab, a.w, a.taps, a.ay, a.ax, a.lo, a.k, nullptr);
    };
    PasteArgs a;
#define REFUSED(field, value) a = ok; a.field = value; CHECK(paste(a) == SPK_EINVAL)
    REFUSED(src, nullptr);
    REFUSED(dst, nullptr);
    REFUSED(tab, nullptr);
    REFUSED(w, nullptr);
    REFUSED(ay, f);                                          // one feather table without the other
    CHECK(std::strstr(spk_last_error(), "feather"));
    REFUSED(ax, f);
    REFUSED(N, 0);
    REFUSED(Hs, 0);
    REFUSED(Ws, -1);
    REFUSED(H, 0);
    REFUSED(W, 0);
    REFUSED(h, 0);
    REFUSED(w_, 0);
    REFUSED(taps, 0);
    REFUSED(row, 23);
    CHECK(std::strstr(spk_last_error(), "row stride"));
    REFUSED(W, 0x7fffffff);                                  // 3 * W does not wrap
    REFUSED(lo, NAN);
    REFUSED(k, 0.f);
    REFUSED(k, INFINITY);
    a = ok; a.N = 2; a.img = 191;                            // two frames of 8 rows of 24 bytes overlap below 192
    CHECK(paste(a) == SPK_EINVAL && std::strstr(spk_last_error(), "overlap"));
    a = ok; a.N = 2; a.img = 0;
    CHECK(paste(a) == SPK_EINVAL);
    a = ok; a.N = 2; a.img = -192;
    CHECK(paste(a) == SPK_EINVAL);
#undef REFUSED

    struct BoxArgs {
        const uint8_t* src; float* dst; const int32_t* tab; const float* w; const int32_t* boxes;
        int N, H, W, Hin, Win, taps, Hout, Wout; int64_t img, row;
    };
    const BoxArgs okb = {u8, f, i4, f, i4, 1, 8, 8, 4, 4, 2, 2, 2, 192, 24};
    auto boxes = [&](const BoxArgs& b) {
        return spk_frames_u8_to_f32_boxes(b.src, b.img, b.row, b.N, b.H, b.W, b.boxes, b.Hin, b.Win, 0, b.tab, b.tab, b.w, b.taps, b.tab, b.tab,
                                          b.w, b.taps, b.dst, b.Hout, b.Wout, 1.f, 1.f, 1.f, 0.f, 0.f, 0.f, nullptr);
    };
    BoxArgs b;
#define REFUSED(field, value) b = okb; b.field = value; CHECK(boxes(b) == SPK_EINVAL)
    REFUSED(src, nullptr);
    REFUSED(dst, nullptr);
    REFUSED(tab, nullptr);
    REFUSED(w, nullptr);
    REFUSED(boxes, nullptr);
    CHECK(std::strstr(spk_last_error(), "box"));
    REFUSED(N, 0);
    REFUSED(Hin, 0);
    REFUSED(Win, 0);
    REFUSED(Hin, 9);                                         // the box does not fit the frame
    CHECK(std::strstr(spk_last_error(), "does not fit"));
    REFUSED(Win, 9);
    REFUSED(H, 0);
    REFUSED(W, -8);
    REFUSED(taps, 0);
    REFUSED(Hout, 0);
    REFUSED(Wout, -1);
    REFUSED(row, 23);
    CHECK(std::strstr(spk_last_error(), "row stride"));
    REFUSED(W, 0x7fffffff);
    REFUSED(img, -1);
#undef REFUSED
    std::printf("paste host check: %d feather tables and the argument refusals of the two entry points passed\n", tables);
    return 0;
}
