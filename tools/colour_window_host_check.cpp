// Host-side check of the colour rows pooled over a frame window under AddressSanitizer / UBSan: the argument validation of
// spk_paste_colour_sums_sim (csrc/frame_blend.hip), spk_paste_colour_sums_nv12_sim (csrc/frame_sim_nv12.hip) and
// spk_colour_rows_window (csrc/colour_window.hip) -- every refusal happens before a launch and before anything is dereferenced, so
// no device is needed -- with the sizes whose sums and products would wrap a 32-bit int.  The three files are linked together and
// with nothing else: what they share lives in headers.  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/frame_blend.hip speak-hack_amd/csrc/frame_sim_nv12.hip speak-hack_amd/csrc/colour_window.hip \
//         tools/colour_window_host_check.cpp -o tools/_bin/colour_window_host_check
//   tools/_bin/colour_window_host_check
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    alignas(8) uint8_t u8[16];
    alignas(8) double d[2];
    float f[4];
    int refusals = 0;
    const size_t need1 = (size_t)spk_paste_colour_match_workspace_bytes(1), need2 = (size_t)spk_paste_colour_match_workspace_bytes(2);

    // ---- the sums of packed frames: one 8 x 8 frame of 24-byte rows
    struct Rgb {
        const float* src; const uint8_t* dst; const float* sim;
        int N, Hs, Ws, H, W; int64_t img, row; double feather; float lo, k;
        const float* matte; int matte_frames; double* out; void* ws; size_t ws_bytes;
    };
    const Rgb rgb_ok = {f, u8, f, 1, 4, 4, 8, 8, 192, 24, 0.0, -1.f, 127.5f, nullptr, 0, d, u8, need2};
    auto rgb = [&](const Rgb& a) {
        return spk_paste_colour_sums_sim(a.src, a.N, a.Hs, a.Ws, a.dst, a.img, a.row, a.H, a.W, a.sim, 0, a.feather, a.lo, a.k, a.matte,
                                         a.matte_frames, a.out, a.ws, a.ws_bytes, nullptr);
    };
    // ---- the sums of surfaces: one 8 x 8 surface, a Y plane of 8 rows of 8 bytes, a UV plane of 4 rows of 8 bytes
    struct Nv12 {
        const float* src; const uint8_t* y; const uint8_t* uv; const float* sim;
        int N, Hs, Ws, H, W; int64_t y_img, y_row, uv_img, uv_row; int standard, full_range; double feather; float lo, k;
        const float* matte; int matte_frames; double* out; void* ws; size_t ws_bytes;
    };
    const Nv12 nv_ok = {f, u8, u8, f, 1, 4, 4, 8, 8, 64, 8, 32, 8, 601, 0, 0.0, -1.f, 127.5f, nullptr, 0, d, u8, need2};
    auto nv12 = [&](const Nv12& a) {
        return spk_paste_colour_sums_nv12_sim(a.src, a.N, a.Hs, a.Ws, a.y, a.y_img, a.y_row, a.uv, a.uv_img, a.uv_row, a.H, a.W, a.sim, a.standard,
                                              a.full_range, a.feather, a.lo, a.k, a.matte, a.matte_frames, a.out, a.ws, a.ws_bytes, nullptr);
    };

    Rgb a;
    Nv12 b;
    // what both refuse alike
#define REFUSED(field, value)                                             \
    a = rgb_ok; a.field = value; CHECK(rgb(a) == SPK_EINVAL);             \
    b = nv_ok; b.field = value; CHECK(nv12(b) == SPK_EINVAL); refusals += 2
    REFUSED(src, nullptr);
    REFUSED(sim, nullptr);
    CHECK(std::strstr(spk_last_error(), "transform"));
    REFUSED(N, 0);
    REFUSED(N, -3);
    REFUSED(Hs, 0);
    REFUSED(Ws, -1);
    REFUSED(H, 0);
    REFUSED(W, 0);
    REFUSED(W, 0x7fffffff);
    REFUSED(feather, -0.5);
    CHECK(std::strstr(spk_last_error(), "feather"));
    REFUSED(feather, NAN);
    REFUSED(feather, INFINITY);
    REFUSED(lo, NAN);
    REFUSED(k, 0.f);
    REFUSED(k, INFINITY);
    REFUSED(matte_frames, 1);                                // frames of a matte that is not there
    CHECK(std::strstr(spk_last_error(), "matte_frames"));
    REFUSED(matte_frames, -1);
    REFUSED(out, nullptr);
    CHECK(std::strstr(spk_last_error(), "sums"));
    REFUSED(out, (double*)(u8 + 4));                         // not aligned for doubles
    CHECK(std::strstr(spk_last_error(), "aligned"));
    REFUSED(ws, nullptr);
    CHECK(std::strstr(spk_last_error(), "workspace"));
    REFUSED(ws, u8 + 4);
    CHECK(std::strstr(spk_last_error(), "aligned"));
    REFUSED(ws_bytes, need1 - 1);
    REFUSED(ws_bytes, 0);
#undef REFUSED
    // the pixel format's own
#define REFUSED(var, ok, call, stmt) var = ok; stmt; CHECK(call(var) == SPK_EINVAL); ++refusals
    REFUSED(a, rgb_ok, rgb, a.dst = nullptr);
    REFUSED(a, rgb_ok, rgb, a.row = 23);
    CHECK(std::strstr(spk_last_error(), "row stride"));
    REFUSED(a, rgb_ok, rgb, (a.N = 2, a.img = 191));         // two frames of 8 rows of 24 bytes overlap below 192
    CHECK(std::strstr(spk_last_error(), "overlap"));
    REFUSED(a, rgb_ok, rgb, (a.N = 2, a.H = 0x7fffffff));    // (H - 1) * row_stride does not wrap
    REFUSED(a, rgb_ok, rgb, (a.N = 2, a.ws_bytes = need1));  // two frames need twice the bytes
    CHECK(std::strstr(spk_last_error(), "workspace"));
    REFUSED(a, rgb_ok, rgb, (a.N = 2, a.matte = f, a.matte_frames = 3));
    REFUSED(b, nv_ok, nv12, b.y = nullptr);
    REFUSED(b, nv_ok, nv12, b.uv = nullptr);
    REFUSED(b, nv_ok, nv12, b.uv = u8 + 1);                  // a (U, V) pair is 2-byte aligned
    REFUSED(b, nv_ok, nv12, b.H = 7);
    REFUSED(b, nv_ok, nv12, b.W = 6 + 1);
    REFUSED(b, nv_ok, nv12, b.y_row = 7);
    REFUSED(b, nv_ok, nv12, b.uv_row = 7);
    REFUSED(b, nv_ok, nv12, b.standard = 2020);
    CHECK(std::strstr(spk_last_error(), "standard"));
    REFUSED(b, nv_ok, nv12, b.full_range = 2);
    REFUSED(b, nv_ok, nv12, (b.N = 2, b.y_img = -64));
    REFUSED(b, nv_ok, nv12, (b.N = 2, b.ws_bytes = need1));
    REFUSED(b, nv_ok, nv12, (b.N = 2, b.matte = f, b.matte_frames = 3));
#undef REFUSED

    // ---- rows from a window of sums
    struct Win { const double* sums; int T, n0, n, radius; double sigma, max_gain, min_sigma, min_weight; float* out; };
    const Win win_ok = {d, 7, 0, 7, 2, 1.0, 2.0, 1.0, 16.0, f};
    auto window = [&](const Win& w) {
        return spk_colour_rows_window(w.sums, w.T, w.n0, w.n, w.radius, w.sigma, w.max_gain, w.min_sigma, w.min_weight, w.out, nullptr);
    };
    Win w;
#define REFUSED(stmt) w = win_ok; stmt; CHECK(window(w) == SPK_EINVAL); ++refusals
    REFUSED(w.sums = nullptr);
    REFUSED(w.out = nullptr);
    REFUSED(w.sums = (const double*)(u8 + 4));
    CHECK(std::strstr(spk_last_error(), "aligned"));
    REFUSED(w.T = 0);
    REFUSED(w.T = -7);
    REFUSED(w.n = 0);
    REFUSED(w.n = -1);
    REFUSED(w.n0 = -1);
    REFUSED(w.n0 = 1);                                       // [1, 8) of a clip of 7
    CHECK(std::strstr(spk_last_error(), "range"));
    REFUSED(w.n = 8);
    REFUSED((w.n0 = 7, w.n = 1));
    REFUSED((w.n0 = 0x7fffffff, w.n = 1));                   // n0 + n does not wrap
    REFUSED((w.n0 = 1, w.n = 0x7fffffff));
    REFUSED((w.T = 0x7fffffff, w.n0 = 0x7fffffff, w.n = 0x7fffffff));
    REFUSED(w.radius = -1);
    REFUSED(w.radius = 65);
    CHECK(std::strstr(spk_last_error(), "radius"));
    REFUSED(w.radius = 0x7fffffff);
    REFUSED(w.sigma = 0.0);
    CHECK(std::strstr(spk_last_error(), "sigma"));
    REFUSED(w.sigma = -1.0);
    REFUSED(w.sigma = NAN);
    REFUSED(w.sigma = INFINITY);
    REFUSED(w.max_gain = 0.999);
    CHECK(std::strstr(spk_last_error(), "max_gain"));
    REFUSED(w.max_gain = NAN);
    REFUSED(w.max_gain = INFINITY);
    REFUSED(w.min_sigma = -1e-9);
    CHECK(std::strstr(spk_last_error(), "min_sigma"));
    REFUSED(w.min_sigma = NAN);
    REFUSED(w.min_sigma = INFINITY);
    REFUSED(w.min_weight = -1.0);
    CHECK(std::strstr(spk_last_error(), "min_weight"));
    REFUSED(w.min_weight = NAN);
    REFUSED(w.min_weight = INFINITY);
#undef REFUSED
    std::printf("colour window host check: %d argument refusals of the three entry points passed\n", refusals);
    return 0;
}
