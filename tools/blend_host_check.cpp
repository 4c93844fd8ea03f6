// Host-side check of the seamless paste-back of csrc/frame_blend.hip under AddressSanitizer / UBSan: the argument validation of
// spk_frames_paste_u8_sim_blend, spk_paste_colour_match_workspace_bytes and spk_paste_colour_match_sim -- every refusal happens
// before a launch and before anything is dereferenced, so no device is needed -- with the sizes whose products would wrap a
// 32-bit int.  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/frame_blend.hip tools/blend_host_check.cpp -o tools/_bin/blend_host_check
//   tools/_bin/blend_host_check
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    alignas(8) uint8_t u8[16];
    float f[4];
    int refusals = 0;

    struct Args {
        const float* src; uint8_t* dst; const float* sim;
        int N, Hs, Ws, H, W; int64_t img, row; double feather; float lo, k;
        const float* matte; int matte_frames;
        // the statistics only
        double max_gain, min_sigma, min_weight; float* out; void* ws; size_t ws_bytes;
    };
    const size_t need1 = (size_t)spk_paste_colour_match_workspace_bytes(1), need2 = (size_t)spk_paste_colour_match_workspace_bytes(2);
    const Args ok = {f, u8, f, 1, 4, 4, 8, 8, 192, 24, 0.0, -1.f, 127.5f, nullptr, 0, 2.0, 1.0, 16.0, f, u8, need2};
    auto blend = [&](const Args& a) {
        return spk_frames_paste_u8_sim_blend(a.src, a.N, a.Hs, a.Ws, a.dst, a.img, a.row, a.H, a.W, a.sim, 0, a.feather, a.lo, a.k, a.matte,
                                             a.matte_frames, nullptr, nullptr);
    };
    auto match = [&](const Args& a) {
        return spk_paste_colour_match_sim(a.src, a.N, a.Hs, a.Ws, a.dst, a.img, a.row, a.H, a.W, a.sim, 0, a.feather, a.lo, a.k, a.matte,
                                          a.matte_frames, a.max_gain, a.min_sigma, a.min_weight, a.out, a.ws, a.ws_bytes, nullptr);
    };

    CHECK(spk_paste_colour_match_workspace_bytes(0) == -1);
    CHECK(spk_paste_colour_match_workspace_bytes(-7) == -1);
    CHECK(need1 > 0 && need1 % (13 * sizeof(double)) == 0 && need2 == 2 * need1);
    CHECK(spk_paste_colour_match_workspace_bytes(0x7fffffff) == (int64_t)0x7fffffff * (int64_t)need1);      // no 32-bit wrap
    refusals += 2;

    Args a;
    // what both entry points refuse alike
#define REFUSED(field, value)                                             \
    a = ok; a.field = value; CHECK(blend(a) == SPK_EINVAL);               \
    a = ok; a.field = value; CHECK(match(a) == SPK_EINVAL); refusals += 2
    REFUSED(src, nullptr);
    REFUSED(dst, nullptr);
    REFUSED(sim, nullptr);
    CHECK(std::strstr(spk_last_error(), "transform"));
    REFUSED(N, 0);
    REFUSED(N, -3);
    REFUSED(Hs, 0);
    REFUSED(Ws, -1);
    REFUSED(H, 0);
    REFUSED(W, 0);
    REFUSED(row, 23);
    CHECK(std::strstr(spk_last_error(), "row stride"));
    REFUSED(W, 0x7fffffff);                                  // 3 * W does not wrap
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
#undef REFUSED
    // two frames: overlapping strides, and a matte of neither 1 nor N frames
#define REFUSED2(stmt)                                                    \
    a = ok; a.N = 2; stmt; CHECK(blend(a) == SPK_EINVAL);                 \
    a = ok; a.N = 2; stmt; CHECK(match(a) == SPK_EINVAL); refusals += 2
    REFUSED2(a.img = 191);                                   // two frames of 8 rows of 24 bytes overlap below 192
    CHECK(std::strstr(spk_last_error(), "overlap"));
    REFUSED2(a.img = 0);
    REFUSED2(a.img = -192);
    REFUSED2((a.H = 0x7fffffff, a.img = 192));               // (H - 1) * row_stride does not wrap
    REFUSED2((a.matte = f, a.matte_frames = 0));
    REFUSED2((a.matte = f, a.matte_frames = 3));
    REFUSED2((a.N = 3, a.img = 192, a.matte = f, a.matte_frames = 2));
    CHECK(std::strstr(spk_last_error(), "matte_frames"));
#undef REFUSED2

    // the statistics' own arguments
#define REFUSED(field, value) a = ok; a.field = value; CHECK(match(a) == SPK_EINVAL); ++refusals
    REFUSED(max_gain, 0.999);
    CHECK(std::strstr(spk_last_error(), "max_gain"));
    REFUSED(max_gain, NAN);
    REFUSED(max_gain, INFINITY);
    REFUSED(min_sigma, -1e-9);
    CHECK(std::strstr(spk_last_error(), "min_sigma"));
    REFUSED(min_sigma, NAN);
    REFUSED(min_sigma, INFINITY);
    REFUSED(min_weight, -1.0);
    CHECK(std::strstr(spk_last_error(), "min_weight"));
    REFUSED(min_weight, NAN);
    REFUSED(min_weight, INFINITY);
    REFUSED(out, nullptr);
    REFUSED(ws, nullptr);
    CHECK(std::strstr(spk_last_error(), "workspace"));
    REFUSED(ws_bytes, need1 - 1);
    REFUSED(ws_bytes, 0);
    REFUSED(ws, u8 + 4);                                     // not aligned for doubles
    CHECK(std::strstr(spk_last_error(), "aligned"));
    a = ok; a.N = 2; a.img = 192; a.ws_bytes = need1;        // two frames need twice the bytes
    CHECK(match(a) == SPK_EINVAL && std::strstr(spk_last_error(), "workspace"));
    ++refusals;
#undef REFUSED
    std::printf("blend host check: %d argument refusals of the three entry points passed\n", refusals);
    return 0;
}
