// Host-side check of the aligned NV12 edge of csrc/frame_sim_nv12.hip under AddressSanitizer / UBSan: the argument validation of
// spk_frames_nv12_to_f32_sim, spk_frames_paste_nv12_sim and spk_paste_colour_match_nv12_sim -- every refusal happens before a
// launch and before anything is dereferenced, so no device is needed -- with the sizes whose products would wrap a 32-bit int.
// The file is linked ALONE: what it shares with csrc/frame_blend.hip and csrc/frame_nv12.hip lives in headers.  Build and run from
// the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/frame_sim_nv12.hip tools/sim_nv12_host_check.cpp -o tools/_bin/sim_nv12_host_check
//   tools/_bin/sim_nv12_host_check
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    alignas(8) uint8_t u8[16];
    float f[4];
    int refusals = 0;

    // one 8 x 8 surface: a Y plane of 8 rows of 8 bytes (64 per frame), a UV plane of 4 rows of 8 bytes (32 per frame)
    struct Args {
        const float* src; uint8_t* y; uint8_t* uv; const float* sim; float* dst;
        int N, Hs, Ws, H, W; int64_t y_img, y_row, uv_img, uv_row; int standard, full_range; double feather; float lo, k;
        const float* matte; int matte_frames;
        // the statistics only
        double max_gain, min_sigma, min_weight; float* out; void* ws; size_t ws_bytes;
    };
    const size_t need1 = 64 * 13 * sizeof(double);           // PASTE_WGS partials of 13 sums: spk_paste_colour_match_workspace_bytes(1)
    const Args ok = {f, u8, u8 + 8, f, f, 1, 4, 4, 8, 8, 64, 8, 32, 8, 601, 0, 0.0, -1.f, 127.5f, nullptr, 0, 2.0, 1.0, 16.0, f, u8, 2 * need1};
    auto in = [&](const Args& a) {
        return spk_frames_nv12_to_f32_sim(a.y, a.y_img, a.y_row, a.uv, a.uv_img, a.uv_row, a.N, a.H, a.W, a.sim, 0, a.standard, a.full_range, a.dst,
                                          a.Hs, a.Ws, 1.f, 1.f, 1.f, 0.f, 0.f, 0.f, nullptr);
    };
    auto paste = [&](const Args& a) {
        return spk_frames_paste_nv12_sim(a.src, a.N, a.Hs, a.Ws, a.y, a.y_img, a.y_row, a.uv, a.uv_img, a.uv_row, a.H, a.W, a.sim, a.standard,
                                         a.full_range, a.feather, a.lo, a.k, a.matte, a.matte_frames, nullptr, nullptr);
    };
    auto match = [&](const Args& a) {
        return spk_paste_colour_match_nv12_sim(a.src, a.N, a.Hs, a.Ws, a.y, a.y_img, a.y_row, a.uv, a.uv_img, a.uv_row, a.H, a.W, a.sim, a.standard,
                                               a.full_range, a.feather, a.lo, a.k, a.matte, a.matte_frames, a.max_gain, a.min_sigma, a.min_weight,
                                               a.out, a.ws, a.ws_bytes, nullptr);
    };

    Args a;
    // what all three entry points refuse alike: the surface, the rows, the sizes, the standard
#define REFUSED(field, value)                                             \
    a = ok; a.field = value; CHECK(in(a) == SPK_EINVAL);                  \
    a = ok; a.field = value; CHECK(paste(a) == SPK_EINVAL);               \
    a = ok; a.field = value; CHECK(match(a) == SPK_EINVAL); refusals += 3
    REFUSED(y, nullptr);
    CHECK(std::strstr(spk_last_error(), "plane pointer"));
    REFUSED(uv, nullptr);
    REFUSED(sim, nullptr);
    CHECK(std::strstr(spk_last_error(), "transform"));
    REFUSED(N, 0);
    REFUSED(N, -3);
    REFUSED(Hs, 0);
    REFUSED(Ws, -1);
    REFUSED(H, 0);
    REFUSED(W, 0);
    REFUSED(H, 7);
    CHECK(std::strstr(spk_last_error(), "even"));
    REFUSED(W, 9);
    REFUSED(uv, u8 + 9);
    CHECK(std::strstr(spk_last_error(), "aligned"));
    REFUSED(uv_row, 9);
    CHECK(std::strstr(spk_last_error(), "even"));
    REFUSED(y_row, 7);
    CHECK(std::strstr(spk_last_error(), "row stride"));
    REFUSED(uv_row, 6);
    REFUSED(W, 0x7ffffffe);                                  // an even W beyond the rows
    REFUSED(standard, 2020);
    CHECK(std::strstr(spk_last_error(), "standard"));
    REFUSED(standard, 0);
    REFUSED(full_range, 2);
    CHECK(std::strstr(spk_last_error(), "full_range"));
    REFUSED(full_range, -1);
#undef REFUSED
    // two frames: an odd UV image stride for all three; a negative stride for the two that read; overlap for the one that writes
#define REFUSED2(call, stmt) a = ok; a.N = 2; stmt; CHECK(call(a) == SPK_EINVAL); ++refusals
    REFUSED2(in, a.uv_img = 33);
    REFUSED2(paste, a.uv_img = 33);
    REFUSED2(match, a.uv_img = 33);
    REFUSED2(in, a.y_img = -64);
    CHECK(std::strstr(spk_last_error(), "negative"));
    REFUSED2(match, a.uv_img = -32);
    REFUSED2(paste, a.y_img = 63);                           // two Y planes of 8 rows of 8 bytes overlap below 64
    CHECK(std::strstr(spk_last_error(), "overlap"));
    REFUSED2(paste, a.uv_img = 30);                          // two UV planes of 4 rows of 8 bytes overlap below 32
    REFUSED2(paste, a.y_img = 0);
    REFUSED2(paste, a.uv_img = -32);
    REFUSED2(paste, (a.H = 0x7ffffffe, a.y_img = 64));       // (H - 1) * row stride does not wrap
#undef REFUSED2
    a = ok; a.dst = nullptr; CHECK(in(a) == SPK_EINVAL); ++refusals;
    a = ok; a.src = nullptr; CHECK(paste(a) == SPK_EINVAL); ++refusals;
    a = ok; a.src = nullptr; CHECK(match(a) == SPK_EINVAL); ++refusals;

    // the way out and its statistics: feather, value range, matte
#define REFUSED(field, value)                                             \
    a = ok; a.field = value; CHECK(paste(a) == SPK_EINVAL);               \
    a = ok; a.field = value; CHECK(match(a) == SPK_EINVAL); refusals += 2
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
#define REFUSED2(stmt)                                                    \
    a = ok; a.N = 2; stmt; CHECK(paste(a) == SPK_EINVAL);                 \
    a = ok; a.N = 2; stmt; CHECK(match(a) == SPK_EINVAL); refusals += 2
    REFUSED2((a.matte = f, a.matte_frames = 0));
    REFUSED2((a.matte = f, a.matte_frames = 3));
    REFUSED2((a.N = 3, a.matte = f, a.matte_frames = 2));
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
    a = ok; a.N = 2; a.ws_bytes = need1;                     // two frames need twice the bytes
    CHECK(match(a) == SPK_EINVAL && std::strstr(spk_last_error(), "workspace"));
    ++refusals;
#undef REFUSED
    std::printf("sim nv12 host check: %d argument refusals of the three entry points passed\n", refusals);
    return 0;
}
