// Host-side check of the aligned video edge of csrc/frame_sim.hip under AddressSanitizer / UBSan: the argument validation of
// spk_frames_u8_to_f32_sim and spk_frames_paste_u8_sim -- every refusal happens before a launch and before anything is
// dereferenced, so no device is needed -- with the sizes whose products would wrap a 32-bit int.  Build and run from the
// repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/frame_sim.hip tools/sim_host_check.cpp -o tools/_bin/sim_host_check
//   tools/_bin/sim_host_check
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    uint8_t u8[4];
    float f[4];
    int refusals = 0;

    struct InArgs {
        const uint8_t* src; float* dst; const float* sim;
        int N, H, W, Hout, Wout; int64_t img, row;
    };
    const InArgs oki = {u8, f, f, 1, 8, 8, 2, 2, 192, 24};
    auto way_in = [&](const InArgs& a) {
        return spk_frames_u8_to_f32_sim(a.src, a.img, a.row, a.N, a.H, a.W, a.sim, 0, a.dst, a.Hout, a.Wout, 1.f, 1.f, 1.f, 0.f, 0.f, 0.f, nullptr);
    };
    InArgs a;
#define REFUSED(field, value) a = oki; a.field = value; CHECK(way_in(a) == SPK_EINVAL); ++refusals
    REFUSED(src, nullptr);
    REFUSED(dst, nullptr);
    REFUSED(sim, nullptr);
    CHECK(std::strstr(spk_last_error(), "transform"));
    REFUSED(N, 0);
    REFUSED(N, -2);
    REFUSED(H, 0);
    REFUSED(W, -8);
    REFUSED(Hout, 0);
    REFUSED(Wout, -1);
    REFUSED(row, 23);
    CHECK(std::strstr(spk_last_error(), "row stride"));
    REFUSED(W, 0x7fffffff);                                  // 3 * W does not wrap
    REFUSED(img, -1);
#undef REFUSED

    struct OutArgs {
        const float* src; uint8_t* dst; const float* sim;
        int N, Hs, Ws, H, W; int64_t img, row; double feather; float lo, k;
    };
    const OutArgs oko = {f, u8, f, 1, 4, 4, 8, 8, 192, 24, 0.0, -1.f, 127.5f};
    auto way_out = [&](const OutArgs& b) {
        return spk_frames_paste_u8_sim(b.src, b.N, b.Hs, b.Ws, b.dst, b.img, b.row, b.H, b.W, b.sim, 0, b.feather, b.lo, b.k, nullptr);
    };
    OutArgs b;
#define REFUSED(field, value) b = oko; b.field = value; CHECK(way_out(b) == SPK_EINVAL); ++refusals
    REFUSED(src, nullptr);
    REFUSED(dst, nullptr);
    REFUSED(sim, nullptr);
    CHECK(std::strstr(spk_last_error(), "transform"));
    REFUSED(N, 0);
    REFUSED(Hs, 0);
    REFUSED(Ws, -1);
    REFUSED(H, 0);
    REFUSED(W, 0);
    REFUSED(row, 23);
    CHECK(std::strstr(spk_last_error(), "row stride"));
    REFUSED(W, 0x7fffffff);
    REFUSED(feather, -0.5);
    CHECK(std::strstr(spk_last_error(), "feather"));
    REFUSED(feather, NAN);
    REFUSED(feather, INFINITY);
    REFUSED(lo, NAN);
    REFUSED(k, 0.f);
    REFUSED(k, INFINITY);
    b = oko; b.N = 2; b.img = 191;                           // two frames of 8 rows of 24 bytes overlap below 192
    CHECK(way_out(b) == SPK_EINVAL && std::strstr(spk_last_error(), "overlap"));
    b = oko; b.N = 2; b.img = 0;
    CHECK(way_out(b) == SPK_EINVAL);
    b = oko; b.N = 2; b.img = -192;
    CHECK(way_out(b) == SPK_EINVAL);
    b = oko; b.N = 2; b.H = 0x7fffffff; b.img = 192;         // (H - 1) * row_stride does not wrap
    CHECK(way_out(b) == SPK_EINVAL);
    refusals += 4;
#undef REFUSED
    std::printf("sim host check: %d argument refusals of the two entry points passed\n", refusals);
    return 0;
}
