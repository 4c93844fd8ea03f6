// Host-side check of the landmark matte (csrc/landmark_matte.hip) under AddressSanitizer / UBSan: the argument validation of
// spk_matte_from_landmarks -- every refusal happens before a launch and before a device pointer is dereferenced, so no device is
// needed -- with N, K, Hs and Ws at 0x7fffffff, whose index products would wrap a 32-bit int, and the contour, the one array the
// entry point READS on the host: Kc beyond the array's end must be refused before an index past it is looked at.  Build and run from
// the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/landmark_matte.hip tools/matte_host_check.cpp -o tools/_bin/matte_host_check
//   tools/_bin/matte_host_check
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_check.hpp"

int main() {
    float f[64];
    int refusals = 0;
    const std::vector<int32_t> four = {0, 3, 6, 9};          // heap arrays of exactly Kc indices: a read past the end is ASan's to find
    const std::vector<int32_t> most(128, 11);

    struct Args {
        const float* pts; int N, K; double offset; const float* sim; const int32_t* contour; int Kc; const float* fallback;
        int radius; double sigma, softness, grow; float* matte; int Hs, Ws;
    };
    const Args ok = {f, 2, 12, 0.0, f, four.data(), 4, nullptr, 2, 1.0, 4.0, 0.0, f, 16, 16};
    auto call = [&](const Args& a) {
        return spk_matte_from_landmarks(a.pts, a.N, a.K, a.offset, a.sim, a.contour, a.Kc, a.fallback, a.radius, a.sigma, a.softness, a.grow,
                                        a.matte, a.Hs, a.Ws, nullptr);
    };
    Args a;
#define REFUSED(field, value) a = ok; a.field = value; CHECK(call(a) == SPK_EINVAL); ++refusals
    REFUSED(pts, nullptr);
    REFUSED(sim, nullptr);
    REFUSED(contour, nullptr);
    CHECK(std::strstr(spk_last_error(), "contour"));
    REFUSED(matte, nullptr);
    CHECK(std::strstr(spk_last_error(), "matte"));
    REFUSED(N, 0);
    REFUSED(N, -3);
    REFUSED(K, 0);
    REFUSED(K, -1);
    REFUSED(K, 4097);
    CHECK(std::strstr(spk_last_error(), "K must be"));
    REFUSED(K, 0x7fffffff);                                  // 2 * K does not wrap
    REFUSED(K, 9);                                           // the contour's last index is K itself
    CHECK(std::strstr(spk_last_error(), "contour[3] = 9"));
    REFUSED(K, 4);
    REFUSED(Kc, 2);
    CHECK(std::strstr(spk_last_error(), "Kc must be"));
    REFUSED(Kc, 0);
    REFUSED(Kc, -4);
    REFUSED(Kc, 129);                                        // refused for its size: index 4 of a 4-element array is never read
    REFUSED(Kc, 0x7fffffff);
    REFUSED(Hs, 0);
    REFUSED(Hs, -16);
    REFUSED(Hs, 4097);
    CHECK(std::strstr(spk_last_error(), "Hs and Ws"));
    REFUSED(Hs, 0x7fffffff);
    REFUSED(Ws, 0);
    REFUSED(Ws, 4097);
    REFUSED(Ws, 0x7fffffff);                                 // BAND_PIXELS + Ws - 1 does not wrap
    REFUSED(radius, -1);
    REFUSED(radius, 65);
    CHECK(std::strstr(spk_last_error(), "radius"));
    REFUSED(radius, 0x7fffffff);
    REFUSED(sigma, 0.0);
    CHECK(std::strstr(spk_last_error(), "sigma"));
    REFUSED(sigma, -1.0);
    REFUSED(sigma, NAN);
    REFUSED(sigma, INFINITY);
    REFUSED(softness, 0.0);
    CHECK(std::strstr(spk_last_error(), "softness"));
    REFUSED(softness, -2.0);
    REFUSED(softness, NAN);
    REFUSED(softness, INFINITY);
    REFUSED(grow, NAN);
    CHECK(std::strstr(spk_last_error(), "grow"));
    REFUSED(grow, INFINITY);
    REFUSED(grow, -INFINITY);
    REFUSED(offset, NAN);
    CHECK(std::strstr(spk_last_error(), "offset"));
    REFUSED(offset, INFINITY);
    REFUSED(offset, -INFINITY);
#undef REFUSED
    const std::vector<int32_t> low = {0, -1, 6}, high = {0, 3, 0x7fffffff}, lowest = {INT32_MIN, 0, 1};
    for (const auto* bad : {&low, &high, &lowest}) {
        a = ok, a.contour = bad->data(), a.Kc = 3;
        CHECK(call(a) == SPK_EINVAL && std::strstr(spk_last_error(), "not a landmark index"));
        ++refusals;
    }
    a = ok, a.contour = most.data(), a.Kc = 128;             // the largest contour is read to its end and no further: index 11 of K = 11
    a.K = 11;
    CHECK(call(a) == SPK_EINVAL && std::strstr(spk_last_error(), "contour[0] = 11"));
    // all four sizes at their largest at once: refused for K, nothing multiplied on the way
    a = ok, a.N = 0x7fffffff, a.K = 0x7fffffff, a.Hs = 0x7fffffff, a.Ws = 0x7fffffff;
    CHECK(call(a) == SPK_EINVAL && std::strstr(spk_last_error(), "K must be"));
    // the largest batch the rules allow, refused only for its last argument: N Hs Ws and N K are formed in 64 bits in front of the launch
    a = ok, a.N = 0x7fffffff, a.K = 4096, a.Hs = 4096, a.Ws = 4096, a.offset = NAN;
    CHECK(call(a) == SPK_EINVAL && std::strstr(spk_last_error(), "offset"));
    refusals += 3;
    std::printf("matte host check: %d argument refusals of the entry point passed\n", refusals);
    return 0;
}
