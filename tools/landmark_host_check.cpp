// Host-side check of landmarks -> rows (csrc/landmark_sim.hip) under AddressSanitizer / UBSan: the argument validation of
// spk_sim_fit_landmarks and spk_sim_smooth -- every refusal happens before a launch and before anything is dereferenced, so no
// device is needed -- with K and N at 0x7fffffff, whose index products would wrap a 32-bit int, and the overlap rule at both ends
// of the two ranges.  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/landmark_sim.hip tools/landmark_host_check.cpp -o tools/_bin/landmark_host_check
//   tools/_bin/landmark_host_check
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    float f[64];
    int refusals = 0;

    struct FitArgs {
        const float* pts; const float* weights; int64_t stride; const float* tmpl;
        int N, K; double offset; float* sim;
    };
    const FitArgs okf = {f, nullptr, 0, f, 1, 5, 0.0, f};
    auto fit = [&](const FitArgs& a) { return spk_sim_fit_landmarks(a.pts, a.weights, a.stride, a.tmpl, a.N, a.K, a.offset, a.sim, nullptr); };
    FitArgs a;
#define REFUSED(field, value) a = okf; a.field = value; CHECK(fit(a) == SPK_EINVAL); ++refusals
    REFUSED(pts, nullptr);
    REFUSED(tmpl, nullptr);
    REFUSED(sim, nullptr);
    CHECK(std::strstr(spk_last_error(), "transform"));
    REFUSED(N, 0);
    REFUSED(N, -2);
    REFUSED(K, 1);
    REFUSED(K, 0);
    REFUSED(K, -5);
    REFUSED(K, 4097);
    CHECK(std::strstr(spk_last_error(), "K must be"));
    REFUSED(K, 0x7fffffff);                                  // 2 * K does not wrap
    REFUSED(stride, -1);
    REFUSED(stride, 1);
    REFUSED(stride, 4);                                      // in (0, K)
    CHECK(std::strstr(spk_last_error(), "weight stride"));
    REFUSED(stride, INT64_MIN);
    REFUSED(offset, NAN);
    CHECK(std::strstr(spk_last_error(), "offset"));
    REFUSED(offset, INFINITY);
    REFUSED(offset, -INFINITY);
#undef REFUSED
    a = okf; a.weights = f; a.stride = 4;                    // the stride rule holds with weights as without
    CHECK(fit(a) == SPK_EINVAL);
    a = okf; a.N = 0x7fffffff; a.K = 4096; a.stride = 4095;  // the largest batch: refused for its stride, no product wrapped on the way
    CHECK(fit(a) == SPK_EINVAL && std::strstr(spk_last_error(), "weight stride"));
    a = okf; a.N = 0x7fffffff; a.K = 4096; a.stride = INT64_MAX; a.offset = NAN;
    CHECK(fit(a) == SPK_EINVAL && std::strstr(spk_last_error(), "offset"));
    refusals += 3;

    struct SmoothArgs { const float* in; int N, radius; double sigma; float* out; };
    const SmoothArgs oks = {f, 4, 2, 1.0, f + 16};           // 4 rows of 4 floats each, end to end
    auto smooth = [&](const SmoothArgs& b) { return spk_sim_smooth(b.in, b.N, b.radius, b.sigma, b.out, nullptr); };
    SmoothArgs b;
#define REFUSED(field, value) b = oks; b.field = value; CHECK(smooth(b) == SPK_EINVAL); ++refusals
    REFUSED(in, nullptr);
    REFUSED(out, nullptr);
    REFUSED(N, 0);
    REFUSED(N, -4);
    REFUSED(radius, -1);
    REFUSED(radius, 65);
    CHECK(std::strstr(spk_last_error(), "radius"));
    REFUSED(radius, 0x7fffffff);
    REFUSED(sigma, 0.0);
    CHECK(std::strstr(spk_last_error(), "sigma"));
    REFUSED(sigma, -1.0);
    REFUSED(sigma, NAN);
    REFUSED(sigma, INFINITY);
    REFUSED(out, f);                                         // the same range
    CHECK(std::strstr(spk_last_error(), "overlap"));
    REFUSED(out, f + 15);                                    // the last float of `in` is the first of `out`
    REFUSED(out, f + 1);
    REFUSED(N, 5);                                           // one row more: the end of `in` runs into `out`
    REFUSED(N, 0x7fffffff);                                  // 16 * N does not wrap
    CHECK(std::strstr(spk_last_error(), "overlap"));
#undef REFUSED
    b = {f + 16, 4, 2, 1.0, f + 1};                          // and from the other end: the last float of `out` is the first of `in`
    CHECK(smooth(b) == SPK_EINVAL && std::strstr(spk_last_error(), "overlap"));
    b = {f + 16, 0x7fffffff, 2, 1.0, f};
    CHECK(smooth(b) == SPK_EINVAL && std::strstr(spk_last_error(), "overlap"));
    refusals += 2;
    std::printf("landmark host check: %d argument refusals of the two entry points passed\n", refusals);
    return 0;
}
