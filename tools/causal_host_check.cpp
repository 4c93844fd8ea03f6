// Host-side check of the causal filters under AddressSanitizer / UBSan: the argument validation of spk_causal_filter and
// spk_colour_rows_causal (csrc/causal_filter.hip) -- every refusal happens before a launch and before anything is dereferenced, so no
// device is needed -- with the sizes whose products would wrap a 32-bit int.  The file is linked with nothing else: what it shares
// lives in headers.  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/causal_filter.hip tools/causal_host_check.cpp -o tools/_bin/causal_host_check
//   tools/_bin/causal_host_check
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    alignas(8) uint8_t raw[4096];
    int refusals = 0;

    // ---- the filter: 3 frames of 5 landmarks.  x, w, y, wy and the state are ranges of one buffer that do not overlap
    struct Filter {
        const float* x; const float* w; int64_t stride; int N, D, group; double rate, min_cutoff, beta, d_cutoff; int hold;
        double* state; float* y; float* wy;
    };
    float* const x = (float*)raw;                                         // [0, 120)
    float* const w = (float*)(raw + 128);                                 // [128, 188)
    float* const y = (float*)(raw + 256);                                 // [256, 376)
    float* const wy = (float*)(raw + 384);                                // [384, 444)
    double* const state = (double*)(raw + 512);                           // [512, 752): 5 groups of 6 doubles
    const Filter ok = {x, w, 5, 3, 10, 2, 30.0, 1.0, 0.05, 1.0, 5, state, y, wy};
    auto filter = [&](const Filter& a) {
        return spk_causal_filter(a.x, a.w, a.stride, a.N, a.D, a.group, a.rate, a.min_cutoff, a.beta, a.d_cutoff, a.hold, a.state, a.y, a.wy,
                                 nullptr);
    };
    Filter a;
#define REFUSED(stmt) a = ok; stmt; CHECK(filter(a) == SPK_EINVAL); ++refusals
    REFUSED(a.x = nullptr);
    CHECK(std::strstr(spk_last_error(), "null"));
    REFUSED(a.y = nullptr);
    REFUSED(a.state = nullptr);
    CHECK(std::strstr(spk_last_error(), "state"));
    REFUSED(a.state = (double*)(raw + 516));
    CHECK(std::strstr(spk_last_error(), "aligned"));
    REFUSED(a.N = 0);
    REFUSED(a.N = -3);
    REFUSED(a.D = 0);
    REFUSED(a.D = -10);
    REFUSED(a.group = 0);
    CHECK(std::strstr(spk_last_error(), "group"));
    REFUSED(a.group = 5);
    REFUSED(a.group = -2);
    REFUSED(a.group = 3);                                    // does not divide 10
    REFUSED(a.group = 4);
    REFUSED((a.D = 0x7fffffff, a.group = 2));                // odd
    REFUSED(a.stride = -1);
    CHECK(std::strstr(spk_last_error(), "stride"));
    REFUSED(a.stride = 4);                                   // in (0, G)
    REFUSED(a.stride = 1);
    REFUSED((a.w = nullptr, a.stride = 3));                  // the rule holds with or without weights
    REFUSED(a.rate = 0.0);
    CHECK(std::strstr(spk_last_error(), "rate"));
    REFUSED(a.rate = -30.0);
    REFUSED(a.rate = NAN);
    REFUSED(a.rate = INFINITY);
    REFUSED(a.min_cutoff = 0.0);
    CHECK(std::strstr(spk_last_error(), "min_cutoff"));
    REFUSED(a.min_cutoff = -1.0);
    REFUSED(a.min_cutoff = NAN);
    REFUSED(a.min_cutoff = INFINITY);
    REFUSED(a.d_cutoff = 0.0);
    CHECK(std::strstr(spk_last_error(), "d_cutoff"));
    REFUSED(a.d_cutoff = NAN);
    REFUSED(a.d_cutoff = INFINITY);
    REFUSED(a.beta = -1e-9);
    CHECK(std::strstr(spk_last_error(), "beta"));
    REFUSED(a.beta = NAN);
    REFUSED(a.beta = INFINITY);
    REFUSED(a.hold = -1);
    CHECK(std::strstr(spk_last_error(), "hold"));
    REFUSED(a.hold = -0x7fffffff - 1);
    // a state range that overlaps x, w, y or wy: the state's first bytes, its last bytes, the other range's last bytes
    REFUSED(a.state = (double*)raw);
    CHECK(std::strstr(spk_last_error(), "overlaps"));
    REFUSED(a.state = (double*)(raw + 112));                 // x ends at 120
    REFUSED(a.x = (const float*)(raw + 748));                // the state ends at 752
    REFUSED(a.state = (double*)(raw + 184));                 // w ends at 188
    REFUSED(a.y = (float*)(raw + 512));
    REFUSED(a.y = (float*)(raw + 396));                      // ... + 120 = 516 > 512
    REFUSED(a.wy = (float*)(raw + 748));
    REFUSED(a.wy = (float*)(raw + 456));                     // ... + 60 = 516
    REFUSED((a.w = (const float*)(raw + 768), a.stride = 0, a.state = (double*)(raw + 784)));    // one set of 5 weights: [768, 788)
    REFUSED((a.N = 0x7fffffff, a.D = 0x7ffffffe, a.w = nullptr, a.stride = 0, a.wy = nullptr, a.x = (const float*)raw, a.y = (float*)raw,
             a.state = (double*)(raw + 2048)));              // N * D * 4 wraps 32 bits (and 2^62 * 4 does not wrap 64): x covers the state
    REFUSED((a.N = 0x7fffffff, a.D = 0x40000000, a.group = 1, a.w = nullptr, a.stride = 0, a.wy = nullptr, a.x = (const float*)raw,
             a.y = (float*)raw, a.state = (double*)(raw + 2048)));
#undef REFUSED
    // what is legal and reaches the launch is not run here: y == x, no weights, no wy are arguments the refusals above pass by
    // (each case changes one thing of a call that is in order)

    // ---- the colour rows: 7 frames
    struct Rows { const double* sums; int N; double decay, max_gain, min_sigma, min_weight; double* state; float* out; };
    double* const sums = (double*)(raw + 1024);                           // [1024, 1752)
    double* const P = (double*)(raw + 1792);                              // [1792, 1896)
    float* const rows = (float*)(raw + 1920);                             // [1920, 2088)
    const Rows rows_ok = {sums, 7, 0.9, 2.0, 1.0, 16.0, P, rows};
    auto causal = [&](const Rows& r) {
        return spk_colour_rows_causal(r.sums, r.N, r.decay, r.max_gain, r.min_sigma, r.min_weight, r.state, r.out, nullptr);
    };
    Rows r;
#define REFUSED(stmt) r = rows_ok; stmt; CHECK(causal(r) == SPK_EINVAL); ++refusals
    REFUSED(r.sums = nullptr);
    REFUSED(r.state = nullptr);
    REFUSED(r.out = nullptr);
    REFUSED(r.sums = (const double*)(raw + 1028));
    CHECK(std::strstr(spk_last_error(), "aligned"));
    REFUSED(r.state = (double*)(raw + 1796));
    REFUSED(r.N = 0);
    REFUSED(r.N = -7);
    REFUSED(r.decay = -1e-9);
    CHECK(std::strstr(spk_last_error(), "decay"));
    REFUSED(r.decay = 1.0000001);
    REFUSED(r.decay = NAN);
    REFUSED(r.decay = INFINITY);
    REFUSED(r.max_gain = 0.999);
    CHECK(std::strstr(spk_last_error(), "max_gain"));
    REFUSED(r.max_gain = NAN);
    REFUSED(r.max_gain = INFINITY);
    REFUSED(r.min_sigma = -1e-9);
    CHECK(std::strstr(spk_last_error(), "min_sigma"));
    REFUSED(r.min_sigma = NAN);
    REFUSED(r.min_sigma = INFINITY);
    REFUSED(r.min_weight = -1.0);
    CHECK(std::strstr(spk_last_error(), "min_weight"));
    REFUSED(r.min_weight = NAN);
    REFUSED(r.min_weight = INFINITY);
    REFUSED(r.state = (double*)(raw + 1744));                // the sums end at 1752
    CHECK(std::strstr(spk_last_error(), "overlap"));
    REFUSED(r.state = (double*)(raw + 1024));
    REFUSED(r.state = (double*)(raw + 2080));                // the rows end at 2088
    REFUSED(r.out = (float*)(raw + 1892));                   // the state ends at 1896
    REFUSED(r.out = (float*)(raw + 1748));
    REFUSED((r.N = 0x7fffffff, r.state = (double*)(raw + 3072)));         // N * 104 wraps 32 bits: the sums cover the state and the rows
#undef REFUSED
    std::printf("causal host check: %d argument refusals of the two entry points passed\n", refusals);
    return 0;
}
