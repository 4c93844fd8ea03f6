// Host-side check of the two entry points a live room adds, under AddressSanitizer / UBSan: the argument validation of
// spk_noise_fill_rows (csrc/noise.hip) and spk_colour_rows_causal_feeds (csrc/causal_filter.hip) -- every refusal happens before a
// launch and before anything is dereferenced, so no device is needed -- with the sizes whose products would wrap a 32-bit int.  The
// two files are linked with nothing else: what they share lives in headers.  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/noise.hip speak-hack_amd/csrc/causal_filter.hip tools/live_room_host_check.cpp \
//         -o tools/_bin/live_room_host_check
//   tools/_bin/live_room_host_check
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    alignas(16) uint8_t raw[8192];
    int refusals = 0;

    // ---- the rows fill: B = 3 rows of two layers of 16 and 64 pixels = 240 floats in [0, 960); the tables behind them
    float* const dst = (float*)raw;
    uint64_t* const seeds = (uint64_t*)(raw + 1024);                      // [1024, 1048)
    int64_t* const frames = (int64_t*)(raw + 1056);                       // [1056, 1080)
    auto good = [&] {
        spk_noise_fill_rows_args a = {};
        a.dst = dst, a.seeds_dev = seeds, a.frames_dev = frames, a.B = 3, a.n_layers = 2, a.layer0 = 0;
        a.hw[0] = 16, a.hw[1] = 64;
        return a;
    };
    spk_noise_fill_rows_args a;
#define REFUSED(stmt, word) a = good(); stmt; CHECK(spk_noise_fill_rows(&a, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    CHECK(spk_noise_fill_rows(nullptr, nullptr) == SPK_EINVAL && std::strstr(spk_last_error(), "null"));
    ++refusals;
    REFUSED(a.dst = nullptr, "dst");
    REFUSED(a.B = 0, "B must");
    REFUSED(a.B = -3, "B must");
    REFUSED(a.n_layers = 0, "n_layers");
    REFUSED(a.n_layers = -1, "n_layers");
    REFUSED(a.n_layers = SPK_NOISE_MAX_LAYERS + 1, "n_layers");
    REFUSED(a.n_layers = SPK_NOISE_MAX_LAYERS, "hw[2]");                  // the layers behind the second have no pixels
    REFUSED(a.hw[1] = 0, "hw[1]");
    REFUSED(a.hw[0] = -4, "hw[0]");
    REFUSED(a.hw[0] = (1ll << 34) + 1, "2^34");
    REFUSED(a.layer0 = -1, "layer0");
    REFUSED(a.layer0 = INT32_MAX, "layer0");
    REFUSED((a.B = 0x7fffffff, a.hw[0] = 1ll << 34), "2^46");             // B * hw wraps 32 bits, and leaves the 2^46 floats
    REFUSED((a.B = 0x10000, a.hw[0] = 0x10000, a.hw[1] = 1ll << 31), "2^46");     // 2^32 floats in layer 0 pass; layer 1 does not
    REFUSED(a.seeds_dev = nullptr, "null");
    REFUSED(a.frames_dev = nullptr, "null");
    REFUSED(a.seeds_dev = (const uint64_t*)(raw + 1028), "aligned");
    REFUSED(a.frames_dev = (const int64_t*)(raw + 1060), "aligned");
    REFUSED(a.seeds_dev = (const uint64_t*)raw, "overlaps");              // a table on dst's first bytes
    REFUSED(a.frames_dev = (const int64_t*)(raw + 952), "overlaps");      // ... on its last: dst ends at 960
    REFUSED(a.dst = (float*)(raw + 1040), "overlaps");                    // dst on the seed table's last bytes
    REFUSED(a.dst = (float*)(raw + 1076), "overlaps");                    // ... on the frame table's (an unaligned dst: the scalar form)
    REFUSED((a.B = 0x8000, a.hw[0] = 0x10000, a.hw[1] = 0x10000, a.seeds_dev = (const uint64_t*)(raw + 4096)), "overlaps");
    //        2^32 floats: their byte count wraps 32 bits (16 GiB), and dst covers the table
#undef REFUSED

    // ---- the feeds' colour rows: 7 frames of 4 feeds.  sums [2048, 4960), states [5120, 5536), rows [5632, 6304)
    struct Rows { const double* sums; int N, S; double decay, max_gain, min_sigma, min_weight; double* state; float* out; };
    double* const sums = (double*)(raw + 2048);
    double* const P = (double*)(raw + 5120);
    float* const rows = (float*)(raw + 5632);
    const Rows rows_ok = {sums, 7, 4, 0.9, 2.0, 1.0, 16.0, P, rows};
    auto feeds = [&](const Rows& r) {
        return spk_colour_rows_causal_feeds(r.sums, r.N, r.S, r.decay, r.max_gain, r.min_sigma, r.min_weight, r.state, r.out, nullptr);
    };
    Rows r;
#define REFUSED(stmt, word) r = rows_ok; stmt; CHECK(feeds(r) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED(r.sums = nullptr, "null");
    REFUSED(r.state = nullptr, "null");
    REFUSED(r.out = nullptr, "null");
    REFUSED(r.sums = (const double*)(raw + 2052), "aligned");
    REFUSED(r.state = (double*)(raw + 5124), "aligned");
    REFUSED(r.N = 0, "N must");
    REFUSED(r.N = -7, "N must");
    REFUSED(r.S = 0, "S must");
    REFUSED(r.S = -4, "S must");
    REFUSED(r.decay = -1e-9, "decay");
    REFUSED(r.decay = 1.0000001, "decay");
    REFUSED(r.decay = NAN, "decay");
    REFUSED(r.decay = INFINITY, "decay");
    REFUSED(r.max_gain = 0.999, "max_gain");
    REFUSED(r.max_gain = NAN, "max_gain");
    REFUSED(r.max_gain = INFINITY, "max_gain");
    REFUSED(r.min_sigma = -1e-9, "min_sigma");
    REFUSED(r.min_sigma = NAN, "min_sigma");
    REFUSED(r.min_sigma = INFINITY, "min_sigma");
    REFUSED(r.min_weight = -1.0, "min_weight");
    REFUSED(r.min_weight = NAN, "min_weight");
    REFUSED(r.min_weight = INFINITY, "min_weight");
    REFUSED(r.state = (double*)(raw + 4952), "overlap");                  // the sums end at 4960
    REFUSED(r.state = (double*)(raw + 2048), "overlap");
    REFUSED(r.state = (double*)(raw + 6296), "overlap");                  // the rows end at 6304
    REFUSED(r.out = (float*)(raw + 5532), "overlap");                     // the states end at 5536
    REFUSED(r.out = (float*)(raw + 4956), "overlap");
    REFUSED((r.S = 5, r.state = (double*)(raw + 5216)), "overlap");       // five states end at 5736, behind the rows' start
    // sizes whose products wrap 32 bits: refused by their size, whatever the pointers
    REFUSED((r.N = 0x7fffffff, r.S = 1), "2^31");                         // N * 13
    REFUSED((r.N = 1, r.S = 0x7fffffff), "2^31");                         // S * 13
    REFUSED((r.N = 0x10000, r.S = 0x10000), "2^31");                      // N * S = 2^32
    REFUSED((r.N = 0x7fffffff, r.S = 0x7fffffff), "2^31");                // N * S * 104 would wrap 64 bits
    REFUSED((r.N = 50, r.S = 3303821), "2^31");                           // N * S * 13 = 2^31 + 2: the first size over the line
#undef REFUSED
    std::printf("live room host check: %d argument refusals of the two entry points passed\n", refusals);
    return 0;
}
