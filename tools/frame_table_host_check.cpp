// Host-side check of the entry points a frame table adds (csrc/frame_table.hip), under AddressSanitizer / UBSan: every refusal of
// spk_frame_table_check -- pure host code over a host copy of a table: the half-formed entries, the extents that wrap 64 bits, the
// overlap cases, and the touching-but-disjoint ranges that must pass -- and every refusal of the five _table entry points, which
// happens before a launch and before anything is dereferenced (the entry points never read a table), so no device is needed.  The
// file is linked with nothing else: what it shares lives in headers.  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/frame_table.hip tools/frame_table_host_check.cpp -o tools/_bin/frame_table_host_check
//   tools/_bin/frame_table_host_check
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    alignas(16) static uint8_t raw[16384];
    int refusals = 0, passes = 0;

    // ---- spk_frame_table_check.  Four frames in raw: 4 x 5 at pitch 16 in [0, 63), 3 x 2 packed in [64, 82), absent, 1 x 1 at [82, 85)
    const spk_frame_ref good[4] = {{raw, 16, 4, 5}, {raw + 64, 6, 3, 2}, {nullptr, 0, 0, 0}, {raw + 82, 3, 1, 1}};
    spk_frame_ref t[4];
#define PASSES(stmt, written) std::memcpy(t, good, sizeof t); stmt; CHECK(spk_frame_table_check(t, 4, written) == SPK_OK); ++passes
#define REFUSED(stmt, written, word) std::memcpy(t, good, sizeof t); stmt; \
    CHECK(spk_frame_table_check(t, 4, written) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    PASSES((void)0, 0);
    PASSES((void)0, 1);                                                   // [64, 82) and [82, 85) touch: apart
    CHECK(spk_frame_table_check(nullptr, 4, 0) == SPK_EINVAL && std::strstr(spk_last_error(), "null"));
    ++refusals;
    CHECK(spk_frame_table_check(good, 0, 0) == SPK_EINVAL && std::strstr(spk_last_error(), "N must"));
    ++refusals;
    CHECK(spk_frame_table_check(good, -4, 1) == SPK_EINVAL && std::strstr(spk_last_error(), "N must"));
    ++refusals;
    // half-formed: not usable and not all zero
    REFUSED(t[1].data = nullptr, 0, "entry 1 is half-formed");
    REFUSED(t[0].H = 0, 0, "entry 0 is half-formed");
    REFUSED(t[3].H = -1, 0, "entry 3 is half-formed");
    REFUSED(t[1].W = 0, 0, "entry 1 is half-formed");
    REFUSED(t[1].W = -2, 0, "entry 1 is half-formed");
    REFUSED(t[0].row_stride = 14, 0, "entry 0 is half-formed");           // 3 W = 15
    REFUSED(t[0].row_stride = -16, 0, "entry 0 is half-formed");
    REFUSED(t[2].row_stride = 8, 0, "entry 2 is half-formed");            // an absent frame with a stride left in it
    REFUSED(t[2].W = 1, 1, "entry 2 is half-formed");
    REFUSED((t[0].row_stride = 0, t[0].H = 0, t[0].W = 0), 0, "entry 0 is half-formed");       // only the pointer is left
    PASSES(t[0].row_stride = 15, 1);                                      // the smallest stride
    PASSES(std::memset(t, 0, sizeof t), 1);                               // every frame absent
    // extents that leave 64 bits: (H - 1) * row_stride, + 3 W, and the address behind the last byte
    REFUSED((t[0].H = INT32_MAX, t[0].row_stride = INT64_MAX / 2), 0, "entry 0: the extent");
    REFUSED((t[1].H = 3, t[1].row_stride = INT64_MAX / 2 + 1), 0, "entry 1: the extent");     // 2 * (2^62) wraps
    REFUSED((t[1].H = 2, t[1].W = 2, t[1].row_stride = INT64_MAX - 5), 0, "entry 1: the extent");   // the product fits, + 6 does not
    REFUSED((t[3].data = (const uint8_t*)(UINTPTR_MAX - 1), t[3].H = 1, t[3].W = 1), 0, "entry 3: the extent");      // data + 3 wraps
    REFUSED((t[3].data = (const uint8_t*)(UINTPTR_MAX / 2 + 8), t[3].H = 2, t[3].row_stride = INT64_MAX - 8), 1, "entry 3: the extent");
    PASSES((t[1].H = 1, t[1].row_stride = INT64_MAX), 0);                 // one row: the stride does not count
    // overlap: tolerated when the frames are read, refused when they are written
    PASSES(t[1].data = raw + 62, 0);
    REFUSED(t[1].data = raw + 62, 1, "entries 0 and 1 overlap");          // frame 0 ends at 63
    PASSES(t[1].data = raw + 63, 1);                                      // ... and this one begins there
    REFUSED(t[3].data = raw + 81, 1, "entries 1 and 3 overlap");          // the last byte of frame 1
    REFUSED(t[3].data = raw + 64, 1, "entries 1 and 3 overlap");          // the first
    REFUSED(t[3].data = raw, 1, "entries 0 and 3 overlap");               // the same first byte as frame 0
    REFUSED(t[1] = good[0], 1, "entries 0 and 1 overlap");                // the same frame twice
    REFUSED((t[1].data = raw + 20, t[1].row_stride = 6), 1, "entries 0 and 1 overlap");       // inside frame 0's padding columns: its byte RANGE
    REFUSED((t[2] = {raw + 8, 3, 1, 1}), 1, "entries 0 and 2 overlap");   // a small frame inside a large one
    REFUSED((t[0].row_stride = 40, t[3].data = raw + 100), 1, "entries 0 and 1 overlap");     // frame 0 now spans [0, 135): 1 is named first
    PASSES((t[0].data = raw + 85, t[0].row_stride = 15), 1);              // order in memory is not the order of the entries
#undef PASSES
#undef REFUSED

    // ---- the five entry points.  A table of 3 entries at [0, 72); sim rows, a matte, colour rows, sums and the workspace behind it
    const spk_frame_ref* const table = (const spk_frame_ref*)raw;
    float* const x = (float*)(raw + 1024);                                // src [3,3,4,4]: [1024, 1600)
    float* const sim = (float*)(raw + 2048);
    float* const matte = (float*)(raw + 2304);
    float* const colour = (float*)(raw + 2560);                           // [2560, 2632)
    double* const sums = (double*)(raw + 2816);                           // [2816, 3128)
    float* const dst = (float*)(raw + 4096);                              // the way in's output [3,3,8,8]: [4096, 6400)
    const size_t ws_bytes = 3 * 64 * 13 * 8;                              // three frames: 64 workgroups x 13 doubles each
    void* const ws = (void*)(uintptr_t)0x10000000;                        // never dereferenced: far from raw

    struct In { const spk_frame_ref* table; int N; const float* sim; float* dst; int Hout, Wout; };
    const In in_ok = {table, 3, sim, dst, 8, 8};
    In i;
    auto way_in = [&](const In& a) { return spk_frames_u8_to_f32_sim_table(a.table, a.N, a.sim, 0, a.dst, a.Hout, a.Wout, 1, 1, 1, 0, 0, 0, nullptr); };
#define REFUSED(stmt, word) i = in_ok; stmt; CHECK(way_in(i) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED(i.table = nullptr, "null frame table");
    REFUSED(i.table = (const spk_frame_ref*)(raw + 4), "aligned");
    REFUSED(i.N = 0, "N must");
    REFUSED(i.N = -3, "N must");
    REFUSED(i.sim = nullptr, "null transform");
    REFUSED(i.dst = nullptr, "null frame pointer");
    REFUSED(i.Hout = 0, "output size");
    REFUSED(i.Wout = -8, "output size");
    REFUSED(i.dst = (float*)(raw + 68), "overlaps dst");                  // dst on the table's last bytes
    REFUSED(i.table = (const spk_frame_ref*)(raw + 6392), "overlaps dst");       // the table on dst's
    REFUSED(i.table = (const spk_frame_ref*)(raw + 4096), "overlaps dst");
    REFUSED((i.N = 0x7fffffff, i.Hout = 0x7fffffff, i.Wout = 1, i.dst = (float*)(raw + 8192)), "overlaps dst");      // 2^62 * 12 bytes and more: the sizes are 64-bit
#undef REFUSED

    struct Paste { const float* src; int N, Hs, Ws; const spk_frame_ref* table; const float* sim; double feather; float lo, k;
                   const float* matte; int matte_frames; const float* colour; };
    const Paste paste_ok = {x, 3, 4, 4, table, sim, 2.0, -1.f, 127.5f, matte, 3, colour};
    Paste p;
    auto paste = [&](const Paste& a) {
        return spk_frames_paste_u8_sim_table(a.src, a.N, a.Hs, a.Ws, a.table, a.sim, 0, a.feather, a.lo, a.k, a.matte, a.matte_frames, a.colour, nullptr);
    };
    auto match = [&](const Paste& a, double max_gain, double min_sigma, double min_weight, float* out, void* w, size_t wb) {
        return spk_paste_colour_match_sim_table(a.src, a.N, a.Hs, a.Ws, a.table, a.sim, 0, a.feather, a.lo, a.k, a.matte, a.matte_frames, max_gain,
                                                min_sigma, min_weight, out, w, wb, nullptr);
    };
    auto totals = [&](const Paste& a, double* out, void* w, size_t wb) {
        return spk_paste_colour_sums_sim_table(a.src, a.N, a.Hs, a.Ws, a.table, a.sim, 0, a.feather, a.lo, a.k, a.matte, a.matte_frames, out, w, wb,
                                               nullptr);
    };
    // what the three share, through each of them
#define REFUSED(stmt, word)                                                                                         \
    p = paste_ok; stmt; CHECK(paste(p) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals;         \
    CHECK(match(p, 2.0, 1.0, 16.0, colour, ws, ws_bytes) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals; \
    CHECK(totals(p, sums, ws, ws_bytes) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED(p.src = nullptr, "null frame pointer");
    REFUSED(p.table = nullptr, "null frame table");
    REFUSED(p.table = (const spk_frame_ref*)(raw + 12), "aligned");
    REFUSED(p.N = 0, "N must");
    REFUSED(p.N = -1, "N must");
    REFUSED(p.sim = nullptr, "null transform");
    REFUSED(p.Hs = 0, "source size");
    REFUSED(p.Ws = -4, "source size");
    REFUSED(p.feather = -1.0, "feather");
    REFUSED(p.feather = NAN, "feather");
    REFUSED(p.feather = INFINITY, "feather");
    REFUSED(p.k = 0.f, "value range");
    REFUSED(p.k = -1.f, "value range");
    REFUSED(p.lo = NAN, "value range");
    REFUSED(p.k = INFINITY, "value range");
    REFUSED(p.matte_frames = 2, "matte_frames");
    REFUSED(p.matte_frames = 0, "matte_frames");
    REFUSED((p.matte = nullptr, p.matte_frames = 1), "matte_frames");
#undef REFUSED
    // the statistics' own
#define REFUSED(call, word) CHECK((call) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    p = paste_ok;
    REFUSED(match(p, 2.0, 1.0, 16.0, nullptr, ws, ws_bytes), "null colour row");
    REFUSED(match(p, 0.999, 1.0, 16.0, colour, ws, ws_bytes), "max_gain");
    REFUSED(match(p, NAN, 1.0, 16.0, colour, ws, ws_bytes), "max_gain");
    REFUSED(match(p, INFINITY, 1.0, 16.0, colour, ws, ws_bytes), "max_gain");
    REFUSED(match(p, 2.0, -1e-9, 16.0, colour, ws, ws_bytes), "min_sigma");
    REFUSED(match(p, 2.0, NAN, 16.0, colour, ws, ws_bytes), "min_sigma");
    REFUSED(match(p, 2.0, 1.0, -1.0, colour, ws, ws_bytes), "min_weight");
    REFUSED(match(p, 2.0, 1.0, INFINITY, colour, ws, ws_bytes), "min_weight");
    REFUSED(match(p, 2.0, 1.0, 16.0, colour, nullptr, ws_bytes), "workspace");
    REFUSED(match(p, 2.0, 1.0, 16.0, colour, ws, ws_bytes - 1), "workspace");
    REFUSED(match(p, 2.0, 1.0, 16.0, colour, (void*)((uintptr_t)ws + 4), ws_bytes), "aligned");
    REFUSED(match(p, 2.0, 1.0, 16.0, (float*)(raw + 68), ws, ws_bytes), "overlaps the colour rows");     // rows on the table's last bytes
    REFUSED(match(p, 2.0, 1.0, 16.0, (float*)raw, ws, ws_bytes), "overlaps the colour rows");
    REFUSED(match(p, 2.0, 1.0, 16.0, colour, raw + 64, ws_bytes), "overlaps the workspace");
    p.table = (const spk_frame_ref*)(raw + 2624);
    REFUSED(match(p, 2.0, 1.0, 16.0, colour, ws, ws_bytes), "overlaps the colour rows");                 // the table on the rows' last bytes
    p = paste_ok;
    REFUSED(totals(p, nullptr, ws, ws_bytes), "null sums");
    REFUSED(totals(p, (double*)(raw + 2820), ws, ws_bytes), "aligned");
    REFUSED(totals(p, sums, nullptr, ws_bytes), "workspace");
    REFUSED(totals(p, sums, ws, ws_bytes - 8), "workspace");
    REFUSED(totals(p, sums, (void*)((uintptr_t)ws + 2), ws_bytes), "aligned");
    REFUSED(totals(p, (double*)(raw + 64), ws, ws_bytes), "overlaps the sums");
    REFUSED(totals(p, (double*)raw, ws, ws_bytes), "overlaps the sums");
    REFUSED(totals(p, sums, raw + 8, ws_bytes), "overlaps the workspace");
    p.table = (const spk_frame_ref*)(raw + 3120);
    REFUSED(totals(p, sums, ws, ws_bytes), "overlaps the sums");                                         // the sums end at 3128
    p = paste_ok, p.table = (const spk_frame_ref*)((uintptr_t)ws + ws_bytes - 8);
    REFUSED(totals(p, sums, ws, ws_bytes), "overlaps the workspace");                                    // the table on the workspace's last bytes
#undef REFUSED
    std::printf("frame table host check: %d refusals and %d passes of spk_frame_table_check and the five _table entry points\n", refusals, passes);
    return 0;
}
