// Host-side check of the entry points a surface table adds (csrc/frame_table_nv12.hip), under AddressSanitizer / UBSan: every
// refusal of spk_surface_table_check -- pure host code over a host copy of a table: the half-formed entries, the plane extents that
// leave 64 bits, the overlap cases (Y of one entry against UV of another, an entry's own two planes) and the tables that must pass
// (touching ranges, every surface absent, entries out of address order, Y and UV in separate allocations) -- and every refusal of the
// four _nv12_sim_table entry points, which happens before a launch and before anything is dereferenced (the entry points never read
// a table), so no device is needed; what the entry points share goes through each of them that shares it.  The file is linked with
// nothing else: what it shares lives in headers.  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/frame_table_nv12.hip tools/surface_table_host_check.cpp -o tools/_bin/surface_table_host_check
//   tools/_bin/surface_table_host_check
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    alignas(16) static uint8_t raw[16384];
    alignas(16) static uint8_t apart[64];                                 // a second allocation
    int refusals = 0, passes = 0;

    // ---- spk_surface_table_check.  Entry 0: 4 x 6 at pitch 16, Y in [0, 54), UV (two rows at pitch 8) in [54, 68); entry 1: 2 x 2
    // packed, Y in [68, 72), UV in [72, 74); entry 2: absent; entry 3: 6 x 4, Y in [4096, 4120), UV (three rows at pitch 6) in `apart`
    const spk_surface_ref good[4] = {{raw, raw + 54, 16, 8, 4, 6}, {raw + 68, raw + 72, 2, 2, 2, 2}, {nullptr, nullptr, 0, 0, 0, 0},
                                     {raw + 4096, apart, 4, 6, 6, 4}};
    spk_surface_ref t[4];
#define PASSES(stmt, written) std::memcpy(t, good, sizeof t); stmt; CHECK(spk_surface_table_check(t, 4, written) == SPK_OK); ++passes
#define REFUSED(stmt, written, word) std::memcpy(t, good, sizeof t); stmt; \
    CHECK(spk_surface_table_check(t, 4, written) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    PASSES((void)0, 0);
    PASSES((void)0, 1);                                                   // four ranges of raw touch: apart; Y and UV of 3 live apart
    CHECK(spk_surface_table_check(nullptr, 4, 0) == SPK_EINVAL && std::strstr(spk_last_error(), "null"));
    ++refusals;
    CHECK(spk_surface_table_check(good, 0, 0) == SPK_EINVAL && std::strstr(spk_last_error(), "N must"));
    ++refusals;
    CHECK(spk_surface_table_check(good, -4, 1) == SPK_EINVAL && std::strstr(spk_last_error(), "N must"));
    ++refusals;
    // half-formed: not usable and not all zero
    REFUSED(t[0].y = nullptr, 0, "entry 0 is half-formed");
    REFUSED(t[0].uv = nullptr, 1, "entry 0 is half-formed");
    REFUSED(t[1].H = 0, 0, "entry 1 is half-formed");
    REFUSED(t[1].H = 3, 0, "entry 1 is half-formed");                     // odd
    REFUSED(t[3].H = -2, 0, "entry 3 is half-formed");
    REFUSED(t[0].W = 5, 0, "entry 0 is half-formed");
    REFUSED(t[0].W = 0, 0, "entry 0 is half-formed");
    REFUSED(t[3].W = 1, 1, "entry 3 is half-formed");
    REFUSED(t[0].y_row_stride = 5, 0, "entry 0 is half-formed");          // W = 6
    REFUSED(t[0].y_row_stride = -16, 0, "entry 0 is half-formed");
    REFUSED(t[0].uv_row_stride = 4, 0, "entry 0 is half-formed");
    REFUSED(t[0].uv_row_stride = 7, 0, "entry 0 is half-formed");         // odd
    REFUSED(t[0].uv = raw + 55, 0, "entry 0 is half-formed");             // not 2-byte aligned
    REFUSED(t[2].y = raw + 512, 0, "entry 2 is half-formed");             // an absent surface with a pointer left in it
    REFUSED(t[2].uv_row_stride = 8, 0, "entry 2 is half-formed");
    REFUSED(t[2].W = 2, 1, "entry 2 is half-formed");
    REFUSED((t[0].y_row_stride = 0, t[0].uv_row_stride = 0, t[0].H = 0, t[0].W = 0), 0, "entry 0 is half-formed");   // only the pointers are left
    PASSES((t[0].y_row_stride = 6, t[0].uv_row_stride = 6), 1);           // the smallest strides
    PASSES(std::memset(t, 0, sizeof t), 1);                               // every surface absent
    PASSES((t[0] = good[3], t[3] = good[0]), 1);                          // entries out of address order
    PASSES(t[0].uv = apart + 16, 1);                                      // Y and UV in separate allocations, behind the UV of 3
    // extents that leave 64 bits: (rows - 1) * stride, + W, and the address behind the last byte
    REFUSED(t[0].y_row_stride = INT64_MAX / 2 + 1, 0, "entry 0: the Y extent");                  // 3 * 2^62
    REFUSED((t[0].H = INT32_MAX - 1, t[0].y_row_stride = (int64_t)1 << 33), 0, "entry 0: the Y extent");
    REFUSED(t[0].uv_row_stride = INT64_MAX - 1, 0, "entry 0: the UV extent");                    // the product fits, + 6 does not
    REFUSED(t[3].uv_row_stride = (int64_t)1 << 62, 0, "entry 3: the UV extent");                 // 2 * 2^62
    REFUSED(t[1].y = (const uint8_t*)(UINTPTR_MAX - 2), 0, "entry 1: the Y extent");             // y + 4 wraps
    REFUSED(t[1].uv = (const uint8_t*)(UINTPTR_MAX - 1), 1, "entry 1: the UV extent");           // uv + 2 wraps
    PASSES((t[1].y_row_stride = (int64_t)1 << 62, t[1].uv_row_stride = INT64_MAX - 1), 0);       // one UV row: its stride does not count
    // overlap: tolerated when the surfaces are read, refused when they are written
    PASSES(t[1].y = raw + 53, 0);
    REFUSED(t[1].y = raw + 53, 1, "entries 0 (Y) and 1 (Y) overlap");     // Y of 0 ends at 54
    REFUSED(t[1].y = raw + 66, 1, "entries 0 (UV) and 1 (Y) overlap");    // Y of one entry against UV of another
    REFUSED(t[1].uv = raw + 20, 1, "entries 0 (Y) and 1 (UV) overlap");   // inside the padding columns of Y 0: its byte RANGE
    PASSES(t[0].uv = raw + 52, 0);
    REFUSED(t[0].uv = raw + 52, 1, "entries 0 (Y) and 0 (UV) overlap");   // an entry's own two planes
    REFUSED(t[0].uv = raw, 1, "entries 0 (Y) and 0 (UV) overlap");        // ... on one first byte
    REFUSED((t[3].y = raw + 72), 1, "entries 1 (UV) and 3 (Y) overlap");
    REFUSED(t[2] = good[1], 1, "entries 1 (Y) and 2 (Y) overlap");        // the same surface twice
    REFUSED(t[3].uv = raw + 4100, 1, "entries 3 (Y) and 3 (UV) overlap");
    REFUSED((t[0] = good[3], t[3] = {raw + 40, raw + 8192, 16, 8, 4, 6}), 1, "entries 1 (Y) and 3 (Y) overlap");     // 3 spans [40, 94): 1 is named first
    PASSES(t[3].uv = raw + 74, 1);                                        // right behind the UV of 1
#undef PASSES
#undef REFUSED

    // ---- the four entry points.  A table of 3 entries at [0, 120); sim rows, a matte, colour rows, sums and the workspace behind it
    const spk_surface_ref* const table = (const spk_surface_ref*)raw;
    float* const x = (float*)(raw + 1024);                                // src [3,3,4,4]: [1024, 1600)
    float* const sim = (float*)(raw + 2048);
    float* const matte = (float*)(raw + 2304);
    float* const colour = (float*)(raw + 2560);                           // [2560, 2632)
    double* const sums = (double*)(raw + 2816);                           // [2816, 3128)
    float* const dst = (float*)(raw + 4096);                              // the way in's output [3,3,8,8]: [4096, 6400)
    const size_t ws_bytes = 3 * 64 * 13 * 8;                              // three frames: 64 workgroups x 13 doubles each
    void* const ws = (void*)(uintptr_t)0x10000000;                        // never dereferenced: far from raw

    struct In { const spk_surface_ref* table; int N; const float* sim; int standard, full_range; float* dst; int Hout, Wout; };
    const In in_ok = {table, 3, sim, 601, 0, dst, 8, 8};
    In i;
    auto way_in = [&](const In& a) {
        return spk_frames_nv12_to_f32_sim_table(a.table, a.N, a.sim, 0, a.standard, a.full_range, a.dst, a.Hout, a.Wout, 1, 1, 1, 0, 0, 0, nullptr);
    };
#define REFUSED(stmt, word) i = in_ok; stmt; CHECK(way_in(i) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED(i.table = nullptr, "null surface table");
    REFUSED(i.table = (const spk_surface_ref*)(raw + 4), "aligned");
    REFUSED(i.N = 0, "N must");
    REFUSED(i.N = -3, "N must");
    REFUSED(i.sim = nullptr, "null transform");
    REFUSED(i.dst = nullptr, "null frame pointer");
    REFUSED(i.Hout = 0, "output size");
    REFUSED(i.Wout = -8, "output size");
    REFUSED(i.standard = 2020, "standard");
    REFUSED(i.standard = 0, "standard");
    REFUSED(i.full_range = 2, "full_range");
    REFUSED(i.full_range = -1, "full_range");
    REFUSED(i.dst = (float*)(raw + 116), "overlaps dst");                 // dst on the table's last bytes
    REFUSED(i.table = (const spk_surface_ref*)(raw + 6392), "overlaps dst");     // the table on dst's
    REFUSED(i.table = (const spk_surface_ref*)(raw + 4096), "overlaps dst");
    REFUSED((i.N = 0x7fffffff, i.Hout = 0x7fffffff, i.Wout = 1, i.dst = (float*)(raw + 8192)), "overlaps dst");      // 2^62 * 12 bytes and more: the sizes are 64-bit
#undef REFUSED

    struct Paste { const float* src; int N, Hs, Ws; const spk_surface_ref* table; const float* sim; int standard, full_range; double feather;
                   float lo, k; const float* matte; int matte_frames; const float* colour; };
    const Paste paste_ok = {x, 3, 4, 4, table, sim, 709, 1, 2.0, -1.f, 127.5f, matte, 3, colour};
    Paste p;
    auto paste = [&](const Paste& a) {
        return spk_frames_paste_nv12_sim_table(a.src, a.N, a.Hs, a.Ws, a.table, a.sim, a.standard, a.full_range, a.feather, a.lo, a.k, a.matte,
                                               a.matte_frames, a.colour, nullptr);
    };
    auto match = [&](const Paste& a, double max_gain, double min_sigma, double min_weight, float* out, void* w, size_t wb) {
        return spk_paste_colour_match_nv12_sim_table(a.src, a.N, a.Hs, a.Ws, a.table, a.sim, a.standard, a.full_range, a.feather, a.lo, a.k, a.matte,
                                                     a.matte_frames, max_gain, min_sigma, min_weight, out, w, wb, nullptr);
    };
    auto totals = [&](const Paste& a, double* out, void* w, size_t wb) {
        return spk_paste_colour_sums_nv12_sim_table(a.src, a.N, a.Hs, a.Ws, a.table, a.sim, a.standard, a.full_range, a.feather, a.lo, a.k, a.matte,
                                                    a.matte_frames, out, w, wb, nullptr);
    };
    // what the three share, through each of them
#define REFUSED(stmt, word)                                                                                         \
    p = paste_ok; stmt; CHECK(paste(p) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals;         \
    CHECK(match(p, 2.0, 1.0, 16.0, colour, ws, ws_bytes) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals; \
    CHECK(totals(p, sums, ws, ws_bytes) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED(p.src = nullptr, "null frame pointer");
    REFUSED(p.table = nullptr, "null surface table");
    REFUSED(p.table = (const spk_surface_ref*)(raw + 12), "aligned");
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
    REFUSED(p.standard = 2020, "standard");
    REFUSED(p.standard = 1, "standard");
    REFUSED(p.full_range = 2, "full_range");
    REFUSED(p.full_range = -1, "full_range");
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
    REFUSED(match(p, 2.0, 1.0, 16.0, (float*)(raw + 116), ws, ws_bytes), "overlaps the colour rows");    // rows on the table's last bytes
    REFUSED(match(p, 2.0, 1.0, 16.0, (float*)raw, ws, ws_bytes), "overlaps the colour rows");
    REFUSED(match(p, 2.0, 1.0, 16.0, colour, raw + 112, ws_bytes), "overlaps the workspace");
    p.table = (const spk_surface_ref*)(raw + 2624);
    REFUSED(match(p, 2.0, 1.0, 16.0, colour, ws, ws_bytes), "overlaps the colour rows");                 // the table on the rows' last bytes
    p = paste_ok;
    REFUSED(totals(p, nullptr, ws, ws_bytes), "null sums");
    REFUSED(totals(p, (double*)(raw + 2820), ws, ws_bytes), "aligned");
    REFUSED(totals(p, sums, nullptr, ws_bytes), "workspace");
    REFUSED(totals(p, sums, ws, ws_bytes - 8), "workspace");
    REFUSED(totals(p, sums, (void*)((uintptr_t)ws + 2), ws_bytes), "aligned");
    REFUSED(totals(p, (double*)(raw + 112), ws, ws_bytes), "overlaps the sums");
    REFUSED(totals(p, (double*)raw, ws, ws_bytes), "overlaps the sums");
    REFUSED(totals(p, sums, raw + 8, ws_bytes), "overlaps the workspace");
    p.table = (const spk_surface_ref*)(raw + 3120);
    REFUSED(totals(p, sums, ws, ws_bytes), "overlaps the sums");                                         // the sums end at 3128
    p = paste_ok, p.table = (const spk_surface_ref*)((uintptr_t)ws + ws_bytes - 8);
    REFUSED(totals(p, sums, ws, ws_bytes), "overlaps the workspace");                                    // the table on the workspace's last bytes
#undef REFUSED
    std::printf("surface table host check: %d refusals and %d passes of spk_surface_table_check and the four _nv12_sim_table entry points\n",
                refusals, passes);
    return 0;
}
