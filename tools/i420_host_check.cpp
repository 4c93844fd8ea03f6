// Host-side check of the aligned I420 edge (csrc/frame_sim_i420.hip, csrc/frame_table_i420.hip) under AddressSanitizer / UBSan:
// every refusal of the nine entry points -- the four strided ones, spk_planar_table_check (pure host code over a host copy of a
// table: the half-formed entries, the plane extents that leave 64 bits, the overlap cases among three planes per entry) and the
// four _i420_sim_table ones -- and the surfaces and tables that must pass the checks: ranges that touch, every surface absent, V
// before U in memory, planes in separate allocations, an odd chroma pitch and an odd chroma base.  Every refusal happens before a
// launch and before anything is dereferenced (the entry points never read a table), so no device is needed.  The two files are
// linked with nothing else: what they share lives in headers.  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/frame_sim_i420.hip speak-hack_amd/csrc/frame_table_i420.hip tools/i420_host_check.cpp \
//         -o tools/_bin/i420_host_check
//   tools/_bin/i420_host_check
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    alignas(16) static uint8_t raw[16384];
    alignas(16) static uint8_t apart[64];                                 // a second allocation
    int refusals = 0, passes = 0;

    // ---- the four strided entry points.  One 8 x 8 surface: Y 8 rows of 8 bytes (64 per frame), U and V 4 rows of 4 bytes (16 each)
    struct Args {
        const float* src; uint8_t* y; uint8_t* u; uint8_t* v; const float* sim; float* dst;
        int N, Hs, Ws, H, W; int64_t y_img, y_row, u_img, u_row, v_img, v_row; int standard, full_range; double feather; float lo, k;
        const float* matte; int matte_frames;
        double max_gain, min_sigma, min_weight; float* out; double* sums; void* ws; size_t ws_bytes;       // the statistics only
    };
    float* const f = (float*)(raw + 8192);
    const size_t need1 = 64 * 13 * sizeof(double);                        // spk_paste_colour_match_workspace_bytes(1)
    const Args ok = {f, raw, raw + 128, raw + 192, f, f, 1, 4, 4, 8, 8, 64, 8, 16, 4, 16, 4, 601, 0, 0.0, -1.f, 127.5f, nullptr, 0,
                     2.0, 1.0, 16.0, f, (double*)f, raw + 1024, 2 * need1};
    auto in = [&](const Args& a) {
        return spk_frames_i420_to_f32_sim(a.y, a.y_img, a.y_row, a.u, a.u_img, a.u_row, a.v, a.v_img, a.v_row, a.N, a.H, a.W, a.sim, 0, a.standard,
                                          a.full_range, a.dst, a.Hs, a.Ws, 1.f, 1.f, 1.f, 0.f, 0.f, 0.f, nullptr);
    };
    auto paste = [&](const Args& a) {
        return spk_frames_paste_i420_sim(a.src, a.N, a.Hs, a.Ws, a.y, a.y_img, a.y_row, a.u, a.u_img, a.u_row, a.v, a.v_img, a.v_row, a.H, a.W, a.sim,
                                         a.standard, a.full_range, a.feather, a.lo, a.k, a.matte, a.matte_frames, nullptr, nullptr);
    };
    auto match = [&](const Args& a) {
        return spk_paste_colour_match_i420_sim(a.src, a.N, a.Hs, a.Ws, a.y, a.y_img, a.y_row, a.u, a.u_img, a.u_row, a.v, a.v_img, a.v_row, a.H, a.W,
                                               a.sim, a.standard, a.full_range, a.feather, a.lo, a.k, a.matte, a.matte_frames, a.max_gain,
                                               a.min_sigma, a.min_weight, a.out, a.ws, a.ws_bytes, nullptr);
    };
    auto totals = [&](const Args& a) {
        return spk_paste_colour_sums_i420_sim(a.src, a.N, a.Hs, a.Ws, a.y, a.y_img, a.y_row, a.u, a.u_img, a.u_row, a.v, a.v_img, a.v_row, a.H, a.W,
                                              a.sim, a.standard, a.full_range, a.feather, a.lo, a.k, a.matte, a.matte_frames, a.sums, a.ws,
                                              a.ws_bytes, nullptr);
    };
    Args a;
    // what all four refuse alike: the surface, the rows, the sizes, the standard
#define REFUSED(stmt, word)                                                                        \
    a = ok; stmt; CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));               \
    CHECK(paste(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));                          \
    CHECK(match(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));                          \
    CHECK(totals(a) == SPK_EINVAL && std::strstr(spk_last_error(), word)); refusals += 4
    REFUSED(a.y = nullptr, "plane pointer");
    REFUSED(a.u = nullptr, "plane pointer");
    REFUSED(a.v = nullptr, "plane pointer");
    REFUSED(a.sim = nullptr, "transform");
    REFUSED(a.N = 0, "N must");
    REFUSED(a.N = -3, "N must");
    REFUSED(a.H = 0, "N must");
    REFUSED(a.W = 0, "N must");
    REFUSED(a.H = 7, "even");
    REFUSED(a.W = 9, "even");
    REFUSED(a.y_row = 7, "Y row stride");
    REFUSED(a.u_row = 3, "U row stride");
    REFUSED(a.v_row = 3, "V row stride");
    REFUSED(a.v_row = -4, "V row stride");
    REFUSED(a.W = 0x7ffffffe, "Y row stride");                            // an even W beyond the rows
    REFUSED(a.standard = 2020, "standard");
    REFUSED(a.standard = 0, "standard");
    REFUSED(a.full_range = 2, "full_range");
    REFUSED(a.full_range = -1, "full_range");
#undef REFUSED
    a = ok; a.Hs = 0; CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), "output size")); ++refusals;
    a = ok; a.dst = nullptr; CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), "null frame pointer")); ++refusals;
    // two frames: a negative stride for the three that read; overlap for the one that writes
#define REFUSED2(call, stmt, word) a = ok; a.N = 2; stmt; CHECK(call(a) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED2(in, a.y_img = -64, "negative");
    REFUSED2(match, a.u_img = -16, "negative");
    REFUSED2(totals, a.v_img = -1, "negative");
    REFUSED2(paste, a.y_img = 63, "overlap");                             // two Y planes of 8 rows of 8 bytes overlap below 64
    REFUSED2(paste, a.u_img = 15, "overlap");                             // two U planes of 4 rows of 4 bytes overlap below 16
    REFUSED2(paste, a.v_img = 15, "overlap");
    REFUSED2(paste, a.v_img = 0, "overlap");
    REFUSED2(paste, a.u_img = -16, "overlap");
    REFUSED2(paste, (a.H = 0x7ffffffe, a.y_img = 64), "overlap");         // (H - 1) * row stride does not wrap
#undef REFUSED2
    // the way out and its statistics
#define REFUSED(stmt, word)                                                                        \
    a = ok; stmt; CHECK(paste(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));            \
    CHECK(match(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));                          \
    CHECK(totals(a) == SPK_EINVAL && std::strstr(spk_last_error(), word)); refusals += 3
    REFUSED(a.src = nullptr, "null frame pointer");
    REFUSED(a.Hs = 0, "source size");
    REFUSED(a.Ws = -1, "source size");
    REFUSED(a.feather = -0.5, "feather");
    REFUSED(a.feather = NAN, "feather");
    REFUSED(a.feather = INFINITY, "feather");
    REFUSED(a.lo = NAN, "value range");
    REFUSED(a.k = 0.f, "value range");
    REFUSED(a.k = INFINITY, "value range");
    REFUSED(a.matte_frames = 1, "matte_frames");                          // frames of a matte that is not there
    REFUSED(a.matte_frames = -1, "matte_frames");
    REFUSED((a.N = 2, a.matte = f, a.matte_frames = 0), "matte_frames");
    REFUSED((a.N = 2, a.matte = f, a.matte_frames = 3), "matte_frames");
#undef REFUSED
    // the statistics' own arguments
#define REFUSED(call, stmt, word) a = ok; stmt; CHECK(call(a) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED(match, a.max_gain = 0.999, "max_gain");
    REFUSED(match, a.max_gain = NAN, "max_gain");
    REFUSED(match, a.max_gain = INFINITY, "max_gain");
    REFUSED(match, a.min_sigma = -1e-9, "min_sigma");
    REFUSED(match, a.min_sigma = NAN, "min_sigma");
    REFUSED(match, a.min_weight = -1.0, "min_weight");
    REFUSED(match, a.min_weight = INFINITY, "min_weight");
    REFUSED(match, a.out = nullptr, "null colour row");
    REFUSED(match, a.ws = nullptr, "workspace");
    REFUSED(match, a.ws_bytes = need1 - 1, "workspace");
    REFUSED(match, a.ws = raw + 1028, "aligned");
    REFUSED(match, (a.N = 2, a.ws_bytes = need1), "workspace");           // two frames need twice the bytes
    REFUSED(totals, a.sums = nullptr, "null sums");
    REFUSED(totals, a.sums = (double*)(raw + 8196), "aligned");
    REFUSED(totals, a.ws = nullptr, "workspace");
    REFUSED(totals, a.ws_bytes = need1 - 8, "workspace");
    REFUSED(totals, a.ws = raw + 1026, "aligned");
#undef REFUSED
    // (a surface the strided checks let through is launched, so the surfaces that must pass are asked of the table check below)

    // ---- spk_planar_table_check.  Entry 0: 4 x 6 at pitch 16, Y in [0, 54); U, two rows of 3 bytes at the ODD pitch 3, in
    // [54, 60); V at pitch 5 from the ODD address 61, in [61, 69).  Entry 1: 2 x 2 packed, V FIRST: V at 69, U at 70, Y in [71, 75).
    // Entry 2: absent.  Entry 3: 6 x 4, Y in [4096, 4120), U (three rows of 2 bytes at pitch 2) and V in `apart`.
    const spk_planar_ref good[4] = {{raw, raw + 54, raw + 61, 16, 3, 5, 4, 6}, {raw + 71, raw + 70, raw + 69, 2, 1, 1, 2, 2},
                                    {nullptr, nullptr, nullptr, 0, 0, 0, 0, 0}, {raw + 4096, apart, apart + 6, 4, 2, 2, 6, 4}};
    spk_planar_ref t[4];
#define PASSES(stmt, written) std::memcpy(t, good, sizeof t); stmt; CHECK(spk_planar_table_check(t, 4, written) == SPK_OK); ++passes
#define REFUSED(stmt, written, word) std::memcpy(t, good, sizeof t); stmt; \
    CHECK(spk_planar_table_check(t, 4, written) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    PASSES((void)0, 0);
    PASSES((void)0, 1);                      // odd chroma pitch and base, V before U, ranges that touch (V 1 | U 1 | Y 1), planes in `apart`
    CHECK(spk_planar_table_check(nullptr, 4, 0) == SPK_EINVAL && std::strstr(spk_last_error(), "null"));
    ++refusals;
    CHECK(spk_planar_table_check(good, 0, 0) == SPK_EINVAL && std::strstr(spk_last_error(), "N must"));
    ++refusals;
    CHECK(spk_planar_table_check(good, -4, 1) == SPK_EINVAL && std::strstr(spk_last_error(), "N must"));
    ++refusals;
    // half-formed: not usable and not all zero
    REFUSED(t[0].y = nullptr, 0, "entry 0 is half-formed");
    REFUSED(t[0].u = nullptr, 1, "entry 0 is half-formed");
    REFUSED(t[0].v = nullptr, 0, "entry 0 is half-formed");
    REFUSED(t[1].H = 0, 0, "entry 1 is half-formed");
    REFUSED(t[1].H = 3, 0, "entry 1 is half-formed");                     // odd
    REFUSED(t[3].H = -2, 0, "entry 3 is half-formed");
    REFUSED(t[0].W = 5, 0, "entry 0 is half-formed");
    REFUSED(t[0].W = 0, 0, "entry 0 is half-formed");
    REFUSED(t[3].W = 1, 1, "entry 3 is half-formed");
    REFUSED(t[0].y_row_stride = 5, 0, "entry 0 is half-formed");          // W = 6
    REFUSED(t[0].y_row_stride = -16, 0, "entry 0 is half-formed");
    REFUSED(t[0].u_row_stride = 2, 0, "entry 0 is half-formed");          // W / 2 = 3
    REFUSED(t[0].v_row_stride = 2, 0, "entry 0 is half-formed");
    REFUSED(t[0].v_row_stride = -5, 1, "entry 0 is half-formed");
    REFUSED(t[2].y = raw + 512, 0, "entry 2 is half-formed");             // an absent surface with a pointer left in it
    REFUSED(t[2].v = raw + 512, 0, "entry 2 is half-formed");
    REFUSED(t[2].u_row_stride = 8, 0, "entry 2 is half-formed");
    REFUSED(t[2].W = 2, 1, "entry 2 is half-formed");
    REFUSED((t[0].y_row_stride = 0, t[0].u_row_stride = 0, t[0].v_row_stride = 0, t[0].H = 0, t[0].W = 0), 0, "entry 0 is half-formed");
    PASSES((t[0].y_row_stride = 6, t[0].u_row_stride = 3, t[0].v_row_stride = 3), 1);            // the smallest strides
    PASSES(std::memset(t, 0, sizeof t), 1);                               // every surface absent
    PASSES((t[0] = good[3], t[3] = good[0]), 1);                          // entries out of address order
    PASSES((t[0].u = apart + 12, t[0].v = apart + 32), 1);                // chroma in a separate allocation, behind the planes of 3
    PASSES((t[0].u = raw + 63, t[0].u_row_stride = 3, t[0].v = raw + 54, t[0].v_row_stride = 6), 1);     // V before U: V [54, 63), U [63, 69)
    // extents that leave 64 bits: (rows - 1) * stride, + width, and the address behind the last byte
    REFUSED(t[0].y_row_stride = INT64_MAX / 2 + 1, 0, "entry 0: the Y extent");                  // 3 * 2^62
    REFUSED((t[0].H = INT32_MAX - 1, t[0].y_row_stride = (int64_t)1 << 33), 0, "entry 0: the Y extent");
    REFUSED(t[0].u_row_stride = INT64_MAX - 1, 0, "entry 0: the U extent");                      // the product fits, + 3 does not
    REFUSED(t[3].v_row_stride = (int64_t)1 << 62, 0, "entry 3: the V extent");                   // 2 * 2^62
    REFUSED(t[1].y = (const uint8_t*)(UINTPTR_MAX - 2), 0, "entry 1: the Y extent");             // y + 4 wraps
    REFUSED(t[1].u = (const uint8_t*)UINTPTR_MAX, 1, "entry 1: the U extent");                   // u + 1 wraps
    REFUSED(t[1].v = (const uint8_t*)UINTPTR_MAX, 1, "entry 1: the V extent");
    PASSES((t[1].y_row_stride = (int64_t)1 << 62, t[1].u_row_stride = INT64_MAX - 1, t[1].v_row_stride = INT64_MAX), 0);   // one chroma row: its stride does not count
    // overlap: tolerated when the surfaces are read, refused when they are written
    PASSES(t[1].y = raw + 53, 0);
    REFUSED(t[1].y = raw + 53, 1, "entries 0 (Y) and 1 (Y) overlap");     // Y of 0 ends at 54
    REFUSED(t[1].y = raw + 66, 1, "entries 0 (V) and 1 (Y) overlap");     // Y of one entry against V of another
    REFUSED(t[1].u = raw + 20, 1, "entries 0 (Y) and 1 (U) overlap");     // inside the padding columns of Y 0: its byte RANGE
    REFUSED(t[1].v = raw + 59, 1, "entries 0 (U) and 1 (V) overlap");
    PASSES(t[0].u = raw + 52, 0);
    REFUSED(t[0].u = raw + 52, 1, "entries 0 (Y) and 0 (U) overlap");     // an entry's own planes
    REFUSED(t[0].v = raw, 1, "entries 0 (Y) and 0 (V) overlap");          // ... on one first byte
    REFUSED(t[0].v = raw + 58, 1, "entries 0 (U) and 0 (V) overlap");
    // chroma halves side by side on one pitch: U [54, 60 + 3), V three bytes in: no byte is shared, the RANGES are
    PASSES((t[0].u = raw + 54, t[0].u_row_stride = 6, t[0].v = raw + 57, t[0].v_row_stride = 6), 0);
    REFUSED((t[0].u = raw + 54, t[0].u_row_stride = 6, t[0].v = raw + 57, t[0].v_row_stride = 6), 1, "entries 0 (U) and 0 (V) overlap");
    REFUSED(t[2] = good[1], 1, "entries 1 (V) and 2 (V) overlap");        // the same surface twice: its first plane in memory is named
    REFUSED(t[3].v = apart + 5, 1, "entries 3 (U) and 3 (V) overlap");
    PASSES(t[3].y = raw + 75, 1);                                         // right behind the Y of 1
#undef PASSES
#undef REFUSED

    // ---- the four table entry points.  A table of 3 entries at [0, 168); sim rows, a matte, colour rows, sums and the workspace behind it
    const spk_planar_ref* const table = (const spk_planar_ref*)raw;
    float* const x = (float*)(raw + 1024);                                // src [3,3,4,4]: [1024, 1600)
    float* const sim = (float*)(raw + 2048);
    float* const matte = (float*)(raw + 2304);
    float* const colour = (float*)(raw + 2560);                           // [2560, 2632)
    double* const sums = (double*)(raw + 2816);                           // [2816, 3128)
    float* const dst = (float*)(raw + 4096);                              // the way in's output [3,3,8,8]: [4096, 6400)
    const size_t ws_bytes = 3 * 64 * 13 * 8;                              // three frames: 64 workgroups x 13 doubles each
    void* const ws = (void*)(uintptr_t)0x10000000;                        // never dereferenced: far from raw

    struct In { const spk_planar_ref* table; int N; const float* sim; int standard, full_range; float* dst; int Hout, Wout; };
    const In in_ok = {table, 3, sim, 601, 0, dst, 8, 8};
    In i;
    auto way_in = [&](const In& b) {
        return spk_frames_i420_to_f32_sim_table(b.table, b.N, b.sim, 0, b.standard, b.full_range, b.dst, b.Hout, b.Wout, 1, 1, 1, 0, 0, 0, nullptr);
    };
#define REFUSED(stmt, word) i = in_ok; stmt; CHECK(way_in(i) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED(i.table = nullptr, "null planar table");
    REFUSED(i.table = (const spk_planar_ref*)(raw + 4), "aligned");
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
    REFUSED(i.dst = (float*)(raw + 164), "overlaps dst");                 // dst on the table's last bytes
    REFUSED(i.table = (const spk_planar_ref*)(raw + 6392), "overlaps dst");      // the table on dst's
    REFUSED(i.table = (const spk_planar_ref*)(raw + 4096), "overlaps dst");
    REFUSED((i.N = 0x7fffffff, i.Hout = 0x7fffffff, i.Wout = 1, i.dst = (float*)(raw + 8192)), "overlaps dst");      // 2^62 * 12 bytes and more: the sizes are 64-bit
#undef REFUSED

    struct Paste { const float* src; int N, Hs, Ws; const spk_planar_ref* table; const float* sim; int standard, full_range; double feather;
                   float lo, k; const float* matte; int matte_frames; const float* colour; };
    const Paste paste_ok = {x, 3, 4, 4, table, sim, 709, 1, 2.0, -1.f, 127.5f, matte, 3, colour};
    Paste p;
    auto tpaste = [&](const Paste& b) {
        return spk_frames_paste_i420_sim_table(b.src, b.N, b.Hs, b.Ws, b.table, b.sim, b.standard, b.full_range, b.feather, b.lo, b.k, b.matte,
                                               b.matte_frames, b.colour, nullptr);
    };
    auto tmatch = [&](const Paste& b, double max_gain, double min_sigma, double min_weight, float* out, void* w, size_t wb) {
        return spk_paste_colour_match_i420_sim_table(b.src, b.N, b.Hs, b.Ws, b.table, b.sim, b.standard, b.full_range, b.feather, b.lo, b.k, b.matte,
                                                     b.matte_frames, max_gain, min_sigma, min_weight, out, w, wb, nullptr);
    };
    auto ttotals = [&](const Paste& b, double* out, void* w, size_t wb) {
        return spk_paste_colour_sums_i420_sim_table(b.src, b.N, b.Hs, b.Ws, b.table, b.sim, b.standard, b.full_range, b.feather, b.lo, b.k, b.matte,
                                                    b.matte_frames, out, w, wb, nullptr);
    };
    // what the three share, through each of them
#define REFUSED(stmt, word)                                                                                         \
    p = paste_ok; stmt; CHECK(tpaste(p) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals;        \
    CHECK(tmatch(p, 2.0, 1.0, 16.0, colour, ws, ws_bytes) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals; \
    CHECK(ttotals(p, sums, ws, ws_bytes) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED(p.src = nullptr, "null frame pointer");
    REFUSED(p.table = nullptr, "null planar table");
    REFUSED(p.table = (const spk_planar_ref*)(raw + 12), "aligned");
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
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, nullptr, ws, ws_bytes), "null colour row");
    REFUSED(tmatch(p, 0.999, 1.0, 16.0, colour, ws, ws_bytes), "max_gain");
    REFUSED(tmatch(p, NAN, 1.0, 16.0, colour, ws, ws_bytes), "max_gain");
    REFUSED(tmatch(p, 2.0, -1e-9, 16.0, colour, ws, ws_bytes), "min_sigma");
    REFUSED(tmatch(p, 2.0, 1.0, -1.0, colour, ws, ws_bytes), "min_weight");
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, colour, nullptr, ws_bytes), "workspace");
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, colour, ws, ws_bytes - 1), "workspace");
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, colour, (void*)((uintptr_t)ws + 4), ws_bytes), "aligned");
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, (float*)(raw + 164), ws, ws_bytes), "overlaps the colour rows");   // rows on the table's last bytes
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, (float*)raw, ws, ws_bytes), "overlaps the colour rows");
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, colour, raw + 160, ws_bytes), "overlaps the workspace");
    p.table = (const spk_planar_ref*)(raw + 2624);
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, colour, ws, ws_bytes), "overlaps the colour rows");                // the table on the rows' last bytes
    p = paste_ok;
    REFUSED(ttotals(p, nullptr, ws, ws_bytes), "null sums");
    REFUSED(ttotals(p, (double*)(raw + 2820), ws, ws_bytes), "aligned");
    REFUSED(ttotals(p, sums, nullptr, ws_bytes), "workspace");
    REFUSED(ttotals(p, sums, ws, ws_bytes - 8), "workspace");
    REFUSED(ttotals(p, sums, (void*)((uintptr_t)ws + 2), ws_bytes), "aligned");
    REFUSED(ttotals(p, (double*)(raw + 160), ws, ws_bytes), "overlaps the sums");
    REFUSED(ttotals(p, (double*)raw, ws, ws_bytes), "overlaps the sums");
    REFUSED(ttotals(p, sums, raw + 8, ws_bytes), "overlaps the workspace");
    p.table = (const spk_planar_ref*)(raw + 3120);
    REFUSED(ttotals(p, sums, ws, ws_bytes), "overlaps the sums");                                        // the sums end at 3128
    p = paste_ok, p.table = (const spk_planar_ref*)((uintptr_t)ws + ws_bytes - 8);
    REFUSED(ttotals(p, sums, ws, ws_bytes), "overlaps the workspace");                                   // the table on the workspace's last bytes
#undef REFUSED
    std::printf("i420 host check: %d refusals and %d passes of the nine entry points of the aligned I420 edge\n", refusals, passes);
    return 0;
}
