// Host-side check of the aligned RGB32 edge (csrc/frame_sim_rgb32.hip, csrc/frame_table_rgb32.hip) under AddressSanitizer / UBSan:
// every refusal of the ten entry points -- the five strided ones, spk_frame_table_check_rgb32 (pure host code over a host copy of a
// table: the half-formed entries, a misaligned one and a pitch that is no multiple of 4 among them, the extents that leave 64 bits,
// the overlap cases) and the four _rgb32_sim_table ones -- and the tables that must pass the check: ranges that touch, every entry
// absent, a view at a pixel offset of a wider surface, frames in separate allocations.  Every refusal happens before a launch and
// before anything is dereferenced (the entry points never read a table), so no device is needed.  The two files are linked with
// nothing else: what they share lives in headers.  Build and run from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         speak-hack_amd/csrc/frame_sim_rgb32.hip speak-hack_amd/csrc/frame_table_rgb32.hip tools/rgb32_host_check.cpp \
//         -o tools/_bin/rgb32_host_check
//   tools/_bin/rgb32_host_check
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_check.hpp"

int main() {
    alignas(16) static uint8_t raw[16384];
    alignas(16) static uint8_t apart[64];                                 // a second allocation
    int refusals = 0, passes = 0;

    // ---- the five strided entry points.  One 8 x 8 frame at pitch 32: 256 bytes per frame
    struct Args {
        const float* src; uint8_t* px; const float* sim; float* dst;
        int N, Hs, Ws, H, W; int64_t img, row; int swap_rb, alpha_first; double feather; float lo, k;
        const float* matte; int matte_frames;
        double max_gain, min_sigma, min_weight; float* out; double* sums; void* ws; size_t ws_bytes;       // the statistics only
    };
    float* const f = (float*)(raw + 8192);
    const size_t need1 = 64 * 13 * sizeof(double);                        // spk_paste_colour_match_workspace_bytes(1)
    const Args ok = {f, raw, f, f, 1, 4, 4, 8, 8, 256, 32, 1, 0, 0.0, -1.f, 127.5f, nullptr, 0, 2.0, 1.0, 16.0, f, (double*)f, raw + 1024, 2 * need1};
    auto in = [&](const Args& a) {
        return spk_frames_rgb32_to_f32_sim(a.px, a.img, a.row, a.N, a.H, a.W, a.sim, a.swap_rb, a.alpha_first, a.dst, a.Hs, a.Ws, 1.f, 1.f, 1.f, 0.f,
                                           0.f, 0.f, nullptr);
    };
    auto paste = [&](const Args& a) {
        return spk_frames_paste_rgb32_sim(a.src, a.N, a.Hs, a.Ws, a.px, a.img, a.row, a.H, a.W, a.sim, a.swap_rb, a.alpha_first, a.feather, a.lo, a.k,
                                          nullptr);
    };
    auto blend = [&](const Args& a) {
        return spk_frames_paste_rgb32_sim_blend(a.src, a.N, a.Hs, a.Ws, a.px, a.img, a.row, a.H, a.W, a.sim, a.swap_rb, a.alpha_first, a.feather, a.lo,
                                                a.k, a.matte, a.matte_frames, nullptr, nullptr);
    };
    auto match = [&](const Args& a) {
        return spk_paste_colour_match_rgb32_sim(a.src, a.N, a.Hs, a.Ws, a.px, a.img, a.row, a.H, a.W, a.sim, a.swap_rb, a.alpha_first, a.feather, a.lo,
                                                a.k, a.matte, a.matte_frames, a.max_gain, a.min_sigma, a.min_weight, a.out, a.ws, a.ws_bytes, nullptr);
    };
    auto totals = [&](const Args& a) {
        return spk_paste_colour_sums_rgb32_sim(a.src, a.N, a.Hs, a.Ws, a.px, a.img, a.row, a.H, a.W, a.sim, a.swap_rb, a.alpha_first, a.feather, a.lo,
                                               a.k, a.matte, a.matte_frames, a.sums, a.ws, a.ws_bytes, nullptr);
    };
    Args a;
    // what all five refuse alike: the frames, the rows, the sizes, the strides, the alignment, where the colour is
#define REFUSED(stmt, word)                                                                        \
    a = ok; stmt; CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));               \
    CHECK(paste(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));                          \
    CHECK(blend(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));                          \
    CHECK(match(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));                          \
    CHECK(totals(a) == SPK_EINVAL && std::strstr(spk_last_error(), word)); refusals += 5
    REFUSED(a.px = nullptr, "null frame pointer");
    REFUSED(a.sim = nullptr, "transform");
    REFUSED(a.N = 0, "N / H / W");
    REFUSED(a.N = -3, "N / H / W");
    REFUSED(a.H = 0, "N / H / W");
    REFUSED(a.W = -8, "N / H / W");
    REFUSED(a.row = 31, "smaller than 4 * W");
    REFUSED(a.row = 24, "smaller than 4 * W");                            // the packed pitch 3 W
    REFUSED(a.row = -32, "smaller than 4 * W");
    REFUSED(a.W = 0x7fffffff, "smaller than 4 * W");                      // 4 W is formed in 64 bits
    REFUSED(a.row = 33, "not a multiple of 4");
    REFUSED(a.row = 34, "not a multiple of 4");
    REFUSED(a.row = 35, "not a multiple of 4");
    REFUSED((a.N = 2, a.img = 258), "image stride 258 is not a multiple of 4");
    REFUSED(a.px = raw + 1, "aligned to 4 bytes");
    REFUSED(a.px = raw + 2, "aligned to 4 bytes");
    REFUSED(a.px = raw + 3, "aligned to 4 bytes");
    REFUSED(a.alpha_first = 2, "alpha_first");
    REFUSED(a.alpha_first = -1, "alpha_first");
#undef REFUSED
    a = ok; a.Hs = 0; CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), "N / H / W")); ++refusals;
    a = ok; a.dst = nullptr; CHECK(in(a) == SPK_EINVAL && std::strstr(spk_last_error(), "null frame pointer")); ++refusals;
    // two frames: a negative stride for the way in, which reads; overlap for the four that share the paste's checks
#define REFUSED2(call, stmt, word) a = ok; a.N = 2; stmt; CHECK(call(a) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED2(in, a.img = -256, "negative");
    REFUSED2(paste, a.img = 252, "overlap");                              // two frames of 8 rows of pitch 32 overlap below 7 * 32 + 32
    REFUSED2(blend, a.img = 0, "overlap");
    REFUSED2(match, a.img = -256, "overlap");
    REFUSED2(totals, a.img = 128, "overlap");
    REFUSED2(paste, (a.H = 0x7ffffffe, a.img = 256), "overlap");          // (H - 1) * row stride does not wrap
#undef REFUSED2
    // the way out and its statistics
#define REFUSED(stmt, word)                                                                        \
    a = ok; stmt; CHECK(paste(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));            \
    CHECK(blend(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));                          \
    CHECK(match(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));                          \
    CHECK(totals(a) == SPK_EINVAL && std::strstr(spk_last_error(), word)); refusals += 4
    REFUSED(a.src = nullptr, "null frame pointer");
    REFUSED(a.Hs = 0, "N / H / W");
    REFUSED(a.Ws = -1, "N / H / W");
    REFUSED(a.feather = -0.5, "feather");
    REFUSED(a.feather = NAN, "feather");
    REFUSED(a.feather = INFINITY, "feather");
    REFUSED(a.lo = NAN, "value range");
    REFUSED(a.k = 0.f, "value range");
    REFUSED(a.k = INFINITY, "value range");
#undef REFUSED
#define REFUSED(stmt, word)                                                                        \
    a = ok; stmt; CHECK(blend(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));            \
    CHECK(match(a) == SPK_EINVAL && std::strstr(spk_last_error(), word));                          \
    CHECK(totals(a) == SPK_EINVAL && std::strstr(spk_last_error(), word)); refusals += 3
    REFUSED(a.matte_frames = 1, "matte_frames");                          // frames of a matte that is not there
    REFUSED(a.matte_frames = -1, "matte_frames");
    REFUSED((a.N = 2, a.img = 256, a.matte = f, a.matte_frames = 0), "matte_frames");
    REFUSED((a.N = 2, a.img = 256, a.matte = f, a.matte_frames = 3), "matte_frames");
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
    // (frames the strided checks let through are launched, so the frames that must pass are asked of the table check below)

    // ---- spk_frame_table_check_rgb32.  Entry 0: 4 x 6 at pitch 32, [0, 120).  Entry 1: 2 x 2 packed, [120, 136): it TOUCHES entry 0.
    // Entry 2: absent.  Entry 3: a 3 x 5 view at pixel offset (1, 2) of a 6 x 8 surface at pitch 48 that begins at 4096: from 4152,
    // 4-aligned and not 16-aligned.  Entry 4: 1 x 1 in `apart`
    const spk_frame_ref good[5] = {{raw, 32, 4, 6}, {raw + 120, 8, 2, 2}, {nullptr, 0, 0, 0}, {raw + 4096 + 48 + 8, 48, 3, 5}, {apart, 4, 1, 1}};
    spk_frame_ref t[5];
#define PASSES(stmt, written) std::memcpy(t, good, sizeof t); stmt; CHECK(spk_frame_table_check_rgb32(t, 5, written) == SPK_OK); ++passes
#define REFUSED(stmt, written, word) std::memcpy(t, good, sizeof t); stmt; \
    CHECK(spk_frame_table_check_rgb32(t, 5, written) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    PASSES((void)0, 0);
    PASSES((void)0, 1);                      // ranges that touch, a view at a pixel offset, a frame in `apart`
    CHECK(spk_frame_table_check_rgb32(nullptr, 5, 0) == SPK_EINVAL && std::strstr(spk_last_error(), "null"));
    ++refusals;
    CHECK(spk_frame_table_check_rgb32(good, 0, 0) == SPK_EINVAL && std::strstr(spk_last_error(), "N must"));
    ++refusals;
    CHECK(spk_frame_table_check_rgb32(good, -5, 1) == SPK_EINVAL && std::strstr(spk_last_error(), "N must"));
    ++refusals;
    // half-formed: not usable and not all zero
    REFUSED(t[0].data = nullptr, 0, "entry 0 is half-formed");
    REFUSED(t[1].H = 0, 0, "entry 1 is half-formed");
    REFUSED(t[3].H = -2, 1, "entry 3 is half-formed");
    REFUSED(t[0].W = 0, 0, "entry 0 is half-formed");
    REFUSED(t[0].W = -6, 0, "entry 0 is half-formed");
    REFUSED(t[0].row_stride = 23, 0, "entry 0 is half-formed");           // W = 6: below 4 W
    REFUSED(t[0].row_stride = 20, 0, "entry 0 is half-formed");           // a multiple of 4 below 4 W (above the packed 3 W)
    REFUSED(t[0].row_stride = -32, 1, "entry 0 is half-formed");
    REFUSED(t[0].row_stride = 26, 0, "entry 0 is half-formed");           // no multiple of 4
    REFUSED(t[0].row_stride = 33, 1, "entry 0 is half-formed");
    REFUSED(t[0].data = raw + 1, 0, "entry 0 is half-formed");            // a misaligned first pixel
    REFUSED(t[1].data = raw + 122, 1, "entry 1 is half-formed");
    REFUSED(t[3].data = raw + 4096 + 3, 0, "entry 3 is half-formed");
    REFUSED(t[4].data = apart + 7, 0, "entry 4 is half-formed");
    REFUSED(t[2].data = raw + 512, 0, "entry 2 is half-formed");          // an absent frame with a pointer left in it
    REFUSED(t[2].row_stride = 8, 0, "entry 2 is half-formed");
    REFUSED(t[2].H = 2, 1, "entry 2 is half-formed");
    REFUSED(t[2].W = 2, 1, "entry 2 is half-formed");
    REFUSED((t[0].row_stride = 0, t[0].H = 0, t[0].W = 0), 0, "entry 0 is half-formed");
    PASSES(t[0].row_stride = 24, 1);                                      // the smallest stride
    PASSES(std::memset(t, 0, sizeof t), 1);                               // every entry absent
    PASSES((t[0] = good[3], t[3] = good[0]), 1);                          // entries out of address order
    PASSES(t[1].data = apart + 16, 1);                                    // two frames in the second allocation
    PASSES(t[4].data = raw + 136, 1);                                     // right behind entry 1
    PASSES((t[3].data = raw + 4096 + 2 * 48 + 4 * 7, t[3].H = 4, t[3].W = 1), 1);      // another view: one pixel wide, its rows far apart
    // extents that leave 64 bits: (H - 1) * row_stride, + 4 W, and the address behind the last byte
    REFUSED(t[0].row_stride = (int64_t)1 << 62, 0, "entry 0: the extent");                       // 3 * 2^62
    REFUSED((t[0].H = INT32_MAX - 1, t[0].row_stride = (int64_t)1 << 33), 0, "entry 0: the extent");
    REFUSED(t[1].data = (const uint8_t*)(UINTPTR_MAX - 7), 0, "entry 1: the extent");            // data + 16 wraps
    REFUSED(t[4].data = (const uint8_t*)(UINTPTR_MAX - 3), 1, "entry 4: the extent");            // data + 4 wraps
    PASSES(t[4].row_stride = (int64_t)1 << 62, 1);                        // one row: its stride does not count
    // overlap: tolerated when the frames are read, refused when they are written
    PASSES(t[1].data = raw + 116, 0);
    REFUSED(t[1].data = raw + 116, 1, "entries 0 (RGB32) and 1 (RGB32) overlap");                // the last pixel of entry 0
    PASSES(t[1].data = raw + 28, 0);
    REFUSED(t[1].data = raw + 28, 1, "entries 0 (RGB32) and 1 (RGB32) overlap");                 // inside the pitch padding of 0: its byte RANGE
    REFUSED(t[4].data = raw + 4096 + 48 * 3 + 24, 1, "entries 3 (RGB32) and 4 (RGB32) overlap");
    REFUSED(t[2] = good[1], 1, "entries 1 (RGB32) and 2 (RGB32) overlap");                       // the same frame twice
    REFUSED(t[4] = good[0], 1, "entries 0 (RGB32) and 4 (RGB32) overlap");
#undef PASSES
#undef REFUSED

    // ---- the four table entry points.  A table of 3 entries at [0, 72); sim rows, a matte, colour rows, sums and the workspace behind it
    const spk_frame_ref* const table = (const spk_frame_ref*)raw;
    float* const x = (float*)(raw + 1024);                                // src [3,3,4,4]: [1024, 1600)
    float* const sim = (float*)(raw + 2048);
    float* const matte = (float*)(raw + 2304);
    float* const colour = (float*)(raw + 2560);                           // [2560, 2632)
    double* const sums = (double*)(raw + 2816);                           // [2816, 3128)
    float* const dst = (float*)(raw + 4096);                              // the way in's output [3,3,8,8]: [4096, 6400)
    const size_t ws_bytes = 3 * 64 * 13 * 8;                              // three frames: 64 workgroups x 13 doubles each
    void* const ws = (void*)(uintptr_t)0x10000000;                        // never dereferenced: far from raw

    struct In { const spk_frame_ref* table; int N; const float* sim; int alpha_first; float* dst; int Hout, Wout; };
    const In in_ok = {table, 3, sim, 1, dst, 8, 8};
    In i;
    auto way_in = [&](const In& b) {
        return spk_frames_rgb32_to_f32_sim_table(b.table, b.N, b.sim, 0, b.alpha_first, b.dst, b.Hout, b.Wout, 1, 1, 1, 0, 0, 0, nullptr);
    };
#define REFUSED(stmt, word) i = in_ok; stmt; CHECK(way_in(i) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED(i.table = nullptr, "null frame table");
    REFUSED(i.table = (const spk_frame_ref*)(raw + 4), "aligned");
    REFUSED(i.N = 0, "N must");
    REFUSED(i.N = -3, "N must");
    REFUSED(i.sim = nullptr, "null transform");
    REFUSED(i.dst = nullptr, "null frame pointer");
    REFUSED(i.Hout = 0, "output size");
    REFUSED(i.Wout = -8, "output size");
    REFUSED(i.alpha_first = 2, "alpha_first");
    REFUSED(i.alpha_first = -1, "alpha_first");
    REFUSED(i.dst = (float*)(raw + 68), "overlaps dst");                  // dst on the table's last bytes
    REFUSED(i.table = (const spk_frame_ref*)(raw + 6392), "overlaps dst");       // the table on dst's
    REFUSED(i.table = (const spk_frame_ref*)(raw + 4096), "overlaps dst");
    REFUSED((i.N = 0x7fffffff, i.Hout = 0x7fffffff, i.Wout = 1, i.dst = (float*)(raw + 8192)), "overlaps dst");      // 2^62 * 12 bytes and more: the sizes are 64-bit
#undef REFUSED

    struct Paste { const float* src; int N, Hs, Ws; const spk_frame_ref* table; const float* sim; int swap_rb, alpha_first; double feather;
                   float lo, k; const float* matte; int matte_frames; const float* colour; };
    const Paste paste_ok = {x, 3, 4, 4, table, sim, 1, 0, 2.0, -1.f, 127.5f, matte, 3, colour};
    Paste p;
    auto tpaste = [&](const Paste& b) {
        return spk_frames_paste_rgb32_sim_table(b.src, b.N, b.Hs, b.Ws, b.table, b.sim, b.swap_rb, b.alpha_first, b.feather, b.lo, b.k, b.matte,
                                                b.matte_frames, b.colour, nullptr);
    };
    auto tmatch = [&](const Paste& b, double max_gain, double min_sigma, double min_weight, float* out, void* w, size_t wb) {
        return spk_paste_colour_match_rgb32_sim_table(b.src, b.N, b.Hs, b.Ws, b.table, b.sim, b.swap_rb, b.alpha_first, b.feather, b.lo, b.k, b.matte,
                                                      b.matte_frames, max_gain, min_sigma, min_weight, out, w, wb, nullptr);
    };
    auto ttotals = [&](const Paste& b, double* out, void* w, size_t wb) {
        return spk_paste_colour_sums_rgb32_sim_table(b.src, b.N, b.Hs, b.Ws, b.table, b.sim, b.swap_rb, b.alpha_first, b.feather, b.lo, b.k, b.matte,
                                                     b.matte_frames, out, w, wb, nullptr);
    };
    // what the three share, through each of them
#define REFUSED(stmt, word)                                                                                         \
    p = paste_ok; stmt; CHECK(tpaste(p) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals;        \
    CHECK(tmatch(p, 2.0, 1.0, 16.0, colour, ws, ws_bytes) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals; \
    CHECK(ttotals(p, sums, ws, ws_bytes) == SPK_EINVAL && std::strstr(spk_last_error(), word)); ++refusals
    REFUSED(p.src = nullptr, "null frame pointer");
    REFUSED(p.table = nullptr, "null frame table");
    REFUSED(p.table = (const spk_frame_ref*)(raw + 12), "aligned");
    REFUSED(p.N = 0, "N must");
    REFUSED(p.N = -1, "N must");
    REFUSED(p.sim = nullptr, "null transform");
    REFUSED(p.Hs = 0, "source size");
    REFUSED(p.Ws = -4, "source size");
    REFUSED(p.alpha_first = 2, "alpha_first");
    REFUSED(p.alpha_first = -1, "alpha_first");
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
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, nullptr, ws, ws_bytes), "null colour row");
    REFUSED(tmatch(p, 0.999, 1.0, 16.0, colour, ws, ws_bytes), "max_gain");
    REFUSED(tmatch(p, NAN, 1.0, 16.0, colour, ws, ws_bytes), "max_gain");
    REFUSED(tmatch(p, 2.0, -1e-9, 16.0, colour, ws, ws_bytes), "min_sigma");
    REFUSED(tmatch(p, 2.0, 1.0, -1.0, colour, ws, ws_bytes), "min_weight");
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, colour, nullptr, ws_bytes), "workspace");
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, colour, ws, ws_bytes - 1), "workspace");
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, colour, (void*)((uintptr_t)ws + 4), ws_bytes), "aligned");
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, (float*)(raw + 68), ws, ws_bytes), "overlaps the colour rows");    // rows on the table's last bytes
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, (float*)raw, ws, ws_bytes), "overlaps the colour rows");
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, colour, raw + 64, ws_bytes), "overlaps the workspace");
    p.table = (const spk_frame_ref*)(raw + 2624);
    REFUSED(tmatch(p, 2.0, 1.0, 16.0, colour, ws, ws_bytes), "overlaps the colour rows");                // the table on the rows' last bytes
    p = paste_ok;
    REFUSED(ttotals(p, nullptr, ws, ws_bytes), "null sums");
    REFUSED(ttotals(p, (double*)(raw + 2820), ws, ws_bytes), "aligned");
    REFUSED(ttotals(p, sums, nullptr, ws_bytes), "workspace");
    REFUSED(ttotals(p, sums, ws, ws_bytes - 8), "workspace");
    REFUSED(ttotals(p, sums, (void*)((uintptr_t)ws + 2), ws_bytes), "aligned");
    REFUSED(ttotals(p, (double*)(raw + 64), ws, ws_bytes), "overlaps the sums");
    REFUSED(ttotals(p, (double*)raw, ws, ws_bytes), "overlaps the sums");
    REFUSED(ttotals(p, sums, raw + 8, ws_bytes), "overlaps the workspace");
    p.table = (const spk_frame_ref*)(raw + 3120);
    REFUSED(ttotals(p, sums, ws, ws_bytes), "overlaps the sums");                                        // the sums end at 3128
    p = paste_ok, p.table = (const spk_frame_ref*)((uintptr_t)ws + ws_bytes - 8);
    REFUSED(ttotals(p, sums, ws, ws_bytes), "overlaps the workspace");                                   // the table on the workspace's last bytes
#undef REFUSED
    std::printf("rgb32 host check: %d refusals and %d passes of the ten entry points of the aligned RGB32 edge\n", refusals, passes);
    return 0;
}
