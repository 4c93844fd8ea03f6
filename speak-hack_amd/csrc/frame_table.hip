// The aligned video edge over a FRAME TABLE (include/spk.h has the definitions): every frame in a buffer of its own, of its own
// size -- what a server with several calls holds, each call's decoder delivering into its own surface at its own resolution.
//   frames_u8_to_f32_sim_table:      the way in of csrc/frame_sim.hip;
//   frames_paste_u8_sim_table:       the paste of csrc/frame_sim.hip / csrc/frame_blend.hip (matte and colour rows may be NULL);
//   paste_colour_{sums,match}_sim_table: the statistics of csrc/frame_blend.hip.
// The kernels are the templates of csrc/frame_sim_common.hpp and csrc/frame_blend_common.hpp: this file holds a third way to say
// where a frame is, beside byte strides and NV12 planes -- entry n of a device table of spk_frame_ref -- and nothing else.  The
// work decomposition of the three kernels does not depend on the frame size (the way in walks output tiles, the paste and the sums
// walk each frame's own region box under blockIdx.y), so frame n of a table is bit for bit the strided launch at N = 1 on entry n.
// The kernels read the table, the entry points never do: an entry is judged in the kernel, before an address is formed from it,
// and one that is not usable means the frame is absent -- it is treated exactly like an invalid row.  spk_frame_table_check is what
// a binder runs over its HOST copy before it uploads.
#include <algorithm>
#include <numeric>
#include <vector>

#include "frame_blend_common.hpp"
#include "frame_table_common.hpp"

static_assert(sizeof(spk_frame_ref) == 24 && alignof(spk_frame_ref) == 8, "spk_frame_ref is 8 + 8 + 4 + 4 bytes");

namespace {

using namespace spk::frame;

// Entry n as a kernel holds it: loaded once per frame (paste, statistics: n comes from blockIdx.y) or once per tile (way in: n is
// the wave's), outside the pixel loops.
struct TableFrame {
    const uint8_t* data;
    long long row_stride;
    int H, W;
    __device__ __forceinline__ bool usable() const { return data != nullptr && H >= 1 && W >= 1 && row_stride >= 3ll * W; }
};

__device__ __forceinline__ TableFrame load_frame(const spk_frame_ref* __restrict__ table, long long n) {
    const spk_frame_ref e = table[n];
    return {e.data, (long long)e.row_stride, e.H, e.W};
}

struct TableSource : RgbTaps {          // the way in
    const spk_frame_ref* table;
    __device__ __forceinline__ TableFrame frame(long long n, int, int) const { return load_frame(table, n); }
    __device__ __forceinline__ const uint8_t* row(const TableFrame& f, long long, int iy) const { return f.data + (long long)iy * f.row_stride; }
};

struct TableBackground {                // the statistics
    const spk_frame_ref* table;
    int swap_rb;
    __device__ __forceinline__ TableFrame frame(long long n, int, int) const { return load_frame(table, n); }
    __device__ __forceinline__ void load(const TableFrame& f, long long, int X, int Y, double (&b)[3]) const {
        rgb_background(f.data + (long long)Y * f.row_stride + (long long)X * 3, swap_rb, b);
    }
};

struct TableTarget {                    // the paste: the frames of a table that is pasted into are the caller's to write
    const spk_frame_ref* table;
    __device__ __forceinline__ TableFrame frame(long long n, int, int) const { return load_frame(table, n); }
    __device__ __forceinline__ uint8_t* pixel(const TableFrame& f, long long, int X, int Y) const {
        return const_cast<uint8_t*>(f.data) + (long long)Y * f.row_stride + (long long)X * 3;
    }
};

// ---- host (ranges_overlap, bytes_of, check_table and check_table_apart: csrc/frame_table_common.hpp) ----
// what the tabled paste and its statistics check alike: check_paste_u8 without the frames' own pointer, strides and size
int check_paste_table(const char* who, const void* src, const spk_frame_ref* table_dev, const float* sim_dev, int N, int Hs, int Ws, double feather,
                      float lo, float k, const float* matte_dev, int matte_frames) {
    SPK_REQUIRE(src, "%s: null frame pointer", who);
    if (int rc = check_table(who, table_dev, N)) return rc;
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(Hs >= 1 && Ws >= 1, "%s: the source size must be >= 1 (got %d x %d)", who, Hs, Ws);
    return check_blend_params(who, N, feather, lo, k, matte_dev, matte_frames);
}

// the extent in bytes of a usable entry, (H - 1) row_stride + 3 W; false when it, or the address behind it, leaves 64 bits
bool entry_extent(const spk_frame_ref& e, unsigned long long* extent) {
    long long rows, bytes;
    if (__builtin_mul_overflow((long long)(e.H - 1), (long long)e.row_stride, &rows)) return false;
    if (__builtin_add_overflow(rows, 3ll * e.W, &bytes)) return false;
    unsigned long long end;
    if (__builtin_add_overflow((unsigned long long)(uintptr_t)e.data, (unsigned long long)bytes, &end)) return false;
    *extent = (unsigned long long)bytes;
    return true;
}

}  // namespace

extern "C" {

int spk_frame_table_check(const spk_frame_ref* host_table, int N, int written) {
    const char* who = "frame_table_check";
    SPK_REQUIRE(host_table, "%s: null frame table", who);
    SPK_REQUIRE(N >= 1, "%s: N must be >= 1 (got %d)", who, N);
    std::vector<int> usable;
    std::vector<unsigned long long> extent((size_t)N, 0ull);
    for (int n = 0; n < N; ++n) {
        const spk_frame_ref& e = host_table[n];
        if (e.data != nullptr && e.H >= 1 && e.W >= 1 && e.row_stride >= 3ll * e.W) {
            SPK_REQUIRE(entry_extent(e, &extent[(size_t)n]), "%s: entry %d: the extent (H - 1) * row_stride + 3 * W of %d x %d with row stride %lld "
                        "overflows 64 bits", who, n, e.H, e.W, (long long)e.row_stride);
            usable.push_back(n);
            continue;
        }
        SPK_REQUIRE(e.data == nullptr && e.row_stride == 0 && e.H == 0 && e.W == 0,
                    "%s: entry %d is half-formed: data %p, row stride %lld, %d x %d is neither usable (data, H >= 1, W >= 1, row stride >= 3 W) "
                    "nor all zero (an absent frame)", who, n, (const void*)e.data, (long long)e.row_stride, e.H, e.W);
    }
    if (!written) return SPK_OK;
    // frames that are written must not share a byte: in the order of their first bytes, each must begin where the ones before it ended
    std::sort(usable.begin(), usable.end(), [&](int a, int b) {
        const uintptr_t pa = (uintptr_t)host_table[a].data, pb = (uintptr_t)host_table[b].data;
        return pa != pb ? pa < pb : a < b;
    });
    for (size_t i = 1, last = 0; i < usable.size(); ++i) {               // last: the entry before i that ends furthest
        const int a = usable[last], b = usable[i];
        const uintptr_t a_end = (uintptr_t)host_table[a].data + extent[(size_t)a], b0 = (uintptr_t)host_table[b].data;
        SPK_REQUIRE(b0 >= a_end, "%s: entries %d and %d overlap: frames that are written must not share bytes", who, std::min(a, b), std::max(a, b));
        if (b0 + extent[(size_t)b] > a_end) last = i;
    }
    return SPK_OK;
}

int spk_frames_u8_to_f32_sim_table(const spk_frame_ref* table_dev, int N, const float* sim_dev, int swap_rb, float* dst, int Hout, int Wout,
                                   float scale0, float scale1, float scale2, float shift0, float shift1, float shift2, void* stream) {
    const char* who = "frames_u8_to_f32_sim_table";
    if (int rc = check_table(who, table_dev, N)) return rc;
    SPK_REQUIRE(dst, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(Hout >= 1 && Wout >= 1, "%s: the output size must be >= 1 (got %d x %d)", who, Hout, Wout);
    if (int rc = check_table_apart(who, table_dev, N, dst, bytes_of(bytes_of((unsigned long long)N * 12ull, (unsigned long long)Hout), (unsigned long long)Wout),
                                   "dst"))
        return rc;
    return launch_frames_to_f32_sim("frames_u8_to_f32_sim_kernel<table>", TableSource{{}, table_dev}, N, 0, 0, sim_dev, swap_rb, dst, Hout, Wout,
                                    Affine3{{scale0, scale1, scale2}, {shift0, shift1, shift2}}, stream);
}

int spk_frames_paste_u8_sim_table(const float* src, int N, int Hs, int Ws, const spk_frame_ref* table_dev, const float* sim_dev, int swap_rb,
                                  double feather, float lo, float k, const float* matte_dev, int matte_frames, const float* colour_dev,
                                  void* stream) {
    const char* who = "frames_paste_u8_sim_table";
    if (int rc = check_paste_table(who, src, table_dev, sim_dev, N, Hs, Ws, feather, lo, k, matte_dev, matte_frames)) return rc;
    const TableTarget out{table_dev};
    if (!matte_dev && !colour_dev)                                        // the plain instance: matte and colour rows absent at compile time
        return launch_paste_sim<false>("frames_paste_u8_sim_kernel<table>", src, N, Hs, Ws, out, 0, 0, sim_dev, swap_rb, feather, lo, k, nullptr, 0,
                                       nullptr, stream);
    return launch_paste_sim<true>("frames_paste_u8_sim_blend_kernel<table>", src, N, Hs, Ws, out, 0, 0, sim_dev, swap_rb, feather, lo, k, matte_dev,
                                  matte_frames, colour_dev, stream);
}

int spk_paste_colour_match_sim_table(const float* src, int N, int Hs, int Ws, const spk_frame_ref* table_dev, const float* sim_dev, int swap_rb,
                                     double feather, float lo, float k, const float* matte_dev, int matte_frames, double max_gain,
                                     double min_sigma, double min_weight, float* colour_out_dev, void* workspace_dev, size_t workspace_bytes,
                                     void* stream) {
    const char* who = "paste_colour_match_sim_table";
    if (int rc = check_paste_table(who, src, table_dev, sim_dev, N, Hs, Ws, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_match(who, N, max_gain, min_sigma, min_weight, colour_out_dev, workspace_dev, workspace_bytes)) return rc;
    if (int rc = check_table_apart(who, table_dev, N, colour_out_dev, (unsigned long long)N * 6ull * sizeof(float), "the colour rows")) return rc;
    if (int rc = check_table_apart(who, table_dev, N, workspace_dev, (unsigned long long)colour_match_workspace_bytes(N), "the workspace")) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<table>", TableBackground{table_dev, swap_rb}, src, N, Hs, Ws, 0, 0, sim_dev, feather, lo,
                                    k, matte_dev, matte_frames, workspace_dev, ColourFinish{colour_out_dev, max_gain, min_sigma, min_weight, nullptr},
                                    stream);
}

int spk_paste_colour_sums_sim_table(const float* src, int N, int Hs, int Ws, const spk_frame_ref* table_dev, const float* sim_dev, int swap_rb,
                                    double feather, float lo, float k, const float* matte_dev, int matte_frames, double* sums_out_dev,
                                    void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_sums_sim_table";
    if (int rc = check_paste_table(who, src, table_dev, sim_dev, N, Hs, Ws, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_sums(who, N, sums_out_dev, workspace_dev, workspace_bytes)) return rc;
    if (int rc = check_table_apart(who, table_dev, N, sums_out_dev, (unsigned long long)N * SUMS * sizeof(double), "the sums")) return rc;
    if (int rc = check_table_apart(who, table_dev, N, workspace_dev, (unsigned long long)colour_match_workspace_bytes(N), "the workspace")) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<table>", TableBackground{table_dev, swap_rb}, src, N, Hs, Ws, 0, 0, sim_dev, feather, lo,
                                    k, matte_dev, matte_frames, workspace_dev, ColourFinish{nullptr, 0.0, 0.0, 0.0, sums_out_dev}, stream);
}

}  // extern "C"
