// The aligned RGB32 edge over a FRAME TABLE (include/spk.h has the definitions): every frame in a buffer of its own, of its own size
// -- what a server holds whose calls arrive as capture surfaces or interop textures, each at its own resolution.  The entries are
// the 24-byte spk_frame_ref of csrc/frame_table.hip: (data, row_stride, H, W) says where an RGB32 frame is as well as a packed one.
//   frames_rgb32_to_f32_sim_table:          the way in of csrc/frame_sim_rgb32.hip;
//   frames_paste_rgb32_sim_table:           its paste (matte and colour rows may be NULL);
//   paste_colour_{sums,match}_rgb32_sim_table: its statistics.
// The kernels are the templates of csrc/frame_sim_common.hpp and csrc/frame_blend_common.hpp, the pixel is
// csrc/frame_rgb32_common.hpp's: this file holds where a tabled frame's bytes are, and nothing else.  The work decomposition of the
// three kernels does not depend on the size, so frame n of a table is bit for bit the strided launch at N = 1 on entry n.  The
// kernels read the table, the entry points never do: an entry is judged in the kernel, with the whole predicate -- the alignment of
// data and row_stride included -- before an address is formed from it, and one that is not usable means the frame is absent: it is
// treated exactly like an invalid row.  spk_frame_table_check_rgb32 is what a binder runs over its HOST copy before it uploads.
#include "frame_rgb32_common.hpp"
#include "frame_table_common.hpp"

namespace {

using namespace spk::frame;

// Entry n as a kernel holds it: loaded once per frame (paste, statistics) or once per tile (way in), outside the pixel loops.
struct TableFrame32 {
    const uint8_t* data;
    long long row_stride;
    int H, W;
    __device__ __forceinline__ bool usable() const {
        return data != nullptr && H >= 1 && W >= 1 && row_stride >= 4ll * W && !(row_stride & 3) && !((uintptr_t)data & 3);
    }
};

__device__ __forceinline__ TableFrame32 load_frame(const spk_frame_ref* __restrict__ table, long long n) {
    const spk_frame_ref e = table[n];
    return {e.data, (long long)e.row_stride, e.H, e.W};
}

struct TableSource32 : Rgb32Taps {      // the way in
    const spk_frame_ref* table;
    __device__ __forceinline__ TableFrame32 frame(long long n, int, int) const { return load_frame(table, n); }
    __device__ __forceinline__ const uint8_t* row(const TableFrame32& f, long long, int iy) const { return f.data + (long long)iy * f.row_stride; }
};

struct TableBackground32 {              // the statistics
    const spk_frame_ref* table;
    int swap_rb, shift0;
    __device__ __forceinline__ TableFrame32 frame(long long n, int, int) const { return load_frame(table, n); }
    __device__ __forceinline__ void load(const TableFrame32& f, long long, int X, int Y, double (&b)[3]) const {
        rgb32_background(f.data + (long long)Y * f.row_stride, X, shift0, swap_rb, b);
    }
};

struct TableTarget32 {                  // the paste: the frames of a table that is pasted into are the caller's to write
    const spk_frame_ref* table;
    int shift0;
    __device__ __forceinline__ TableFrame32 frame(long long n, int, int) const { return load_frame(table, n); }
    __device__ __forceinline__ Rgb32Pixel pixel(const TableFrame32& f, long long, int X, int Y) const {
        return {reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(f.data) + (long long)Y * f.row_stride) + X, shift0};
    }
};

// ---- host (ranges, byte counts, check_table, plane_extent and check_planes_apart: csrc/frame_table_common.hpp) ----
// what the tabled paste and its statistics check alike
int check_paste_table(const char* who, const void* src, const spk_frame_ref* table_dev, const float* sim_dev, int N, int Hs, int Ws, int alpha_first,
                      double feather, float lo, float k, const float* matte_dev, int matte_frames) {
    SPK_REQUIRE(src, "%s: null frame pointer", who);
    if (int rc = check_table(who, table_dev, N)) return rc;
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(Hs >= 1 && Ws >= 1, "%s: the source size must be >= 1 (got %d x %d)", who, Hs, Ws);
    if (int rc = check_alpha_first(who, alpha_first)) return rc;
    return check_blend_params(who, N, feather, lo, k, matte_dev, matte_frames);
}

bool entry_usable(const spk_frame_ref& e) {
    return e.data != nullptr && e.H >= 1 && e.W >= 1 && e.row_stride >= 4ll * e.W && e.row_stride % 4 == 0 && (uintptr_t)e.data % 4 == 0;
}

}  // namespace

extern "C" {

int spk_frame_table_check_rgb32(const spk_frame_ref* host_table, int N, int written) {
    const char* who = "frame_table_check_rgb32";
    SPK_REQUIRE(host_table, "%s: null frame table", who);
    SPK_REQUIRE(N >= 1, "%s: N must be >= 1 (got %d)", who, N);
    static const char* const names[1] = {"RGB32"};
    std::vector<PlaneRange> frames;
    for (int n = 0; n < N; ++n) {
        const spk_frame_ref& e = host_table[n];
        if (entry_usable(e)) {
            SPK_REQUIRE(e.W <= INT32_MAX / 4, "%s: entry %d: 4 * W overflows a row of %d pixels", who, n, e.W);
            unsigned long long bytes;                                 // a frame is one plane of H rows of 4 W bytes
            SPK_REQUIRE(plane_extent(e.data, e.H, e.row_stride, 4 * e.W, &bytes), "%s: entry %d: the extent (H - 1) * row_stride + 4 * W of %d x %d "
                        "with row stride %lld overflows 64 bits", who, n, e.H, e.W, (long long)e.row_stride);
            frames.push_back({(uintptr_t)e.data, bytes, n, 0});
            continue;
        }
        SPK_REQUIRE(e.data == nullptr && e.row_stride == 0 && e.H == 0 && e.W == 0,
                    "%s: entry %d is half-formed: data %p, row stride %lld, %d x %d is neither usable (data aligned to 4, H >= 1, W >= 1, a row "
                    "stride >= 4 W that is a multiple of 4) nor all zero (an absent frame)", who, n, (const void*)e.data, (long long)e.row_stride,
                    e.H, e.W);
    }
    return written ? check_planes_apart(who, frames, names) : SPK_OK;
}

int spk_frames_rgb32_to_f32_sim_table(const spk_frame_ref* table_dev, int N, const float* sim_dev, int swap_rb, int alpha_first, float* dst,
                                      int Hout, int Wout, float scale0, float scale1, float scale2, float shift0, float shift1, float shift2,
                                      void* stream) {
    const char* who = "frames_rgb32_to_f32_sim_table";
    if (int rc = check_table(who, table_dev, N)) return rc;
    SPK_REQUIRE(dst, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(Hout >= 1 && Wout >= 1, "%s: the output size must be >= 1 (got %d x %d)", who, Hout, Wout);
    if (int rc = check_alpha_first(who, alpha_first)) return rc;
    if (int rc = check_table_apart(who, table_dev, N, dst, bytes_of(bytes_of((unsigned long long)N * 12ull, (unsigned long long)Hout), (unsigned long long)Wout),
                                   "dst"))
        return rc;
    return launch_frames_to_f32_sim("frames_rgb32_to_f32_sim_kernel<table>", TableSource32{{8 * alpha_first}, table_dev}, N, 0, 0, sim_dev, swap_rb, dst,
                                    Hout, Wout, Affine3{{scale0, scale1, scale2}, {shift0, shift1, shift2}}, stream);
}

int spk_frames_paste_rgb32_sim_table(const float* src, int N, int Hs, int Ws, const spk_frame_ref* table_dev, const float* sim_dev, int swap_rb,
                                     int alpha_first, double feather, float lo, float k, const float* matte_dev, int matte_frames,
                                     const float* colour_dev, void* stream) {
    const char* who = "frames_paste_rgb32_sim_table";
    if (int rc = check_paste_table(who, src, table_dev, sim_dev, N, Hs, Ws, alpha_first, feather, lo, k, matte_dev, matte_frames)) return rc;
    const TableTarget32 out{table_dev, 8 * alpha_first};
    if (!matte_dev && !colour_dev)                                        // the plain instance: matte and colour rows absent at compile time
        return launch_paste_sim<false>("frames_paste_rgb32_sim_kernel<table>", src, N, Hs, Ws, out, 0, 0, sim_dev, swap_rb, feather, lo, k, nullptr, 0,
                                       nullptr, stream);
    return launch_paste_sim<true>("frames_paste_rgb32_sim_blend_kernel<table>", src, N, Hs, Ws, out, 0, 0, sim_dev, swap_rb, feather, lo, k, matte_dev,
                                  matte_frames, colour_dev, stream);
}

int spk_paste_colour_match_rgb32_sim_table(const float* src, int N, int Hs, int Ws, const spk_frame_ref* table_dev, const float* sim_dev,
                                           int swap_rb, int alpha_first, double feather, float lo, float k, const float* matte_dev,
                                           int matte_frames, double max_gain, double min_sigma, double min_weight, float* colour_out_dev,
                                           void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_match_rgb32_sim_table";
    if (int rc = check_paste_table(who, src, table_dev, sim_dev, N, Hs, Ws, alpha_first, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_match(who, N, max_gain, min_sigma, min_weight, colour_out_dev, workspace_dev, workspace_bytes)) return rc;
    if (int rc = check_table_apart(who, table_dev, N, colour_out_dev, (unsigned long long)N * 6ull * sizeof(float), "the colour rows")) return rc;
    if (int rc = check_table_apart(who, table_dev, N, workspace_dev, (unsigned long long)colour_match_workspace_bytes(N), "the workspace")) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<rgb32 table>", TableBackground32{table_dev, swap_rb, 8 * alpha_first}, src, N, Hs, Ws, 0,
                                    0, sim_dev, feather, lo, k, matte_dev, matte_frames, workspace_dev,
                                    ColourFinish{colour_out_dev, max_gain, min_sigma, min_weight, nullptr}, stream);
}

int spk_paste_colour_sums_rgb32_sim_table(const float* src, int N, int Hs, int Ws, const spk_frame_ref* table_dev, const float* sim_dev,
                                          int swap_rb, int alpha_first, double feather, float lo, float k, const float* matte_dev,
                                          int matte_frames, double* sums_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_sums_rgb32_sim_table";
    if (int rc = check_paste_table(who, src, table_dev, sim_dev, N, Hs, Ws, alpha_first, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_sums(who, N, sums_out_dev, workspace_dev, workspace_bytes)) return rc;
    if (int rc = check_table_apart(who, table_dev, N, sums_out_dev, (unsigned long long)N * SUMS * sizeof(double), "the sums")) return rc;
    if (int rc = check_table_apart(who, table_dev, N, workspace_dev, (unsigned long long)colour_match_workspace_bytes(N), "the workspace")) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<rgb32 table>", TableBackground32{table_dev, swap_rb, 8 * alpha_first}, src, N, Hs, Ws, 0,
                                    0, sim_dev, feather, lo, k, matte_dev, matte_frames, workspace_dev,
                                    ColourFinish{nullptr, 0.0, 0.0, 0.0, sums_out_dev}, stream);
}

}  // extern "C"
