// The aligned I420 edge over a PLANAR TABLE (include/spk.h has the definitions): every surface in three planes of its own, of its
// own pitches and size -- what a server with several calls holds when software decoders (or WebRTC's frame buffers) deliver each
// call's frames into that call's own buffers at its own resolution, and the encoders take them back from there.
//   frames_i420_to_f32_sim_table:          the way in of csrc/frame_sim_i420.hip;
//   frames_paste_i420_sim_table:           its paste (matte and colour rows may be NULL);
//   paste_colour_{sums,match}_i420_sim_table: its statistics.
// The kernels are the templates of csrc/frame_sim_common.hpp, csrc/frame_blend_common.hpp and csrc/frame_sim_nv12_common.hpp, the
// taps are I420Taps' (csrc/frame_i420_common.hpp): this file holds where a tabled surface's bytes are -- entry n of a device table
// of spk_planar_ref -- and nothing else.  The work decomposition of the three kernels does not depend on the size, so surface n of
// a table is bit for bit the strided launch at N = 1 on entry n.  The kernels read the table, the entry points never do: an entry
// is judged in the kernel, with the whole predicate, before an address is formed from it, and one that is not usable means the
// surface is absent -- it is treated exactly like an invalid row.  H and W of a usable entry are even, so a chroma block lies wholly
// inside its surface and the clamps of the shared geometry keep every load and store in bounds.  Chroma is bytes: no plane needs an
// alignment or an even pitch.  spk_planar_table_check is what a binder runs over its HOST copy before it uploads.
#include "frame_i420_common.hpp"
#include "frame_sim_nv12_common.hpp"
#include "frame_table_common.hpp"

static_assert(sizeof(spk_planar_ref) == 56 && alignof(spk_planar_ref) == 8, "spk_planar_ref is 3 x 8 + 3 x 8 + 4 + 4 bytes");

namespace {

using namespace spk::frame;

// Entry n as a kernel holds it: loaded once per frame (paste, statistics: n comes from blockIdx.y) or once per tile (way in: n is
// the wave's), outside the pixel loops.
struct TablePlanar {
    const uint8_t* y;
    const uint8_t* u;
    const uint8_t* v;
    long long y_row_stride, u_row_stride, v_row_stride;
    int H, W;
    __device__ __forceinline__ bool usable() const {
        return y != nullptr && u != nullptr && v != nullptr && H >= 2 && W >= 2 && !((H | W) & 1) && y_row_stride >= (long long)W &&
               u_row_stride >= (long long)(W >> 1) && v_row_stride >= (long long)(W >> 1);
    }
};

__device__ __forceinline__ TablePlanar load_planar(const spk_planar_ref* __restrict__ table, long long n) {
    const spk_planar_ref e = table[n];
    return {e.y, e.u, e.v, (long long)e.y_row_stride, (long long)e.u_row_stride, (long long)e.v_row_stride, e.H, e.W};
}

struct TablePlanarRead : I420Taps<TablePlanarRead> {            // the way in and the statistics
    const spk_planar_ref* table;
    Mat34 to_rgb;
    __device__ __forceinline__ TablePlanar frame(long long n, int, int) const { return load_planar(table, n); }
    __device__ __forceinline__ Row row(const TablePlanar& f, long long, int iy) const {
        return open_row(f.y, f.y_row_stride, f.u, f.u_row_stride, f.v, f.v_row_stride, iy);
    }
    __device__ __forceinline__ void load(const TablePlanar& f, long long, int X, int Y, double (&b)[3]) const {
        background(f.y, f.y_row_stride, f.u, f.u_row_stride, f.v, f.v_row_stride, X, Y, b);
    }
};

struct TablePlanarTarget {              // the paste: the surfaces of a table that is pasted into are the caller's to write
    const spk_planar_ref* table;
    __device__ __forceinline__ TablePlanar frame(long long n, int, int) const { return load_planar(table, n); }
    __device__ __forceinline__ static uint8_t* at(const uint8_t* p, long long row_stride, int X, int Y) {
        return const_cast<uint8_t*>(p) + (long long)Y * row_stride + X;
    }
    __device__ __forceinline__ uint8_t* luma(const TablePlanar& f, long long, int X, int Y) const { return at(f.y, f.y_row_stride, X, Y); }
    __device__ __forceinline__ void load_chroma(const TablePlanar& f, long long, int CX, int CY, unsigned& cu, unsigned& cv) const {
        PlanarPair::load(at(f.u, f.u_row_stride, CX, CY), at(f.v, f.v_row_stride, CX, CY), cu, cv);
    }
    __device__ __forceinline__ void store_chroma(const TablePlanar& f, long long, int CX, int CY, unsigned cu, unsigned cv) const {
        PlanarPair::store(at(f.u, f.u_row_stride, CX, CY), at(f.v, f.v_row_stride, CX, CY), cu, cv);
    }
};

// ---- host (ranges, byte counts, check_table, plane_extent and check_planes_apart: csrc/frame_table_common.hpp) ----
// what the tabled paste and its statistics check alike: check_paste of csrc/frame_sim_i420.hip without the surfaces' own arguments
int check_paste_table(const char* who, const void* src, const spk_planar_ref* table_dev, const float* sim_dev, int N, int Hs, int Ws, double feather,
                      float lo, float k, const float* matte_dev, int matte_frames) {
    SPK_REQUIRE(src, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    if (int rc = check_table(who, table_dev, N)) return rc;
    SPK_REQUIRE(Hs >= 1 && Ws >= 1, "%s: the source size must be >= 1 (got %d x %d)", who, Hs, Ws);
    return check_blend_params(who, N, feather, lo, k, matte_dev, matte_frames);
}

bool entry_usable(const spk_planar_ref& e) {
    return e.y != nullptr && e.u != nullptr && e.v != nullptr && e.H >= 2 && e.W >= 2 && e.H % 2 == 0 && e.W % 2 == 0 &&
           e.y_row_stride >= (int64_t)e.W && e.u_row_stride >= (int64_t)(e.W / 2) && e.v_row_stride >= (int64_t)(e.W / 2);
}

}  // namespace

extern "C" {

int spk_planar_table_check(const spk_planar_ref* host_table, int N, int written) {
    const char* who = "planar_table_check";
    SPK_REQUIRE(host_table, "%s: null planar table", who);
    SPK_REQUIRE(N >= 1, "%s: N must be >= 1 (got %d)", who, N);
    static const char* const names[3] = {"Y", "U", "V"};
    std::vector<PlaneRange> planes;
    for (int n = 0; n < N; ++n) {
        const spk_planar_ref& e = host_table[n];
        if (entry_usable(e)) {
            const uint8_t* const base[3] = {e.y, e.u, e.v};
            const int64_t stride[3] = {e.y_row_stride, e.u_row_stride, e.v_row_stride};
            for (int p = 0; p < 3; ++p) {
                const int rows = p ? e.H / 2 : e.H, width = p ? e.W / 2 : e.W;
                unsigned long long bytes;
                SPK_REQUIRE(plane_extent(base[p], rows, stride[p], width, &bytes), "%s: entry %d: the %s extent (rows - 1) * row stride + width of "
                            "%d rows of %d bytes with row stride %lld (a surface of %d x %d) overflows 64 bits", who, n, names[p], rows, width,
                            (long long)stride[p], e.H, e.W);
                planes.push_back({(uintptr_t)base[p], bytes, n, p});
            }
            continue;
        }
        SPK_REQUIRE(e.y == nullptr && e.u == nullptr && e.v == nullptr && e.y_row_stride == 0 && e.u_row_stride == 0 && e.v_row_stride == 0 &&
                    e.H == 0 && e.W == 0,
                    "%s: entry %d is half-formed: y %p, u %p, v %p, row strides %lld / %lld / %lld, %d x %d is neither usable (y, u, v, even H, "
                    "W >= 2, a Y row stride >= W, U and V row strides >= W / 2) nor all zero (an absent surface)", who, n, (const void*)e.y,
                    (const void*)e.u, (const void*)e.v, (long long)e.y_row_stride, (long long)e.u_row_stride, (long long)e.v_row_stride, e.H, e.W);
    }
    return written ? check_planes_apart(who, planes, names) : SPK_OK;
}

int spk_frames_i420_to_f32_sim_table(const spk_planar_ref* table_dev, int N, const float* sim_dev, int swap_rb, int standard, int full_range,
                                     float* dst, int Hout, int Wout, float scale0, float scale1, float scale2, float shift0, float shift1,
                                     float shift2, void* stream) {
    const char* who = "frames_i420_to_f32_sim_table";
    if (int rc = check_table(who, table_dev, N)) return rc;
    SPK_REQUIRE(dst, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(Hout >= 1 && Wout >= 1, "%s: the output size must be >= 1 (got %d x %d)", who, Hout, Wout);
    if (int rc = check_table_apart(who, table_dev, N, dst, bytes_of(bytes_of((unsigned long long)N * 12ull, (unsigned long long)Hout), (unsigned long long)Wout),
                                   "dst"))
        return rc;
    TablePlanarRead in = {{}, table_dev, {}};
    if (int rc = colour_maps(who, standard, full_range, in.to_rgb.m, nullptr)) return rc;
    return launch_frames_to_f32_sim("frames_i420_to_f32_sim_kernel<table>", in, N, 0, 0, sim_dev, swap_rb, dst, Hout, Wout,
                                    Affine3{{scale0, scale1, scale2}, {shift0, shift1, shift2}}, stream);
}

int spk_frames_paste_i420_sim_table(const float* src, int N, int Hs, int Ws, const spk_planar_ref* table_dev, const float* sim_dev, int standard,
                                    int full_range, double feather, float lo, float k, const float* matte_dev, int matte_frames,
                                    const float* colour_dev, void* stream) {
    const char* who = "frames_paste_i420_sim_table";
    if (int rc = check_paste_table(who, src, table_dev, sim_dev, N, Hs, Ws, feather, lo, k, matte_dev, matte_frames)) return rc;
    Mat34 M;
    if (int rc = colour_maps(who, standard, full_range, nullptr, M.m)) return rc;
    return launch_paste_nv12_sim("frames_paste_nv12_sim_kernel<i420 table>", src, N, Hs, Ws, TablePlanarTarget{table_dev}, 0, 0, sim_dev, feather, lo, k,
                                 matte_dev, matte_frames, colour_dev, M, stream);
}

int spk_paste_colour_match_i420_sim_table(const float* src, int N, int Hs, int Ws, const spk_planar_ref* table_dev, const float* sim_dev,
                                          int standard, int full_range, double feather, float lo, float k, const float* matte_dev,
                                          int matte_frames, double max_gain, double min_sigma, double min_weight, float* colour_out_dev,
                                          void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_match_i420_sim_table";
    if (int rc = check_paste_table(who, src, table_dev, sim_dev, N, Hs, Ws, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_match(who, N, max_gain, min_sigma, min_weight, colour_out_dev, workspace_dev, workspace_bytes)) return rc;
    if (int rc = check_table_apart(who, table_dev, N, colour_out_dev, (unsigned long long)N * 6ull * sizeof(float), "the colour rows")) return rc;
    if (int rc = check_table_apart(who, table_dev, N, workspace_dev, (unsigned long long)colour_match_workspace_bytes(N), "the workspace")) return rc;
    TablePlanarRead bg = {{}, table_dev, {}};
    if (int rc = colour_maps(who, standard, full_range, bg.to_rgb.m, nullptr)) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<i420 table>", bg, src, N, Hs, Ws, 0, 0, sim_dev, feather, lo, k, matte_dev, matte_frames,
                                    workspace_dev, ColourFinish{colour_out_dev, max_gain, min_sigma, min_weight, nullptr}, stream);
}

int spk_paste_colour_sums_i420_sim_table(const float* src, int N, int Hs, int Ws, const spk_planar_ref* table_dev, const float* sim_dev,
                                         int standard, int full_range, double feather, float lo, float k, const float* matte_dev,
                                         int matte_frames, double* sums_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_sums_i420_sim_table";
    if (int rc = check_paste_table(who, src, table_dev, sim_dev, N, Hs, Ws, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_sums(who, N, sums_out_dev, workspace_dev, workspace_bytes)) return rc;
    if (int rc = check_table_apart(who, table_dev, N, sums_out_dev, (unsigned long long)N * SUMS * sizeof(double), "the sums")) return rc;
    if (int rc = check_table_apart(who, table_dev, N, workspace_dev, (unsigned long long)colour_match_workspace_bytes(N), "the workspace")) return rc;
    TablePlanarRead bg = {{}, table_dev, {}};
    if (int rc = colour_maps(who, standard, full_range, bg.to_rgb.m, nullptr)) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<i420 table>", bg, src, N, Hs, Ws, 0, 0, sim_dev, feather, lo, k, matte_dev, matte_frames,
                                    workspace_dev, ColourFinish{nullptr, 0.0, 0.0, 0.0, sums_out_dev}, stream);
}

}  // extern "C"
