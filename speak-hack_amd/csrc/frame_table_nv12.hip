// The aligned NV12 edge over a SURFACE TABLE (include/spk.h has the definitions): every surface in planes of its own, of its own
// pitches and size -- what a server with several calls holds, each call's hardware decoder delivering into its own buffer at its
// own resolution, the encoder taking it back from there.
//   frames_nv12_to_f32_sim_table:          the way in of csrc/frame_sim_nv12.hip;
//   frames_paste_nv12_sim_table:           its paste (matte and colour rows may be NULL);
//   paste_colour_{sums,match}_nv12_sim_table: its statistics.
// The kernels are the templates of csrc/frame_sim_common.hpp, csrc/frame_blend_common.hpp and csrc/frame_sim_nv12_common.hpp, the
// taps and the colour arithmetic are Nv12Taps' (csrc/frame_nv12_common.hpp): this file holds where a tabled surface's bytes are --
// entry n of a device table of spk_surface_ref -- and nothing else.  The work decomposition of the three kernels does not depend on
// the size, so surface n of a table is bit for bit the strided launch at N = 1 on entry n.  The kernels read the table, the entry
// points never do: an entry is judged in the kernel, with the whole predicate, before an address is formed from it, and one that is
// not usable means the surface is absent -- it is treated exactly like an invalid row.  H and W of a usable entry are even, so a
// chroma block lies wholly inside its surface and the clamps of the shared geometry keep every load and store in bounds.
// spk_surface_table_check is what a binder runs over its HOST copy before it uploads.
#include "frame_sim_nv12_common.hpp"
#include "frame_table_common.hpp"

static_assert(sizeof(spk_surface_ref) == 40 && alignof(spk_surface_ref) == 8, "spk_surface_ref is 8 + 8 + 8 + 8 + 4 + 4 bytes");

namespace {

using namespace spk::frame;

// Entry n as a kernel holds it: loaded once per frame (paste, statistics: n comes from blockIdx.y) or once per tile (way in: n is
// the wave's), outside the pixel loops.
struct TableSurface {
    const uint8_t* y;
    const uint8_t* uv;
    long long y_row_stride, uv_row_stride;
    int H, W;
    __device__ __forceinline__ bool usable() const {
        return y != nullptr && uv != nullptr && H >= 2 && W >= 2 && !((H | W) & 1) && y_row_stride >= (long long)W &&
               uv_row_stride >= (long long)W && !(uv_row_stride & 1) && !((uintptr_t)uv & 1);
    }
};

__device__ __forceinline__ TableSurface load_surface(const spk_surface_ref* __restrict__ table, long long n) {
    const spk_surface_ref e = table[n];
    return {e.y, e.uv, (long long)e.y_row_stride, (long long)e.uv_row_stride, e.H, e.W};
}

struct TableSurfaceRead : Nv12Taps<TableSurfaceRead> {          // the way in and the statistics
    const spk_surface_ref* table;
    Mat34 to_rgb;
    __device__ __forceinline__ TableSurface frame(long long n, int, int) const { return load_surface(table, n); }
    __device__ __forceinline__ Row row(const TableSurface& f, long long, int iy) const {
        return open_row(f.y, f.y_row_stride, f.uv, f.uv_row_stride, iy);
    }
    __device__ __forceinline__ void load(const TableSurface& f, long long, int X, int Y, double (&b)[3]) const {
        background(f.y, f.y_row_stride, f.uv, f.uv_row_stride, X, Y, b);
    }
};

struct TableSurfaceTarget {             // the paste: the surfaces of a table that is pasted into are the caller's to write
    const spk_surface_ref* table;
    __device__ __forceinline__ TableSurface frame(long long n, int, int) const { return load_surface(table, n); }
    __device__ __forceinline__ uint8_t* luma(const TableSurface& f, long long, int X, int Y) const {
        return const_cast<uint8_t*>(f.y) + (long long)Y * f.y_row_stride + X;
    }
    __device__ __forceinline__ static uint8_t* chroma(const TableSurface& f, int CX, int CY) {
        return const_cast<uint8_t*>(f.uv) + (long long)CY * f.uv_row_stride + (long long)CX * 2;
    }
    __device__ __forceinline__ void load_chroma(const TableSurface& f, long long, int CX, int CY, unsigned& u, unsigned& v) const {
        Nv12Pair::load(chroma(f, CX, CY), u, v);
    }
    __device__ __forceinline__ void store_chroma(const TableSurface& f, long long, int CX, int CY, unsigned u, unsigned v) const {
        Nv12Pair::store(chroma(f, CX, CY), u, v);
    }
};

// ---- host ----
// what the tabled paste and its statistics check alike: check_paste of csrc/frame_sim_nv12.hip without the surfaces' own arguments
int check_paste_table(const char* who, const void* src, const spk_surface_ref* table_dev, const float* sim_dev, int N, int Hs, int Ws, double feather,
                      float lo, float k, const float* matte_dev, int matte_frames) {
    SPK_REQUIRE(src, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    if (int rc = check_table(who, table_dev, N)) return rc;
    SPK_REQUIRE(Hs >= 1 && Ws >= 1, "%s: the source size must be >= 1 (got %d x %d)", who, Hs, Ws);
    return check_blend_params(who, N, feather, lo, k, matte_dev, matte_frames);
}

bool entry_usable(const spk_surface_ref& e) {
    return e.y != nullptr && e.uv != nullptr && e.H >= 2 && e.W >= 2 && e.H % 2 == 0 && e.W % 2 == 0 && e.y_row_stride >= (int64_t)e.W &&
           e.uv_row_stride >= (int64_t)e.W && e.uv_row_stride % 2 == 0 && (uintptr_t)e.uv % 2 == 0;
}

}  // namespace

extern "C" {

int spk_surface_table_check(const spk_surface_ref* host_table, int N, int written) {
    const char* who = "surface_table_check";
    SPK_REQUIRE(host_table, "%s: null surface table", who);
    SPK_REQUIRE(N >= 1, "%s: N must be >= 1 (got %d)", who, N);
    std::vector<PlaneRange> planes;
    for (int n = 0; n < N; ++n) {
        const spk_surface_ref& e = host_table[n];
        if (entry_usable(e)) {
            unsigned long long y_bytes, uv_bytes;
            SPK_REQUIRE(plane_extent(e.y, e.H, e.y_row_stride, e.W, &y_bytes), "%s: entry %d: the Y extent (H - 1) * y_row_stride + W of %d x %d with "
                        "row stride %lld overflows 64 bits", who, n, e.H, e.W, (long long)e.y_row_stride);
            SPK_REQUIRE(plane_extent(e.uv, e.H / 2, e.uv_row_stride, e.W, &uv_bytes), "%s: entry %d: the UV extent (H / 2 - 1) * uv_row_stride + W of "
                        "%d x %d with row stride %lld overflows 64 bits", who, n, e.H, e.W, (long long)e.uv_row_stride);
            planes.push_back({(uintptr_t)e.y, y_bytes, n, 0});
            planes.push_back({(uintptr_t)e.uv, uv_bytes, n, 1});
            continue;
        }
        SPK_REQUIRE(e.y == nullptr && e.uv == nullptr && e.y_row_stride == 0 && e.uv_row_stride == 0 && e.H == 0 && e.W == 0,
                    "%s: entry %d is half-formed: y %p, uv %p, row strides %lld / %lld, %d x %d is neither usable (y, uv, even H, W >= 2, row strides "
                    ">= W, an even UV stride and a 2-byte aligned uv) nor all zero (an absent surface)", who, n, (const void*)e.y, (const void*)e.uv,
                    (long long)e.y_row_stride, (long long)e.uv_row_stride, e.H, e.W);
    }
    if (!written) return SPK_OK;
    static const char* const names[2] = {"Y", "UV"};
    return check_planes_apart(who, planes, names);                       // csrc/frame_table_common.hpp
}

int spk_frames_nv12_to_f32_sim_table(const spk_surface_ref* table_dev, int N, const float* sim_dev, int swap_rb, int standard, int full_range,
                                     float* dst, int Hout, int Wout, float scale0, float scale1, float scale2, float shift0, float shift1,
                                     float shift2, void* stream) {
    const char* who = "frames_nv12_to_f32_sim_table";
    if (int rc = check_table(who, table_dev, N)) return rc;
    SPK_REQUIRE(dst, "%s: null frame pointer", who);
    SPK_REQUIRE(sim_dev, "%s: null transform array", who);
    SPK_REQUIRE(Hout >= 1 && Wout >= 1, "%s: the output size must be >= 1 (got %d x %d)", who, Hout, Wout);
    if (int rc = check_table_apart(who, table_dev, N, dst, bytes_of(bytes_of((unsigned long long)N * 12ull, (unsigned long long)Hout), (unsigned long long)Wout),
                                   "dst"))
        return rc;
    TableSurfaceRead in = {{}, table_dev, {}};
    if (int rc = colour_maps(who, standard, full_range, in.to_rgb.m, nullptr)) return rc;
    return launch_frames_to_f32_sim("frames_nv12_to_f32_sim_kernel<table>", in, N, 0, 0, sim_dev, swap_rb, dst, Hout, Wout,
                                    Affine3{{scale0, scale1, scale2}, {shift0, shift1, shift2}}, stream);
}

int spk_frames_paste_nv12_sim_table(const float* src, int N, int Hs, int Ws, const spk_surface_ref* table_dev, const float* sim_dev, int standard,
                                    int full_range, double feather, float lo, float k, const float* matte_dev, int matte_frames,
                                    const float* colour_dev, void* stream) {
    const char* who = "frames_paste_nv12_sim_table";
    if (int rc = check_paste_table(who, src, table_dev, sim_dev, N, Hs, Ws, feather, lo, k, matte_dev, matte_frames)) return rc;
    Mat34 M;
    if (int rc = colour_maps(who, standard, full_range, nullptr, M.m)) return rc;
    return launch_paste_nv12_sim("frames_paste_nv12_sim_kernel<table>", src, N, Hs, Ws, TableSurfaceTarget{table_dev}, 0, 0, sim_dev, feather, lo, k,
                                 matte_dev, matte_frames, colour_dev, M, stream);
}

int spk_paste_colour_match_nv12_sim_table(const float* src, int N, int Hs, int Ws, const spk_surface_ref* table_dev, const float* sim_dev,
                                          int standard, int full_range, double feather, float lo, float k, const float* matte_dev,
                                          int matte_frames, double max_gain, double min_sigma, double min_weight, float* colour_out_dev,
                                          void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_match_nv12_sim_table";
    if (int rc = check_paste_table(who, src, table_dev, sim_dev, N, Hs, Ws, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_match(who, N, max_gain, min_sigma, min_weight, colour_out_dev, workspace_dev, workspace_bytes)) return rc;
    if (int rc = check_table_apart(who, table_dev, N, colour_out_dev, (unsigned long long)N * 6ull * sizeof(float), "the colour rows")) return rc;
    if (int rc = check_table_apart(who, table_dev, N, workspace_dev, (unsigned long long)colour_match_workspace_bytes(N), "the workspace")) return rc;
    TableSurfaceRead bg = {{}, table_dev, {}};
    if (int rc = colour_maps(who, standard, full_range, bg.to_rgb.m, nullptr)) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<nv12 table>", bg, src, N, Hs, Ws, 0, 0, sim_dev, feather, lo, k, matte_dev, matte_frames,
                                    workspace_dev, ColourFinish{colour_out_dev, max_gain, min_sigma, min_weight, nullptr}, stream);
}

int spk_paste_colour_sums_nv12_sim_table(const float* src, int N, int Hs, int Ws, const spk_surface_ref* table_dev, const float* sim_dev,
                                         int standard, int full_range, double feather, float lo, float k, const float* matte_dev,
                                         int matte_frames, double* sums_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "paste_colour_sums_nv12_sim_table";
    if (int rc = check_paste_table(who, src, table_dev, sim_dev, N, Hs, Ws, feather, lo, k, matte_dev, matte_frames)) return rc;
    if (int rc = check_colour_sums(who, N, sums_out_dev, workspace_dev, workspace_bytes)) return rc;
    if (int rc = check_table_apart(who, table_dev, N, sums_out_dev, (unsigned long long)N * SUMS * sizeof(double), "the sums")) return rc;
    if (int rc = check_table_apart(who, table_dev, N, workspace_dev, (unsigned long long)colour_match_workspace_bytes(N), "the workspace")) return rc;
    TableSurfaceRead bg = {{}, table_dev, {}};
    if (int rc = colour_maps(who, standard, full_range, bg.to_rgb.m, nullptr)) return rc;
    return launch_colour_statistics("paste_colour_sums_kernel<nv12 table>", bg, src, N, Hs, Ws, 0, 0, sim_dev, feather, lo, k, matte_dev, matte_frames,
                                    workspace_dev, ColourFinish{nullptr, 0.0, 0.0, 0.0, sums_out_dev}, stream);
}

}  // extern "C"
