// What the table files share on the host (csrc/frame_table.hip: packed frames, entries of spk_frame_ref; csrc/frame_table_nv12.hip:
// NV12 surfaces, entries of spk_surface_ref; csrc/frame_table_i420.hip: I420 surfaces, entries of spk_planar_ref): how byte ranges
// are compared, how a byte count saturates, what an entry point checks of a table -- a device pointer and a count, whose entries are
// the kernels' to judge -- and, for surfaces of several planes, the extent of a plane and the rule that planes which are written
// share no byte.  Each file still links alone (the functions are inline).
#pragma once

#include <algorithm>
#include <vector>

#include "spk_common.hpp"

namespace spk::frame {

template <class Ref> struct TableName;
template <> struct TableName<spk_frame_ref> { static constexpr const char* value = "frame table"; };
template <> struct TableName<spk_surface_ref> { static constexpr const char* value = "surface table"; };
template <> struct TableName<spk_planar_ref> { static constexpr const char* value = "planar table"; };

inline bool ranges_overlap(const void* a, unsigned long long a_bytes, const void* b, unsigned long long b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 ? b0 - a0 < a_bytes : a0 - b0 < b_bytes;
}

// a table as an entry point sees it: a device pointer and a count (its entries are the kernels' to judge)
template <class Ref>
int check_table(const char* who, const Ref* table_dev, int N) {
    SPK_REQUIRE(table_dev, "%s: null %s", who, TableName<Ref>::value);
    SPK_REQUIRE((uintptr_t)table_dev % alignof(Ref) == 0, "%s: the %s must be aligned to %zu bytes", who, TableName<Ref>::value, alignof(Ref));
    SPK_REQUIRE(N >= 1, "%s: N must be >= 1 (got %d)", who, N);
    return SPK_OK;
}

// count * each bytes, saturated: a size that leaves 64 bits covers everything behind its first byte
inline unsigned long long bytes_of(unsigned long long count, unsigned long long each) {
    unsigned long long b;
    return __builtin_mul_overflow(count, each, &b) ? ~0ull : b;
}

template <class Ref>
int check_table_apart(const char* who, const Ref* table_dev, int N, const void* written, unsigned long long bytes, const char* name) {
    SPK_REQUIRE(!ranges_overlap(table_dev, (unsigned long long)N * sizeof(Ref), written, bytes), "%s: the %s overlaps %s", who,
                TableName<Ref>::value, name);
    return SPK_OK;
}

// the extent in bytes of a plane of `rows` rows of W bytes, (rows - 1) stride + W; false when it, or the address behind it, leaves 64 bits
inline bool plane_extent(const uint8_t* base, int rows, int64_t stride, int W, unsigned long long* extent) {
    long long lines, bytes;
    if (__builtin_mul_overflow((long long)(rows - 1), (long long)stride, &lines)) return false;
    if (__builtin_add_overflow(lines, (long long)W, &bytes)) return false;
    unsigned long long end;
    if (__builtin_add_overflow((unsigned long long)(uintptr_t)base, (unsigned long long)bytes, &end)) return false;
    *extent = (unsigned long long)bytes;
    return true;
}

// plane `plane` (an index into the format's names, in the order of an entry's fields) of entry `entry` as a byte range
struct PlaneRange { uintptr_t first; unsigned long long bytes; int entry; int plane; };

// planes that are written must not share a byte: in the order of their first bytes, each must begin where the ones before it ended.
// The pair a refusal names comes in the order (entry, plane).
inline int check_planes_apart(const char* who, std::vector<PlaneRange>& planes, const char* const* names) {
    std::sort(planes.begin(), planes.end(), [](const PlaneRange& a, const PlaneRange& b) {
        return a.first != b.first ? a.first < b.first : a.entry != b.entry ? a.entry < b.entry : a.plane < b.plane;
    });
    for (size_t i = 1, last = 0; i < planes.size(); ++i) {               // last: the plane before i that ends furthest
        const PlaneRange &a = planes[last], &b = planes[i];
        const bool a_first = a.entry < b.entry || (a.entry == b.entry && a.plane < b.plane);
        const PlaneRange &p = a_first ? a : b, &q = a_first ? b : a;
        SPK_REQUIRE(b.first >= a.first + a.bytes, "%s: entries %d (%s) and %d (%s) overlap: surfaces that are written must not share bytes", who,
                    p.entry, names[p.plane], q.entry, names[q.plane]);
        if (b.first + b.bytes > a.first + a.bytes) last = i;
    }
    return SPK_OK;
}

}  // namespace spk::frame
