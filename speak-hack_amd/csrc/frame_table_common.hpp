// What the table files share on the host (csrc/frame_table.hip: packed frames, entries of spk_frame_ref; csrc/frame_table_nv12.hip:
// NV12 surfaces, entries of spk_surface_ref): how byte ranges are compared, how a byte count saturates, and what an entry point
// checks of a table -- a device pointer and a count, whose entries are the kernels' to judge.  Each file still links alone (the
// functions are inline).
#pragma once

#include "spk_common.hpp"

namespace spk::frame {

template <class Ref> struct TableName;
template <> struct TableName<spk_frame_ref> { static constexpr const char* value = "frame table"; };
template <> struct TableName<spk_surface_ref> { static constexpr const char* value = "surface table"; };

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

}  // namespace spk::frame
