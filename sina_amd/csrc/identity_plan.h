// Planning of the in-place family identity (identity.hip: two words per query of a DP launch range), as plain host
// code: no HIP, no context, no environment -- identity.hip sizes its launch with it, the launch driver decides with it
// whether a call counts, and tests/identity_plan_check.cpp runs it without a device.
#pragma once

#include <cstddef>
#include <cstdint>

namespace sina_hip {

// one workgroup of kIdentityThreads (= compare_dev.h's kCT) per query of the range
constexpr uint32_t kIdentityThreads = 256;
inline uint32_t identity_grid(uint32_t n_queries) { return n_queries; }

// LDS of a workgroup: the query tables of compare_dev.h (compare_table_bytes, asserted equal in identity.hip) for an
// alignment of `width` columns and the longest query of the range -- a bitmap word and a 16-bit running count per 32
// columns (and two counts of slack), a mask byte per base (rounded up to 16, 16 of slack).  The family routes take at
// most 524 288 columns and 10 240 bases: 108 579 bytes, above the 64 KB a kernel gets without asking.
constexpr size_t identity_lds_bytes(uint32_t width, uint32_t max_l) {
    const size_t nwords = ((size_t)width + 31) / 32;
    return 4 * nwords + 2 * (nwords + 2) + ((size_t)max_l + 15) + 16;
}
constexpr size_t kIdentityMaxLds = 150 * 1024;  // (compare_dev.h, kCompareMaxLds)

// Whether an align call counts: the context's switch is on, the call assembles, it brings families to the device (the
// align_families / _families_wsets / _profiles entries; align_graphs* bring none) and it has a query.
inline bool identity_call_counts(bool switch_on, bool assemble, bool has_families, uint32_t n_queries) {
    return switch_on && assemble && has_families && n_queries != 0;
}

// bytes of the rows of n_queries queries: the best score's float bits and the number of members that scored
inline size_t identity_row_bytes(uint32_t n_queries) { return 8 * (size_t)n_queries; }

}  // namespace sina_hip
