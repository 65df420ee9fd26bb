// Planning of the --show-dist kernel (showdist.hip: twenty words per query), as plain host code: no HIP, no context,
// no environment -- showdist.hip sizes and cuts its launches with it, the host stage reads its rows with it and
// tests/showdist_plan_check.cpp runs it without a device.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace sina_hip {

// A query's row, in 32-bit words: three sets of six counters in sina_hip_match_counts' order (only_a_overhang,
// only_b_overhang, only_a, only_b, match, mismatch), the closest relative's id and the flags.
constexpr uint32_t kShowDistSelf = 0;       // orig against aligned, SINA_CMP_IUPAC_EXACT
constexpr uint32_t kShowDistBefore = 6;     // orig against the closest relative, SINA_CMP_IUPAC_OPTIMISTIC
constexpr uint32_t kShowDistAfter = 12;     // aligned against the closest relative, SINA_CMP_IUPAC_OPTIMISTIC
constexpr uint32_t kShowDistClosest = 18;   // its reference id, kShowDistNone without one
constexpr uint32_t kShowDistFlags = 19;
constexpr uint32_t kShowDistRowWords = 20;
constexpr uint32_t kShowDistNone = 0xFFFFFFFFu;
constexpr uint32_t kShowDistFlagNan = 1u;       // a member of the list had a denominator of 0: it was left out
constexpr uint32_t kShowDistFlagComputed = 2u;  // the kernel wrote the row
inline size_t show_dist_row_bytes(uint32_t n_queries) { return 4 * (size_t)kShowDistRowWords * n_queries; }

// one workgroup of kShowDistThreads (= compare_dev.h's kCT) per query of the range
constexpr uint32_t kShowDistThreads = 256;
inline uint32_t show_dist_grid(uint32_t n_queries) { return n_queries; }

// LDS of a workgroup: the query tables of compare_dev.h (compare_table_bytes, asserted equal in showdist.hip) for an
// alignment of `width` columns, sized for the longer of the two sequences the workgroup tables one after the other.
constexpr size_t show_dist_lds_bytes(uint32_t width, uint32_t max_orig, uint32_t max_aligned) {
    const size_t nwords = ((size_t)width + 31) / 32;
    const size_t max_l = max_orig > max_aligned ? max_orig : max_aligned;
    return 4 * nwords + 2 * (nwords + 2) + (max_l + 15) + 16;
}
constexpr size_t kShowDistMaxLds = 150 * 1024;  // (compare_dev.h, kCompareMaxLds)
constexpr uint32_t kShowDistMaxBases = 65535;   // the tables' running counts are 16 bits wide

// A launch takes a range of consecutive queries: as many as keep the words uploaded for it -- both alignments and the
// list -- within kShowDistRangeWords (256 MiB of staging and device memory) and the workgroups within
// kShowDistRangeQueries, one query at least: a query larger than the limit opens a range of its own.
constexpr uint64_t kShowDistRangeWords = 1ull << 26;
constexpr uint32_t kShowDistRangeQueries = 1u << 22;

struct ShowDistRange {
    uint32_t q0, q1;  // queries [q0, q1) of the call
};

// orig_off, al_off, ref_off: [nq + 1], ascending (absolute offsets: only differences count).  The ranges are not empty,
// follow each other without a gap and cover 0 .. nq.  max_queries: SINA_HIP_TEST=showdist_range=N.
inline std::vector<ShowDistRange> show_dist_ranges(const uint64_t *orig_off, const uint64_t *al_off, const uint64_t *ref_off, uint32_t nq,
                                                   uint64_t max_words = kShowDistRangeWords,
                                                   uint32_t max_queries = kShowDistRangeQueries) {
    std::vector<ShowDistRange> out;
    if (max_queries == 0) max_queries = 1;
    uint32_t q0 = 0;
    while (q0 < nq) {
        uint32_t q1 = q0 + 1;
        while (q1 < nq && q1 - q0 < max_queries &&
               (orig_off[q1 + 1] - orig_off[q0]) + (al_off[q1 + 1] - al_off[q0]) + (ref_off[q1 + 1] - ref_off[q0]) <= max_words)
            q1++;
        out.push_back(ShowDistRange{q0, q1});
        q0 = q1;
    }
    return out;
}

}  // namespace sina_hip
