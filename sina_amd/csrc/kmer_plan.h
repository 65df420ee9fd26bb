// Launch ranges of the k-mer search's big select (kmer.hip: more than kKmerSelMax candidates per query), as plain
// host code: no HIP, no context, no environment -- kmer.hip cuts its launches with it, host/store.cpp its calls, and
// tests/kmer_plan_check.cpp runs it without a device.
#pragma once

#include <cstdint>

namespace sina_hip {

// candidates per query the LDS select kernels sort; a larger top-M goes through the big select
constexpr uint32_t kKmerSelMax = 4096;
// What a query of the big select holds per candidate while its launch range is in flight: the 64-bit key and its
// double buffer for the segmented sort (16 bytes), the id and the score on the device (8) -- and 8 more in pinned
// staging, which the budget leaves out.
constexpr uint64_t kBigSelBytesPerCand = 24;
// ... and what a launch range may hold of it; a range holds at least one query whatever it needs
constexpr uint64_t kBigSelBudget = 1ull << 30;

// Queries per launch range of the big select: as many as fit `budget_bytes` with M candidates each, one at least and
// no more than nq.  (64-bit throughout: nq = M = 2^20 is 24 TiB of candidates.)
inline uint32_t big_select_range(uint32_t nq, uint32_t M, uint64_t budget_bytes) {
    const uint64_t per_query = kBigSelBytesPerCand * (uint64_t)(M ? M : 1u);
    uint64_t fit = budget_bytes / per_query;
    if (fit < 1) fit = 1;
    if (fit > nq) fit = nq;
    return fit ? (uint32_t)fit : 1u;
}
// ... and how many ranges nq queries take
inline uint32_t big_select_ranges(uint32_t nq, uint32_t M, uint64_t budget_bytes) {
    if (nq == 0) return 0;
    const uint32_t per = big_select_range(nq, M, budget_bytes);
    return (uint32_t)(((uint64_t)nq + per - 1) / per);
}

}  // namespace sina_hip
