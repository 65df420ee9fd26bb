// What a k-mer search call is planned from, as plain host code: no HIP, no context, no environment (knob values come
// in as arguments) -- the geometry of the count kernels, which path a launch range takes, how a call is cut into
// ranges, which posting lists are dense, the order that puts long queries last and the copies that bring a call's
// inputs into it and its rows back.  kmer.hip sizes its launches with it,
// kmer_launch.hip walks its ranges and moves its queries, kmer_index.hip takes the dense rule, host/store.cpp cuts its calls with
// big_select_range, and tests/kmer_plan_check.cpp runs all of it without a device.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sina_hip {

// ---- constants
// bases of the longest query the fast count kernel takes: SINA_HIP_MAX_QUERY_LEN of sina_hip.h (common.h asserts it; this
// header includes nothing of the project, so that a host tool or a test builds it with this directory alone)
constexpr uint32_t kKmerMaxQueryLen = 10240;
constexpr int kTileRefs = 32768;  // references per LDS tile of the count kernels: 64 KiB of int16 counters
constexpr int kLongQbExtra = 64;  // bytes of query masks the long count kernel keeps before a chunk's first window end
constexpr uint32_t kNoDense = 0xFFFFFFFFu;  // a k-mer's entry in the dense table: its posting list has no bitmap
// candidates per query the LDS select kernels sort; a larger top-M goes through the big select
constexpr uint32_t kKmerSelMax = 4096;
// the candidate-list path: keys a query's list holds, the largest top-M it serves, queries per launch range (32 KB of
// list each)
constexpr uint32_t kCandCap = 4096, kCandMaxM = 128, kCandRangeQueries = 16384;
// what the [queries][stride] int16 score matrix of a launch range may hold; a range holds at least one query
constexpr uint64_t kScoreMatrixBytes = 2ull << 30;
// What a query of the big select holds per candidate while its launch range is in flight: the 64-bit key and its
// double buffer for the segmented sort (16 bytes), the id and the score on the device (8) -- and 8 more in pinned
// staging, which the budget leaves out.
constexpr uint64_t kBigSelBytesPerCand = 24;
// ... and what a launch range may hold of it; a range holds at least one query whatever it needs
constexpr uint64_t kBigSelBudget = 1ull << 30;

// ---- paths.  What a launch range runs: the fast count kernel leaving candidate lists (kmer_select_cand_kernel
// sorts them) or score rows, or -- queries of more than SINA_HIP_MAX_QUERY_LEN bases -- the long count kernel, score
// rows only.  Rows go through the LDS select or, for more than kKmerSelMax candidates, the big select.
enum KmerPath : uint32_t { kKmerCand, kKmerRows, kKmerLong };
// The candidate path needs a top-M small enough for the list and two tiles of references or more (tile 0 alone must
// hold M of them); force_rows: SINA_HIP_TEST=kmer_rows=1.
inline bool kmer_cand_gate(uint32_t max, uint32_t n_refs, bool force_rows) {
    return max <= kCandMaxM && n_refs >= 2u * (uint32_t)kTileRefs && !force_rows;
}
inline bool kmer_big_select(uint32_t max) { return max > kKmerSelMax; }

// ---- geometry
// entries of a score row: 16-byte aligned rows for the select kernel's vector loads (64 bits: n_refs may be 2^32 - 1)
constexpr uint64_t kmer_row_stride(uint32_t n_refs) { return ((uint64_t)n_refs + 7u) & ~(uint64_t)7u; }
// k-mer list capacity of a workgroup: the range's longest query rounded to 64, or the long kernel's chunk capacity
constexpr uint32_t kmer_kmax(uint32_t max_qlen, KmerPath path) {
    return path == kKmerLong ? kKmerMaxQueryLen : (max_qlen + 63u) & ~63u;
}
// dynamic LDS of a count kernel: the tile's counters, two cursors and a mask byte per k-mer slot
constexpr size_t kmer_count_lds(uint32_t kmax, KmerPath path) {
    return (size_t)kTileRefs * 2 + (size_t)kmax * 9 + 64 + (path == kKmerLong ? (size_t)kLongQbExtra : 0);
}

// ---- dense posting lists (kmer_index.hip, ensure_dense): lists longer than 1 / div of the references (div = 64, or
// SINA_HIP_TEST=dense_div=N) and than 256 are kept as bitmaps of whole tiles
inline uint32_t kmer_dense_threshold(uint32_t n_refs, uint32_t div) { return n_refs / div > 256u ? n_refs / div : 256u; }
inline uint32_t kmer_dense_words(uint32_t n_refs) {
    return (uint32_t)(((uint64_t)n_refs + kTileRefs - 1) / kTileRefs) * (uint32_t)(kTileRefs / 32);
}

// ---- launch ranges
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
// Queries per launch range on score rows: what kScoreMatrixBytes holds of rows, and for the big select no more than
// its budget holds of candidates (max: clipped to n_refs by the caller)
inline uint32_t kmer_rows_range(uint32_t nq, uint32_t max, uint32_t n_refs, uint64_t big_budget) {
    const uint64_t row_bytes = 2 * kmer_row_stride(n_refs ? n_refs : 1u);
    uint32_t per = (uint32_t)(kScoreMatrixBytes / row_bytes ? kScoreMatrixBytes / row_bytes : 1u);
    if (kmer_big_select(max)) per = per < big_select_range(nq, max, big_budget) ? per : big_select_range(nq, max, big_budget);
    return per;
}
struct KmerRange {
    uint32_t q0, bq;  // queries q0 .. q0 + bq - 1 of the call
    KmerPath path;
    bool big;  // the range's select is the big select
};
inline void kmer_cut(std::vector<KmerRange> *out, uint64_t lo, uint64_t hi, uint32_t per, KmerPath path, bool big) {
    for (uint64_t q0 = lo; q0 < hi; q0 += per) out->push_back({(uint32_t)q0, (uint32_t)(hi - q0 < per ? hi - q0 : per), path, big});
}
// The ranges of a call in launch order: queries 0 .. n_fast - 1 (none longer than SINA_HIP_MAX_QUERY_LEN) on the fast
// count kernel, queries n_fast .. nq - 1 (every one of them longer) on the long kernel in ranges of their own.
inline std::vector<KmerRange> kmer_ranges(uint32_t nq, uint32_t n_fast, uint32_t max, uint32_t n_refs, uint64_t big_budget,
                                          bool force_rows) {
    std::vector<KmerRange> out;
    const bool cand = kmer_cand_gate(max, n_refs, force_rows), big = kmer_big_select(max);
    const uint32_t per = kmer_rows_range(nq, max, n_refs, big_budget);
    kmer_cut(&out, 0, n_fast, cand ? kCandRangeQueries : per, cand ? kKmerCand : kKmerRows, big && !cand);
    kmer_cut(&out, n_fast, nq, per, kKmerLong, big);
    return out;
}
// A candidate range one of whose lists overflowed (a giant group of equal scores) is repeated on score rows with the
// LDS select: its top-M is at most kCandMaxM
inline std::vector<KmerRange> kmer_overflow_ranges(const KmerRange &r, uint32_t n_refs) {
    std::vector<KmerRange> out;
    kmer_cut(&out, r.q0, (uint64_t)r.q0 + r.bq, kmer_rows_range(r.bq, kCandMaxM, n_refs, 0), kKmerRows, false);
    return out;
}

// ---- a batch with long queries: order[slot] = the caller's query, the queries of at most SINA_HIP_MAX_QUERY_LEN bases
// first, the longer ones behind them, each class in the caller's order; *n_fast: how many the first class has
inline std::vector<uint32_t> kmer_fast_first(const uint64_t *qoff, uint32_t nq, uint32_t *n_fast) {
    uint32_t nf = 0;
    for (uint32_t q = 0; q < nq; q++) nf += qoff[q + 1] - qoff[q] <= (uint64_t)kKmerMaxQueryLen;
    std::vector<uint32_t> order(nq);
    for (uint32_t q = 0, f = 0, l = nf; q < nq; q++) order[qoff[q + 1] - qoff[q] > (uint64_t)kKmerMaxQueryLen ? l++ : f++] = q;
    *n_fast = nf;
    return order;
}

// ---- ... and what moves with the queries, as data.  A ragged input: query q's elements of `elem` bytes are
// off[q] .. off[q + 1] of `base` (the mask bytes and the packed bases of a call share the queries' offsets, its self
// lists have their own).  An output column: `bytes` per query from `base` on (ids and scores: 4 per entry of a row, the
// count and the flag: 4, match counts: 2 per candidate, family rows: 4 per word).
struct KmerRagged {
    const void *base;
    const uint64_t *off;
    size_t elem;
};
struct KmerColumn {
    void *base;
    size_t bytes;
    template <class T>
    T *row(size_t q) const { return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + q * bytes); }
};
// the offsets of nq queries' elements once query order[x] stands in slot x, from 0 ...
inline std::vector<uint64_t> kmer_gather_offsets(const uint64_t *off, const uint32_t *order, uint32_t nq) {
    std::vector<uint64_t> out((size_t)nq + 1, 0);
    for (uint32_t x = 0; x < nq; x++) out[x + 1] = out[x] + (off[order[x] + 1] - off[order[x]]);
    return out;
}
// ... and the elements at those offsets, in storage of the call's own (one element more than there are: data() is an
// address whatever the queries hold)
inline std::vector<uint8_t> kmer_gather(const KmerRagged &in, const uint32_t *order, uint32_t nq, const uint64_t *new_off) {
    std::vector<uint8_t> out((new_off[nq] + 1) * in.elem);
    for (uint32_t x = 0; x < nq; x++)
        if (const uint64_t n = new_off[x + 1] - new_off[x])
            memcpy(out.data() + new_off[x] * in.elem, static_cast<const uint8_t *>(in.base) + in.off[order[x]] * in.elem, n * in.elem);
    return out;
}
// row x of `from` to row order[x] of `to`, a column of the same width (order null: row x to row x)
inline void kmer_scatter(const KmerColumn &from, const KmerColumn &to, const uint32_t *order, uint32_t nq) {
    if (from.bytes == 0 || nq == 0) return;
    if (!order) memcpy(to.base, from.base, (size_t)nq * from.bytes);
    else
        for (uint32_t x = 0; x < nq; x++) memcpy(to.row<uint8_t>(order[x]), from.row<uint8_t>(x), from.bytes);
}

}  // namespace sina_hip
