// Planning of a k-mer search call that orients its queries (turn.hip: turn_orient_kernel, turn_pick_kernel;
// kmer_launch.hip walks it), as plain host code: no HIP, no context, no environment -- which orientations a call
// tries and in which order, where the variants of a query lie among the call's virtual queries, how the virtual
// queries are cut into launch ranges of whole queries, the pick rule and the grids.  tests/turn_plan_check.cpp runs
// it without a device.
//
// Orientation o = (bit 0: reversed) | (bit 1: complemented).  A call tries n = 2 ("revcomp": 0, 3) or n = 4 ("all":
// 0, 3, 1, 2) orientations, in the order the host stage tried them (host/famfinder.cpp, best_orientations).  Query q's
// variants are the virtual queries q n .. q n + n - 1, each of the query's length: what the count and select kernels
// see is a call of nq n queries.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "kmer_plan.h"

namespace sina_hip {

constexpr uint32_t kTurnOrder[4] = {0, 3, 1, 2};
// ... and its inverse: the variant that holds orientation o (tried by a call of n variants if it is below n)
constexpr uint32_t kTurnVariantOf[4] = {0, 2, 3, 1};
inline uint32_t turn_variants(bool all) { return all ? 4u : 2u; }
// the orientation virtual query v of a call of n variants per query holds
inline uint32_t turn_orientation_of(uint32_t v, uint32_t n) { return kTurnOrder[v % n]; }
// the tried orientations, variant x in bits 2x, 2x + 1: what the kernels take
inline uint32_t turn_order_word(uint32_t n) {
    uint32_t w = 0;
    for (uint32_t x = 0; x < n; x++) w |= kTurnOrder[x] << (2 * x);
    return w;
}
// most queries a call takes: its virtual queries are counted in 32 bits
constexpr uint32_t kTurnMaxQueries = 0xFFFFFFFFu / 4u;

// base_iupac::complement on one mask byte: bits 1 <-> 8 and 2 <-> 4, the case bit (16) kept
constexpr uint8_t turn_complement(uint8_t d) {
    return (uint8_t)(((d & 2) << 1) | ((d & 4) >> 1) | ((d & 1) << 3) | ((d & 8) >> 3) | (d & 16));
}
// byte i of a query's variant in orientation o (src: the query's len mask bytes)
inline uint8_t turn_variant_byte(const uint8_t *src, uint64_t len, uint32_t o, uint64_t i) {
    const uint8_t d = src[(o & 1) ? len - 1 - i : i];
    return (o & 2) ? turn_complement(d) : d;
}

// The virtual queries' offsets, nq n + 1 of them from 0 (qoff: the queries', absolute): query q's variants lie behind
// each other from n (qoff[q] - qoff[0]) on.
inline std::vector<uint64_t> turn_offsets(const uint64_t *qoff, uint32_t nq, uint32_t n) {
    std::vector<uint64_t> out((size_t)nq * n + 1);
    for (uint32_t q = 0; q < nq; q++) {
        const uint64_t at = (uint64_t)n * (qoff[q] - qoff[0]), len = qoff[q + 1] - qoff[q];
        for (uint32_t x = 0; x < n; x++) out[(size_t)q * n + x] = at + x * len;
    }
    out[(size_t)nq * n] = (uint64_t)n * (qoff[nq] - qoff[0]);
    return out;
}

// The pick over the four orientations' top-1 scores (untried: 0): the first strictly largest above 0, else 0
// (src/famfinder.cpp:344-378).
inline uint32_t turn_pick(const float score[4]) {
    uint32_t best = 0;
    float top = 0;
    for (uint32_t o = 0; o < 4; o++)
        if (score[o] > top) {
            top = score[o];
            best = o;
        }
    return best;
}

// ---- launch ranges over the virtual queries: whole queries only, i.e. multiples of n; a range holds one query's
// variants at least, whatever they need, and stays within kmer_ranges' budgets otherwise
inline uint32_t turn_whole(uint32_t per, uint32_t n) { return per / n ? per / n * n : n; }
// nq, n_fast: the call's queries, the first n_fast of them not longer than SINA_HIP_MAX_QUERY_LEN; range_queries: 0,
// or the most queries a range may hold (SINA_HIP_TEST=turn_range=N); the rest as kmer_ranges takes it
inline std::vector<KmerRange> turn_ranges(uint32_t nq, uint32_t n_fast, uint32_t n, uint32_t max, uint32_t n_refs, uint64_t big_budget,
                                          bool force_rows, uint32_t range_queries = 0) {
    std::vector<KmerRange> out;
    const bool cand = kmer_cand_gate(max, n_refs, force_rows), big = kmer_big_select(max);
    uint32_t per = turn_whole(kmer_rows_range(nq * n, max, n_refs, big_budget), n);
    uint32_t per_cand = turn_whole(kCandRangeQueries, n);
    if (range_queries && (uint64_t)range_queries * n < per) per = range_queries * n;
    if (range_queries && (uint64_t)range_queries * n < per_cand) per_cand = range_queries * n;
    kmer_cut(&out, 0, (uint64_t)n_fast * n, cand ? per_cand : per, cand ? kKmerCand : kKmerRows, big && !cand);
    kmer_cut(&out, (uint64_t)n_fast * n, (uint64_t)nq * n, per, kKmerLong, big);
    return out;
}
// the sub-ranges a candidate range one of whose lists overflowed is repeated in (kmer_overflow_ranges): whole queries too
inline std::vector<KmerRange> turn_overflow_ranges(const KmerRange &r, uint32_t n, uint32_t n_refs) {
    std::vector<KmerRange> out;
    kmer_cut(&out, r.q0, (uint64_t)r.q0 + r.bq, turn_whole(kmer_rows_range(r.bq, kCandMaxM, n_refs, 0), n), kKmerRows, false);
    return out;
}

// ---- grids.  The orient kernel: one workgroup per query, its threads over the variants' dwords.  The pick kernel:
// one wave per query, kTurnPickQueriesPerWg waves to a workgroup.
constexpr uint32_t kTurnOrientThreads = 256;
inline uint32_t turn_orient_grid(uint32_t nq) { return nq; }
constexpr uint32_t kTurnWave = 64, kTurnPickQueriesPerWg = 4, kTurnPickThreads = kTurnWave * kTurnPickQueriesPerWg;
inline uint32_t turn_pick_grid(uint32_t bq) { return (bq + kTurnPickQueriesPerWg - 1) / kTurnPickQueriesPerWg; }
// bytes of the source copy the orient kernel reads as aligned dwords (one word of slack), and of the variants
inline size_t turn_source_bytes(uint64_t n_bases) { return (size_t)((n_bases + 3) / 4 * 4 + 4); }
inline size_t turn_variant_bytes(uint64_t n_bases, uint32_t n) { return (size_t)(n_bases * n + 4); }

}  // namespace sina_hip
