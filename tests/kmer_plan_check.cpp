// csrc/kmer_plan.h -- what a k-mer search call is planned from: the launch ranges of the big select, the paths and
// ranges of a call, the count kernels' geometry, the dense rule, the fast-first order, the gather and scatter that move
// a call's queries and rows by it -- against plain arithmetic and plain per-query loops, as a stand-alone program:
// tests/test_kmer_big_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it once.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/sina_hip.h"  // (beside this file's directory: the limits the plan must agree with)
#include "kmer_plan.h"

using namespace sina_hip;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            fails++;                                                  \
        }                                                             \
    } while (0)

// walks the big select's ranges as host/store.cpp does; returns their number, checks that they tile [0, nq)
static uint64_t walk(uint32_t nq, uint32_t M, uint64_t budget, uint32_t *first, uint32_t *last) {
    const uint32_t per = big_select_range(nq, M, budget);
    EXPECT(per >= 1 && per <= (nq ? nq : 1u));
    uint64_t n = 0;
    *first = *last = 0;
    for (uint64_t q0 = 0; q0 < nq; q0 += per) {
        const uint32_t bq = (uint32_t)(nq - q0 < per ? nq - q0 : per);
        if (n == 0) *first = bq;
        *last = bq;
        // a range of more than one query is within the budget
        EXPECT(bq == 1 || (uint64_t)bq * M * kBigSelBytesPerCand <= budget);
        n++;
    }
    EXPECT(n == big_select_ranges(nq, M, budget));
    return n;
}

// ---- the rest of the plan, against arithmetic written out here (none of it calls the plan to learn what to expect)
static uint64_t own_stride(uint32_t n_refs) { return ((uint64_t)n_refs + 7) / 8 * 8; }
static const uint64_t kTwoGiB = 1ull << 31;
static uint64_t own_rows_per(uint32_t n_refs) {
    const uint64_t per = kTwoGiB / (2 * own_stride(n_refs ? n_refs : 1));
    return per ? per : 1;
}
// queries per range of the score-row paths
static uint64_t own_per(uint32_t nq, uint32_t max, uint32_t n_refs, uint64_t budget) {
    uint64_t per = own_rows_per(n_refs);
    if (max > 4096) {
        uint64_t fit = budget / (24ull * max);
        if (fit > nq) fit = nq;
        if (fit < 1) fit = 1;
        if (fit < per) per = fit;
    }
    return per;
}
static bool own_cand(uint32_t max, uint32_t n_refs, bool force_rows) { return max <= 128 && n_refs >= 65536 && !force_rows; }

// a score-row range is within 2 GiB of rows, and within the budget if its select is the big one -- or holds one query
static void check_rows_range(const KmerRange &r, uint32_t max, uint32_t n_refs, uint64_t budget) {
    EXPECT(r.bq == 1 || (uint64_t)r.bq * own_stride(n_refs) * 2 <= kTwoGiB);
    EXPECT(r.big == (max > 4096));
    if (r.big) EXPECT(r.bq == 1 || (uint64_t)r.bq * max * 24 <= budget);
}
static size_t check_ranges(uint32_t nq, uint32_t n_fast, uint32_t max, uint32_t n_refs, uint64_t budget, bool force_rows) {
    const std::vector<KmerRange> rs = kmer_ranges(nq, n_fast, max, n_refs, budget, force_rows);
    const bool cand = own_cand(max, n_refs, force_rows);
    uint64_t at = 0;
    for (const KmerRange &r : rs) {
        EXPECT(r.q0 == at && r.bq >= 1);  // in order, no gap, no overlap
        at += r.bq;
        EXPECT(at <= n_fast || r.q0 >= n_fast);  // none straddles n_fast
        if (r.q0 >= n_fast) {
            EXPECT(r.path == kKmerLong);
            check_rows_range(r, max, n_refs, budget);
        } else if (cand) {
            EXPECT(r.path == kKmerCand && !r.big && r.bq <= 16384);
            // its repeat tiles exactly the range, on score rows with the LDS select
            uint64_t rat = r.q0;
            for (const KmerRange &h : kmer_overflow_ranges(r, n_refs)) {
                EXPECT(h.q0 == rat && h.bq >= 1 && h.path == kKmerRows && !h.big);
                EXPECT(h.bq == 1 || (uint64_t)h.bq * own_stride(n_refs) * 2 <= kTwoGiB);
                rat += h.bq;
            }
            EXPECT(rat == (uint64_t)r.q0 + r.bq);
        } else {
            EXPECT(r.path == kKmerRows);
            check_rows_range(r, max, n_refs, budget);
        }
        EXPECT(!(r.path == kKmerCand && r.big));  // the candidate path and the big select never coincide
    }
    EXPECT(at == nq);
    return rs.size();
}
// one case of (max, n_refs, budget, force_rows) at nq in {0, 1, per, per + 1}, the batch all fast, all long and split
static void check_case(uint32_t max, uint32_t n_refs, uint64_t budget, bool force_rows) {
    const uint64_t per = own_cand(max, n_refs, force_rows) ? 16384 : own_per(0xFFFFFFFFu, max, n_refs, budget);
    const uint64_t nqs[4] = {0, 1, per, per + 1};
    for (uint64_t nq64 : nqs) {
        const uint32_t nq = (uint32_t)nq64;
        const uint32_t fasts[4] = {nq, 0, nq / 2, nq ? nq - 1 : 0};
        for (uint32_t n_fast : fasts) check_ranges(nq, n_fast, max, n_refs, budget, force_rows);
    }
}
static void check_plan() {
    static_assert(kKmerMaxQueryLen == SINA_HIP_MAX_QUERY_LEN, "the plan's own statement of the fast kernel's limit");
    // ---- gate edges
    EXPECT(kmer_cand_gate(128, 65536, false) && !kmer_cand_gate(129, 65536, false));
    EXPECT(!kmer_cand_gate(128, 65535, false) && kmer_cand_gate(1, 0xFFFFFFFFu, false));
    EXPECT(!kmer_cand_gate(128, 65536, true) && !kmer_cand_gate(1, 500000, true));
    EXPECT(!kmer_big_select(4096) && kmer_big_select(4097) && !kmer_big_select(1) && kmer_big_select(0xFFFFFFFFu));
    static_assert(kCandCap == 4096 && kCandMaxM == 128 && kCandRangeQueries == 16384, "the candidate lists");
    static_assert(kScoreMatrixBytes == (1ull << 31) && kTileRefs == 32768 && kNoDense == 0xFFFFFFFFu, "constants");
    // ---- ranges: every gate edge, with budgets that cut and budgets that do not
    const uint32_t maxes[] = {1, 128, 129, 4096, 4097, 5000, 100000};
    const uint32_t refs[] = {1, 7, 8, 9, 65535, 65536, 65537, 500000, 0x7FFFFFFFu, 0xFFFFFFFFu};
    const uint64_t budgets[] = {0, 1000, 24ull * 5000 * 4, kBigSelBudget};
    for (uint32_t max : maxes)
        for (uint32_t n_refs : refs)
            for (uint64_t budget : budgets)
                for (int force = 0; force < 2; force++)
                    if (max <= n_refs) check_case(max, n_refs, budget, force != 0);  // (the driver clips max to n_refs)
    // the paths at the edges, as ranges
    EXPECT(kmer_ranges(10, 10, 128, 65536, kBigSelBudget, false)[0].path == kKmerCand);
    EXPECT(kmer_ranges(10, 10, 129, 65536, kBigSelBudget, false)[0].path == kKmerRows);
    EXPECT(kmer_ranges(10, 10, 128, 65535, kBigSelBudget, false)[0].path == kKmerRows);
    EXPECT(kmer_ranges(10, 10, 128, 65536, kBigSelBudget, true)[0].path == kKmerRows);
    EXPECT(!kmer_ranges(10, 10, 4096, 65536, kBigSelBudget, false)[0].big && kmer_ranges(10, 10, 4097, 65536, kBigSelBudget, false)[0].big);
    EXPECT(kmer_ranges(10, 4, 4097, 65536, kBigSelBudget, false).back().big && kmer_ranges(10, 4, 4097, 65536, kBigSelBudget, false).back().path == kKmerLong);
    // a batch with both classes on the candidate path: fast ranges of 16384, long ranges of 2^30 / 65536
    {
        const std::vector<KmerRange> rs = kmer_ranges(16384 + 5 + 16384 + 1, 16384 + 5, 10, 65536, kBigSelBudget, false);
        EXPECT(rs.size() == 4 && rs[0].bq == 16384 && rs[1].bq == 5 && rs[1].path == kKmerCand);
        EXPECT(rs[2].q0 == 16389 && rs[2].bq == 16384 && rs[2].path == kKmerLong && rs[3].bq == 1);
    }
    // ---- known values: 500 000 references, 9216 queries on score rows -- 2^30 / 500 000 = 2147 queries per range, five ranges
    EXPECT(check_ranges(9216, 9216, 10, 500000, kBigSelBudget, true) == 5);
    EXPECT(kmer_ranges(9216, 9216, 10, 500000, kBigSelBudget, true)[0].bq == 2147 && kmer_ranges(9216, 9216, 10, 500000, kBigSelBudget, true)[4].bq == 9216 - 4 * 2147);
    EXPECT(check_ranges(9216, 9216, 10, 500000, kBigSelBudget, false) == 1);  // (candidate lists: one)
    // the smallest and the largest store.  One reference: a row is 8 entries, 2^27 rows are 2 GiB -- any real batch is
    // one range.  2^32 - 1 references: a row alone is 8 GiB, one query per range, and no 32-bit product on the way
    EXPECT(check_ranges(1000, 1000, 1, 1, kBigSelBudget, false) == 1);
    EXPECT(check_ranges((1u << 27) + 1, (1u << 27) + 1, 1, 1, kBigSelBudget, false) == 2);
    EXPECT(check_ranges(3, 3, 200, 0xFFFFFFFFu, kBigSelBudget, false) == 3);
    EXPECT(check_ranges(3, 2, 10, 0xFFFFFFFFu, kBigSelBudget, true) == 3);
    {
        const std::vector<KmerRange> rs = kmer_ranges(3, 3, 10, 0xFFFFFFFFu, kBigSelBudget, false);  // candidate lists: one range ...
        EXPECT(rs.size() == 1 && rs[0].path == kKmerCand && kmer_overflow_ranges(rs[0], 0xFFFFFFFFu).size() == 3);  // ... repeated query by query
    }
    // ---- geometry
    for (uint32_t n_refs : {0u, 1u, 7u, 8u, 9u, 65537u, 500000u, 0xFFFFFFF8u, 0xFFFFFFF9u, 0xFFFFFFFFu}) {
        const uint64_t s = kmer_row_stride(n_refs);
        EXPECT(s % 8 == 0 && s >= n_refs && s < (uint64_t)n_refs + 8);
    }
    EXPECT(kmer_row_stride(0xFFFFFFFFu) == (1ull << 32) && kmer_row_stride(500000) == 500000 && kmer_row_stride(65537) == 65544);
    EXPECT(kmer_kmax(1, kKmerRows) == 64 && kmer_kmax(64, kKmerCand) == 64 && kmer_kmax(65, kKmerRows) == 128);
    EXPECT(kmer_kmax(SINA_HIP_MAX_QUERY_LEN - 1, kKmerCand) == SINA_HIP_MAX_QUERY_LEN && kmer_kmax(SINA_HIP_MAX_QUERY_LEN, kKmerRows) == SINA_HIP_MAX_QUERY_LEN);
    EXPECT(kmer_kmax(1, kKmerLong) == SINA_HIP_MAX_QUERY_LEN && kmer_kmax(32767, kKmerLong) == SINA_HIP_MAX_QUERY_LEN);
    const size_t kmax = SINA_HIP_MAX_QUERY_LEN;
    EXPECT(kmer_count_lds(SINA_HIP_MAX_QUERY_LEN, kKmerRows) == 32768 * 2 + kmax * 9 + 64 && kmer_count_lds(SINA_HIP_MAX_QUERY_LEN, kKmerRows) <= 160 * 1024);
    EXPECT(kmer_count_lds(SINA_HIP_MAX_QUERY_LEN, kKmerCand) == kmer_count_lds(SINA_HIP_MAX_QUERY_LEN, kKmerRows));
    EXPECT(kmer_count_lds(SINA_HIP_MAX_QUERY_LEN, kKmerLong) == 32768 * 2 + kmax * 9 + 64 + 64 && kmer_count_lds(SINA_HIP_MAX_QUERY_LEN, kKmerLong) <= 160 * 1024);
    EXPECT(kmer_count_lds(64, kKmerRows) == 65536 + 576 + 64);
    // ---- dense lists
    EXPECT(kmer_dense_threshold(0, 64) == 256 && kmer_dense_threshold(255 * 64, 64) == 256 && kmer_dense_threshold(256 * 64 + 64, 64) == 257);
    EXPECT(kmer_dense_threshold(256 * 64 + 63, 64) == 256 && kmer_dense_threshold(100000, 64) == 1562 && kmer_dense_threshold(500000, 64) == 7812);
    EXPECT(kmer_dense_threshold(1000, 1) == 1000 && kmer_dense_threshold(100, 1) == 256 && kmer_dense_threshold(0xFFFFFFFFu, 1) == 0xFFFFFFFFu);
    EXPECT(kmer_dense_words(1) == 1024 && kmer_dense_words(32768) == 1024 && kmer_dense_words(32769) == 2048 && kmer_dense_words(0) == 0);
    EXPECT(kmer_dense_words(0xFFFFFFFFu) == 131072u * 1024u);
    // ---- the fast-first order
    const uint32_t S = 100, L = SINA_HIP_MAX_QUERY_LEN + 1;  // a short and a long query
    const std::vector<std::vector<uint32_t>> batches = {{S, S, SINA_HIP_MAX_QUERY_LEN, 0, S}, {L, L + 5, 32767}, {S, L, S, L, S, L, S}, {L, S, L, S}, {}};
    for (const std::vector<uint32_t> &lens : batches) {
        const uint32_t nq = (uint32_t)lens.size();
        std::vector<uint64_t> qoff(nq + 1, 17);  // (offsets need not start at 0)
        for (uint32_t q = 0; q < nq; q++) qoff[q + 1] = qoff[q] + lens[q];
        uint32_t n_fast = 12345, want_fast = 0;
        const std::vector<uint32_t> order = kmer_fast_first(qoff.data(), nq, &n_fast);
        for (uint32_t q = 0; q < nq; q++) want_fast += lens[q] <= SINA_HIP_MAX_QUERY_LEN;
        EXPECT(order.size() == nq && n_fast == want_fast);
        for (uint32_t x = 0; x < nq; x++) {
            EXPECT(order[x] < nq && (lens[order[x]] <= SINA_HIP_MAX_QUERY_LEN) == (x < n_fast));  // the classes, in their places
            if (x && x != n_fast) EXPECT(order[x - 1] < order[x]);                                   // stable within each
        }
        // gather by the order, scatter back: the caller's rows
        std::vector<uint32_t> gathered(nq), back(nq, 0xdeadu);
        for (uint32_t x = 0; x < nq; x++) gathered[x] = 1000 + order[x];
        for (uint32_t x = 0; x < nq; x++) back[order[x]] = gathered[x];
        for (uint32_t q = 0; q < nq; q++) EXPECT(back[q] == 1000 + q);
    }
    {
        const uint64_t qoff[5] = {0, L, L + S, 2 * L + S, 2 * L + 2 * S};  // long, short, long, short
        uint32_t n_fast = 0;
        const std::vector<uint32_t> order = kmer_fast_first(qoff, 4, &n_fast);
        EXPECT(n_fast == 2 && order[0] == 1 && order[1] == 3 && order[2] == 0 && order[3] == 2);
    }
}

// ---- the copies that bring a call's inputs into the fast-first order and its rows back, against plain per-query loops
static std::vector<uint64_t> offsets_of(const std::vector<uint32_t> &lens, uint64_t first) {
    std::vector<uint64_t> off(lens.size() + 1, first);
    for (size_t q = 0; q < lens.size(); q++) off[q + 1] = off[q] + lens[q];
    return off;
}
// a ragged input of `elem`-byte elements at `off`, every byte its own function of its place; gathered, byte by byte
static void check_gather(const std::vector<uint64_t> &off, size_t elem, const std::vector<uint32_t> &order) {
    const uint32_t nq = (uint32_t)order.size();
    std::vector<uint8_t> src((off[nq] + 3) * elem);  // (elements before the first offset and behind the last one)
    for (size_t i = 0; i < src.size(); i++) src[i] = (uint8_t)(i * 131 + i / 251 + elem);
    const std::vector<uint64_t> new_off = kmer_gather_offsets(off.data(), order.data(), nq);
    EXPECT(new_off.size() == (size_t)nq + 1 && new_off[0] == 0);
    const std::vector<uint8_t> got = kmer_gather(KmerRagged{src.data(), off.data(), elem}, order.data(), nq, new_off.data());
    EXPECT(got.size() == (new_off[nq] + 1) * elem && got.data() != nullptr);
    uint64_t at = 0, bad = 0;
    for (uint32_t x = 0; x < nq; x++) {
        EXPECT(new_off[x] == at);
        for (uint64_t i = off[order[x]]; i < off[order[x] + 1]; i++, at++)
            for (size_t b = 0; b < elem; b++) bad += got[at * elem + b] != src[i * elem + b];
    }
    EXPECT(new_off[nq] == at && at == off[nq] - off[0] && bad == 0);
}
// a column of `bytes` per query scattered into the caller's rows, a guard row behind them
static void check_scatter(size_t bytes, const std::vector<uint32_t> &order, bool identity) {
    const uint32_t nq = (uint32_t)order.size();
    std::vector<uint8_t> from((size_t)nq * bytes + 1), to(((size_t)nq + 1) * bytes + 1, 0xEE);
    for (size_t i = 0; i < from.size(); i++) from[i] = (uint8_t)(i * 37 + i / 253 + 1);
    kmer_scatter(KmerColumn{from.data(), bytes}, KmerColumn{to.data(), bytes}, identity ? nullptr : order.data(), nq);
    uint64_t bad = 0;
    for (uint32_t x = 0; x < nq; x++)
        for (size_t b = 0; b < bytes; b++) bad += to[(size_t)(identity ? x : order[x]) * bytes + b] != from[(size_t)x * bytes + b];
    for (size_t i = (size_t)nq * bytes; i < to.size(); i++) bad += to[i] != 0xEE;  // the guard row
    EXPECT(bad == 0);
}
static void check_moves() {
    const uint32_t S = 100, L = SINA_HIP_MAX_QUERY_LEN + 1;
    struct Batch {
        std::vector<uint32_t> lens, self_lens;
        uint64_t first, self_first;
    };
    const std::vector<Batch> batches = {
        {{S, 7, SINA_HIP_MAX_QUERY_LEN, S}, {2, 0, 0, 5}, 0, 0},                        // no long query
        {{L, L + 5, 32767}, {1, 1, 1}, 0, 3},                                           // only long queries
        {{S, L, 50, L + 9, 30}, {0, 3, 0, 0, 4}, 0, 0},                                 // long and short interleaved
        {{S, L, 50, L + 9, 30}, {0, 0, 0, 0, 0}, 17, 5},                                // a sub-range of larger arrays; no self list at all
        {{S, 0, L, 0, 1}, {3, 0, 2, 1, 0}, 4099, 11},                                   // queries of length 0                                
        {{0}, {0}, 9, 9},                                                               // one empty query
        {{}, {}, 5, 5},                                                                 // no query
    };
    for (const Batch &b : batches) {
        const uint32_t nq = (uint32_t)b.lens.size();
        const std::vector<uint64_t> qoff = offsets_of(b.lens, b.first), self_off = offsets_of(b.self_lens, b.self_first);
        uint32_t n_fast = 0;
        const std::vector<uint32_t> order = kmer_fast_first(qoff.data(), nq, &n_fast);
        check_gather(qoff, 1, order);      // mask bytes ...
        check_gather(qoff, 4, order);      // ... and packed bases, on the queries' offsets
        check_gather(self_off, 4, order);  // the self lists on their own
        // ids and scores of rows of 1, 10, 41 and 4097 entries, n and flag, match counts of 1 and 41 candidates, family
        // rows of 2 + 2 * 41 words; a column without bytes (max == 0)
        for (size_t bytes : {(size_t)1 * 4, (size_t)10 * 4, (size_t)41 * 4, (size_t)4097 * 4, (size_t)4, (size_t)1 * 2, (size_t)41 * 2, (size_t)84 * 4, (size_t)0})
            for (int identity = 0; identity < 2; identity++) check_scatter(bytes, order, identity != 0);
    }
    {
        // known values: long, short, long, short with 2, 1, 0, 3 self ids
        const uint64_t qoff[5] = {10, 10 + L, 10 + L + S, 10 + 2 * L + S, 10 + 2 * L + 2 * S}, self_off[5] = {4, 6, 7, 7, 10};
        const uint32_t self_ids[10] = {90, 91, 92, 93, 40, 41, 50, 60, 61, 62};
        uint32_t n_fast = 0;
        const std::vector<uint32_t> order = kmer_fast_first(qoff, 4, &n_fast);
        const std::vector<uint64_t> q_new = kmer_gather_offsets(qoff, order.data(), 4), s_new = kmer_gather_offsets(self_off, order.data(), 4);
        EXPECT(q_new[1] == S && q_new[2] == 2 * S && q_new[3] == 2 * S + L && q_new[4] == 2 * S + 2 * L);
        EXPECT(s_new[1] == 1 && s_new[2] == 4 && s_new[3] == 6 && s_new[4] == 6);
        const std::vector<uint8_t> got = kmer_gather(KmerRagged{self_ids, self_off, 4}, order.data(), 4, s_new.data());
        const uint32_t want[6] = {50, 60, 61, 62, 40, 41};
        EXPECT(got.size() == 7 * 4 && memcmp(got.data(), want, sizeof(want)) == 0);
        uint32_t rows[4] = {1000, 1001, 1002, 1003}, back[5] = {7, 7, 7, 7, 7};
        kmer_scatter(KmerColumn{rows, 4}, KmerColumn{back, 4}, order.data(), 4);
        EXPECT(back[0] == 1002 && back[1] == 1000 && back[2] == 1003 && back[3] == 1001 && back[4] == 7);
        EXPECT((KmerColumn{back, 8}.row<uint32_t>(2) == back + 4));
    }
}

int main() {
    check_plan();
    check_moves();
    static_assert(kBigSelBudget <= (1ull << 30), "the budget is at most 1 GiB");
    static_assert(kKmerSelMax == 4096, "the LDS select kernels' limit");
    uint32_t first, last;
    // a budget below one query: one query per range
    EXPECT(big_select_range(7, 5000, 1000) == 1);
    EXPECT(walk(7, 5000, 1000, &first, &last) == 7 && first == 1 && last == 1);
    EXPECT(big_select_range(7, 5000, 0) == 1);
    EXPECT(big_select_range(7, 5000, kBigSelBytesPerCand * 5000 - 1) == 1);
    EXPECT(big_select_range(7, 5000, kBigSelBytesPerCand * 5000) == 1);
    // an exact multiple: 12 queries, 4 per range
    EXPECT(big_select_range(12, 5000, 4 * kBigSelBytesPerCand * 5000) == 4);
    EXPECT(walk(12, 5000, 4 * kBigSelBytesPerCand * 5000, &first, &last) == 3 && first == 4 && last == 4);
    // a remainder: 14 queries, 4 per range, 2 left
    EXPECT(walk(14, 5000, 4 * kBigSelBytesPerCand * 5000 + 17, &first, &last) == 4 && first == 4 && last == 2);
    // a budget for more than there are: one range
    EXPECT(big_select_range(5, 4097, kBigSelBudget) == 5);
    EXPECT(walk(5, 4097, kBigSelBudget, &first, &last) == 1 && first == 5);
    // no queries
    EXPECT(big_select_ranges(0, 5000, kBigSelBudget) == 0);
    EXPECT(big_select_range(0, 5000, kBigSelBudget) == 1);
    // nq = M = 2^20: 24 MiB per query, 42 queries per GiB, no overflow on the way
    const uint32_t big = 1u << 20;
    EXPECT(big_select_range(big, big, kBigSelBudget) == 42);
    EXPECT(big_select_ranges(big, big, kBigSelBudget) == (big + 41) / 42);
    EXPECT(big_select_range(big, big, 1) == 1 && big_select_ranges(big, big, 1) == big);
    // the largest arguments there are
    EXPECT(big_select_range(0xFFFFFFFFu, 0xFFFFFFFFu, kBigSelBudget) == 1);
    EXPECT(big_select_ranges(0xFFFFFFFFu, 0xFFFFFFFFu, kBigSelBudget) == 0xFFFFFFFFu);
    EXPECT(big_select_range(0xFFFFFFFFu, 1, ~0ull) == 0xFFFFFFFFu);
    // what DESIGN.md 3.4 quotes: queries per range at 4100, 41 000 and 100 000 candidates
    EXPECT(big_select_range(100000, 4100, kBigSelBudget) == 10912);
    EXPECT(big_select_range(100000, 41000, kBigSelBudget) == 1091);
    EXPECT(big_select_range(100000, 100000, kBigSelBudget) == 447);
    if (fails) return 1;
    printf("kmer_plan_check: ok\n");
    return 0;
}
