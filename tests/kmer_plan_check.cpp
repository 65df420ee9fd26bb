// csrc/kmer_plan.h -- the launch ranges of the k-mer search's big select -- against plain arithmetic, as a stand-alone
// program: tests/test_kmer_big_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it once.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

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

// walks the ranges as kmer.hip and host/store.cpp do; returns their number, checks that they tile [0, nq)
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

int main() {
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
