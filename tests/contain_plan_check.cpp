// csrc/contain_plan.h -- the grid, the key, the query packing, the staging sizes and the launch ranges of the
// containment kernel -- against plain arithmetic, as a stand-alone program: tests/test_contain_cpu.py builds it with
// the address and undefined-behaviour sanitizers and runs it once.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "contain_plan.h"

using namespace sina_hip;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            fails++;                                                  \
        }                                                             \
    } while (0)

// the ranges of n_pairs pairs: not empty, in order, without gaps, covering 0 .. n_pairs once, none larger than it may be
static std::vector<ContainRange> check_ranges(uint64_t n_pairs, uint64_t max_pairs) {
    const std::vector<ContainRange> r = contain_ranges(n_pairs, max_pairs);
    const uint64_t cap = max_pairs == 0 ? 1 : (max_pairs > kContainRangePairs ? kContainRangePairs : max_pairs);
    EXPECT(r.empty() == (n_pairs == 0));
    EXPECT(r.size() == (n_pairs + cap - 1) / cap);
    uint64_t at = 0;
    for (size_t k = 0; k < r.size(); k++) {
        EXPECT(r[k].p0 == at && r[k].p1 > r[k].p0 && r[k].p1 <= n_pairs);
        EXPECT(r[k].p1 - r[k].p0 <= cap);
        if (k + 1 < r.size()) EXPECT(r[k].p1 - r[k].p0 == cap);  // (only the last range is short)
        EXPECT(contain_grid((uint32_t)(r[k].p1 - r[k].p0)) <= 0x7FFFFFFFu);
        at = r[k].p1;
    }
    EXPECT(at == n_pairs);
    return r;
}

int main() {
    // ---- the answer and the limits
    EXPECT(kContainNone == 0xFFFFFFFFu && kContainMaxBases == 65535);
    // ---- the grid: one wave per pair, four to a workgroup of 256
    EXPECT(kContainWave == 64 && kContainPairsPerWg == 4 && kContainThreads == 256);
    EXPECT(contain_grid(0) == 0 && contain_grid(1) == 1 && contain_grid(4) == 1 && contain_grid(5) == 2 && contain_grid(41000) == 10250);
    EXPECT(contain_grid((uint32_t)kContainRangePairs) == kContainRangePairs / 4);
    for (uint32_t n = 0; n < 1000; n++) EXPECT((uint64_t)contain_grid(n) * kContainPairsPerWg >= n && (uint64_t)contain_grid(n) * kContainPairsPerWg < n + kContainPairsPerWg);
    // ---- the key: the first min(n, 8) codes
    EXPECT(kContainKeyBases == 8);
    EXPECT(contain_key_mask(1) == 0xFu && contain_key_mask(7) == 0x0FFFFFFFu && contain_key_mask(8) == 0xFFFFFFFFu &&
           contain_key_mask(9) == 0xFFFFFFFFu && contain_key_mask(65535) == 0xFFFFFFFFu);
    for (uint32_t n = 1; n < 8; n++) EXPECT(contain_key_mask(n) == (uint32_t)((1ull << (4 * n)) - 1));
    // ---- the packing: eight codes to a word, code j of a word in bits 4j .. 4j + 3, the case bit dropped, zeros behind
    EXPECT(contain_query_words(0) == 0 && contain_query_words(1) == 1 && contain_query_words(8) == 1 && contain_query_words(9) == 2 &&
           contain_query_words(65535) == 8192);
    for (uint64_t n : {1u, 7u, 8u, 9u, 63u, 64u, 65u, 129u, 1500u}) {
        std::vector<uint8_t> mask(n);  // (exactly n bytes: a read past them is the sanitizer's to find)
        for (uint64_t j = 0; j < n; j++) mask[j] = (uint8_t)(((j * 7 + 3) % 16) | ((j % 3) ? 0x10 : 0) | ((j % 5) ? 0 : 0xE0));
        std::vector<uint32_t> words(contain_query_words(n), 0xDEADBEEFu);
        contain_pack_query(mask.data(), n, words.data());
        for (uint64_t j = 0; j < 8 * words.size(); j++) {
            const uint32_t code = (words[j >> 3] >> (4 * (j & 7))) & 0xFu;
            EXPECT(code == (j < n ? (uint32_t)(mask[j] & 0xF) : 0u));
        }
    }
    // ---- staging: a word per pair each way
    EXPECT(contain_pair_bytes(0) == 0 && contain_pair_bytes(1) == 4 && contain_pair_bytes(kContainRangePairs) == 4 * kContainRangePairs);
    // ---- the worst case's bound
    EXPECT(contain_worst_steps(5, 4) == 0 && contain_worst_steps(1, 1) == 1 && contain_worst_steps(64, 64) == 1 &&
           contain_worst_steps(65, 65) == 2 && contain_worst_steps(750, 1500) == 751 * 12);
    for (uint64_t R : {1u, 64u, 1500u, 65535u})
        for (uint64_t n : {1u, 8u, 64u, 65u, 1499u}) EXPECT(contain_worst_steps(n, R) <= R * ((n + 63) / 64));
    // ---- launch ranges: 0, 1, the range size - 1, the size, the size + 1, a multiple -- at the default and at the knob's sizes
    for (uint64_t size : {(uint64_t)1, (uint64_t)3, (uint64_t)64, (uint64_t)1000, kContainRangePairs})
        for (uint64_t n : {(uint64_t)0, (uint64_t)1, size - 1, size, size + 1, 3 * size, 3 * size + 1}) check_ranges(n, size);
    EXPECT(check_ranges(7, 0).size() == 7);                                                   // 0 counts as 1
    EXPECT(check_ranges(2 * kContainRangePairs + 5, ~0ull).size() == 3);                      // never more than the default
    {
        const auto r = check_ranges(10, 4);
        EXPECT(r.size() == 3 && r[0].p1 == 4 && r[1].p1 == 8 && r[2].p1 == 10);
    }
    {
        uint64_t x = 88172645463325252ull;
        auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        for (int round = 0; round < 2000; round++) check_ranges(rnd() % 5000, rnd() % 70);
    }
    if (fails) return 1;
    printf("contain_plan_check: ok\n");
    return 0;
}
