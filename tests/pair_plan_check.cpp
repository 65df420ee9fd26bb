// csrc/pair_plan.h -- the compaction of the helix map and the launch ranges of the pair-count kernel -- against plain
// arithmetic, as a stand-alone program: tests/test_bps_cpu.py builds it with the address and undefined-behaviour
// sanitizers and runs it once.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pair_plan.h"

using namespace sina_hip;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            fails++;                                                  \
        }                                                             \
    } while (0)

// the ranges of sequences of these lengths: not empty, without gaps, covering everything, none larger than it may be
static std::vector<PairRange> check_ranges(const std::vector<uint64_t> &len, uint64_t base, uint64_t max_words, uint32_t max_seqs) {
    std::vector<uint64_t> off(len.size() + 1, base);
    for (size_t i = 0; i < len.size(); i++) off[i + 1] = off[i] + len[i];
    const uint32_t nq = (uint32_t)len.size();
    const std::vector<PairRange> r = pair_ranges(off.data(), nq, max_words, max_seqs);
    EXPECT(r.empty() == (nq == 0));
    uint32_t at = 0;
    for (size_t k = 0; k < r.size(); k++) {
        EXPECT(r[k].q0 == at && r[k].q1 > r[k].q0 && r[k].q1 <= nq);
        const uint64_t words = off[r[k].q1] - off[r[k].q0];
        EXPECT(r[k].q1 - r[k].q0 <= (max_seqs ? max_seqs : 1));
        uint32_t with_words = 0;
        for (uint32_t q = r[k].q0; q < r[k].q1; q++) with_words += len[q] != 0 ? 1 : 0;
        EXPECT(words <= max_words || with_words == 1);  // (a sequence larger than a range: the only one in it with words)
        // greedy: the next sequence has words and would not have fitted
        if (r[k].q1 < nq && r[k].q1 - r[k].q0 < max_seqs) EXPECT(len[r[k].q1] != 0 && off[r[k].q1 + 1] - off[r[k].q0] > max_words);
        at = r[k].q1;
    }
    EXPECT(at == nq);
    return r;
}

int main() {
    // ---- compaction
    EXPECT(pair_compact(nullptr, 0).empty());  // an empty map
    {
        const std::vector<uint32_t> zero(1000, 0);
        EXPECT(pair_compact(zero.data(), (uint32_t)zero.size()).empty());  // an all-zero map
    }
    {
        std::vector<uint32_t> all(257);
        for (uint32_t i = 0; i < all.size(); i++) all[i] = 1000 - i;  // every column paired (column 0 too)
        const std::vector<uint32_t> e = pair_compact(all.data(), (uint32_t)all.size());
        EXPECT(e.size() == 2 * all.size());
        for (uint32_t i = 0; 2 * i + 1 < e.size(); i++) EXPECT(e[2 * i] == i && e[2 * i + 1] == 1000 - i);
    }
    {
        const uint32_t m[] = {0, 7, 0, 0, 0xFFFFFFFFu, 0, 1u << 24, 1, 0};
        const std::vector<uint32_t> e = pair_compact(m, 9);
        const uint32_t want[] = {1, 7, 4, 0xFFFFFFFFu, 6, 1u << 24, 7, 1};
        EXPECT(e.size() == 8);
        for (size_t i = 0; i < 8 && i < e.size(); i++) EXPECT(e[i] == want[i]);
        EXPECT(pair_compact(m, 1).empty() && pair_compact(m, 2).size() == 2);  // (only the first n entries are read)
    }
    // ---- launch ranges
    check_ranges({}, 0, 100, 10);
    check_ranges({0}, 5, 100, 10);
    check_ranges({0, 0, 0}, 0, 100, 2);
    {
        const auto r = check_ranges({10, 20, 30, 40, 50}, 17, 60, 100);  // (offsets that do not start at 0)
        EXPECT(r.size() == 3 && r[0].q1 == 3 && r[1].q1 == 4 && r[2].q1 == 5);
    }
    {
        const auto r = check_ranges({5, 500, 5, 5}, 0, 100, 100);  // one sequence larger than a range
        EXPECT(r.size() == 3 && r[0].q0 == 0 && r[0].q1 == 1 && r[1].q1 == 2 && r[2].q1 == 4);
    }
    {
        const auto r = check_ranges({0, 0, 60, 60, 0, 0}, 3, 100, 100);  // zero-length sequences at both ends
        EXPECT(r.size() == 2 && r[0].q1 == 3 && r[1].q0 == 3 && r[1].q1 == 6);
    }
    {
        const auto r = check_ranges({0, 700, 0}, 0, 100, 100);  // ... around a sequence larger than a range
        EXPECT(r.size() == 2 && r[0].q1 == 1 && r[1].q1 == 3);
    }
    {
        const auto r = check_ranges(std::vector<uint64_t>(10, 1), 0, 1000, 4);  // the sequence limit
        EXPECT(r.size() == 3 && r[2].q1 - r[2].q0 == 2);
    }
    check_ranges({1ull << 40, 1, 1ull << 40}, 1ull << 50, kPairRangeWords, kPairRangeSeqs);
    {
        uint64_t x = 88172645463325252ull;
        auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        for (int round = 0; round < 2000; round++) {
            std::vector<uint64_t> len(rnd() % 40);
            for (auto &l : len) l = rnd() % 3 ? rnd() % 50 : (rnd() % 5 ? 0 : rnd() % 400);
            check_ranges(len, rnd() % 1000, 1 + rnd() % 200, 1 + (uint32_t)(rnd() % 12));
        }
    }
    // ---- the grid: one wave per sequence, kPairWaves per workgroup
    EXPECT(pair_grid(0) == 0 && pair_grid(1) == 1 && pair_grid(kPairWaves) == 1 && pair_grid(kPairWaves + 1) == 2);
    EXPECT((uint64_t)pair_grid(kPairRangeSeqs) * kPairWaves >= kPairRangeSeqs && pair_grid(kPairRangeSeqs) <= 0x7FFFFFFFu);
    // ---- descending columns: equal neighbours pass; the check stays inside each sequence
    {
        const uint32_t ab[] = {5, 5 | (1u << 24), 9, 2, 3, 3, 1};
        const uint64_t off[] = {0, 3, 6, 7};
        EXPECT(pair_first_descending(ab, off, 3) == 3);  // (9 -> 2 and 3 -> 1 are sequence borders; the mask bits do not count)
        const uint64_t off2[] = {0, 4, 7};
        EXPECT(pair_first_descending(ab, off2, 2) == 0);
        const uint64_t off3[] = {1, 3, 7};
        EXPECT(pair_first_descending(ab, off3, 2) == 1);
        EXPECT(pair_first_descending(ab, off, 0) == 0);
    }
    if (fails) return 1;
    printf("pair_plan_check: ok\n");
    return 0;
}
