// csrc/showdist_plan.h -- the row layout, the LDS size, the grid and the launch ranges of the show-dist kernel --
// against plain arithmetic, as a stand-alone program: tests/test_showdist_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it once.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "showdist_plan.h"

using namespace sina_hip;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            fails++;                                                  \
        }                                                             \
    } while (0)

struct Lens {
    uint64_t orig, aligned, list;
};

// the ranges of queries of these sizes: not empty, without gaps, covering everything, none larger than it may be
static std::vector<ShowDistRange> check_ranges(const std::vector<Lens> &len, uint64_t base, uint64_t max_words, uint32_t max_queries) {
    const uint32_t nq = (uint32_t)len.size();
    std::vector<uint64_t> o(nq + 1, base), a(nq + 1, 3 * base + 1), l(nq + 1, base / 2);
    for (uint32_t i = 0; i < nq; i++) {
        o[i + 1] = o[i] + len[i].orig;
        a[i + 1] = a[i] + len[i].aligned;
        l[i + 1] = l[i] + len[i].list;
    }
    const std::vector<ShowDistRange> r = show_dist_ranges(o.data(), a.data(), l.data(), nq, max_words, max_queries);
    EXPECT(r.empty() == (nq == 0));
    auto words = [&](uint32_t q0, uint32_t q1) { return (o[q1] - o[q0]) + (a[q1] - a[q0]) + (l[q1] - l[q0]); };
    uint32_t at = 0;
    for (size_t k = 0; k < r.size(); k++) {
        EXPECT(r[k].q0 == at && r[k].q1 > r[k].q0 && r[k].q1 <= nq);
        EXPECT(r[k].q1 - r[k].q0 <= (max_queries ? max_queries : 1));
        EXPECT(words(r[k].q0, r[k].q1) <= max_words || r[k].q1 - r[k].q0 == 1);  // (a query larger than a range: alone in it)
        // greedy: the next query would not have fitted
        if (r[k].q1 < nq && r[k].q1 - r[k].q0 < (max_queries ? max_queries : 1)) EXPECT(words(r[k].q0, r[k].q1 + 1) > max_words);
        at = r[k].q1;
    }
    EXPECT(at == nq);
    return r;
}

int main() {
    // ---- the row: three sets of six counters, the closest relative, the flags
    EXPECT(kShowDistSelf == 0 && kShowDistBefore == 6 && kShowDistAfter == 12 && kShowDistClosest == 18 && kShowDistFlags == 19);
    EXPECT(kShowDistRowWords == 20 && show_dist_row_bytes(0) == 0 && show_dist_row_bytes(1) == 80);
    EXPECT(show_dist_row_bytes(kShowDistRangeQueries) == 80ull * kShowDistRangeQueries);
    EXPECT(kShowDistNone == 0xFFFFFFFFu && kShowDistFlagNan == 1 && kShowDistFlagComputed == 2);
    // ---- the LDS: a bitmap word and a 16-bit count per 32 columns (two counts of slack), a mask byte per base of the
    // longer sequence (rounded up to 16, 16 of slack)
    for (uint32_t width : {1u, 31u, 32u, 33u, 64u, 8224u, 50000u, 524288u})
        for (uint32_t lo : {0u, 1u, 17u, 1500u, 65535u})
            for (uint32_t la : {0u, 5u, 1500u, 65535u}) {
                const size_t nwords = (width + 31) / 32, longer = lo > la ? lo : la;
                EXPECT(show_dist_lds_bytes(width, lo, la) == 6 * nwords + 4 + longer + 31);
                EXPECT(show_dist_lds_bytes(width, lo, la) == show_dist_lds_bytes(width, la, lo));
            }
    EXPECT(show_dist_lds_bytes(50000, 1500, 1500) <= 64 * 1024);                 // 16S: within what a kernel gets unasked
    EXPECT(show_dist_lds_bytes(524288, 10240, 10240) == 108579 && show_dist_lds_bytes(524288, 10240, 10240) <= kShowDistMaxLds);
    EXPECT(show_dist_lds_bytes(900000, 10, 10) > kShowDistMaxLds);               // refused as a limit
    EXPECT(kShowDistMaxBases == 65535 && kShowDistMaxLds == 150 * 1024);
    // ---- the grid: one workgroup per query
    EXPECT(show_dist_grid(0) == 0 && show_dist_grid(1) == 1 && show_dist_grid(600) == 600 && kShowDistThreads == 256);
    EXPECT(show_dist_grid(kShowDistRangeQueries) <= 0x7FFFFFFFu);
    // ---- launch ranges
    check_ranges({}, 0, 100, 10);
    check_ranges({{0, 0, 0}}, 5, 100, 10);
    {
        const auto r = check_ranges({{10, 10, 5}, {10, 10, 5}, {10, 10, 5}, {10, 10, 5}, {10, 10, 5}}, 17, 60, 100);
        EXPECT(r.size() == 3 && r[0].q1 == 2 && r[1].q1 == 4 && r[2].q1 == 5);
    }
    {
        const auto r = check_ranges({{5, 5, 1}, {500, 400, 40}, {5, 5, 1}, {5, 5, 1}}, 0, 100, 100);  // one query larger than a range
        EXPECT(r.size() == 3 && r[0].q1 == 1 && r[1].q1 == 2 && r[2].q1 == 4);
    }
    {
        const auto r = check_ranges(std::vector<Lens>(10, Lens{1, 1, 1}), 0, 1000, 4);  // the query limit (showdist_range=4)
        EXPECT(r.size() == 3 && r[2].q1 - r[2].q0 == 2);
    }
    {
        const auto r = check_ranges(std::vector<Lens>(5, Lens{3, 3, 2}), 9, kShowDistRangeWords, 1);  // showdist_range=1
        EXPECT(r.size() == 5);
    }
    {
        const auto r = check_ranges(std::vector<Lens>(3, Lens{3, 3, 2}), 9, kShowDistRangeWords, 0);  // 0 counts as 1
        EXPECT(r.size() == 3);
    }
    {
        const auto r = check_ranges({{0, 0, 90}, {0, 0, 90}}, 0, 100, 100);  // the list alone fills a range
        EXPECT(r.size() == 2);
    }
    check_ranges({{1ull << 40, 1, 1}, {1, 1, 1}, {1, 1ull << 40, 0}}, 1ull << 50, kShowDistRangeWords, kShowDistRangeQueries);
    {
        uint64_t x = 88172645463325252ull;
        auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        for (int round = 0; round < 2000; round++) {
            std::vector<Lens> len(rnd() % 40);
            for (auto &l : len) l = Lens{rnd() % 50, rnd() % 3 ? rnd() % 50 : 0, rnd() % 5 ? rnd() % 42 : 0};
            check_ranges(len, rnd() % 1000, 1 + rnd() % 300, (uint32_t)(rnd() % 12));
        }
    }
    if (fails) return 1;
    printf("showdist_plan_check: ok\n");
    return 0;
}
