// Checks sina_amd/csrc/family_plan.h (the family cascade's row width, bound and grid) against plain arithmetic and a
// plain cascade, without a device.  Built and run by tests/test_cascade_cpu.py as a stand-alone program under the
// address sanitizer; exits non-zero with a message on the first difference.  All inputs are seeded.
//   family_plan_check                           the checks
//   family_plan_check min max full cover nq     prints "ok K row_words grid" of family_plan, for the Python mirror
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "family_plan.h"

using namespace sina_hip;

#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            fprintf(stderr, "family_plan_check: ");      \
            fprintf(stderr, __VA_ARGS__);                \
            fprintf(stderr, "\n");                       \
            exit(1);                                     \
        }                                                \
    } while (0)

struct Cand {
    bool eligible, full, left, right, good;
};

int main(int argc, char **argv) {
    if (argc == 6) {
        const FamilyPlan p = family_plan((uint32_t)strtoul(argv[1], nullptr, 10), (uint32_t)strtoul(argv[2], nullptr, 10),
                                         (uint32_t)strtoul(argv[3], nullptr, 10), (uint32_t)strtoul(argv[4], nullptr, 10),
                                         (uint32_t)strtoul(argv[5], nullptr, 10));
        printf("%d %u %u %u\n", p.ok ? 1 : 0, p.K, p.row_words, p.grid);
        return 0;
    }
    // the defaults: 41 entries, 84 words
    CHECK(family_bound(40, 40, 1, 0) == 41 && family_row_words(41) == 84, "the defaults' row");
    // the cap, on either side, and options that overflow 32 bits
    CHECK(family_plan(kFamilyCascadeMaxK, 0, 0, 0, 1).ok && family_plan(kFamilyCascadeMaxK - 3, 5, 1, 1, 1).ok, "a rule at the cap");
    CHECK(!family_plan(kFamilyCascadeMaxK, 0, 1, 0, 1).ok && !family_plan(0, kFamilyCascadeMaxK - 1, 0, 1, 1).ok, "a rule over the cap");
    CHECK(!family_plan(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 1).ok && family_bound(0xFFFFFFFFu, 1, 0xFFFFFFFFu, 0xFFFFFFFFu) == 4ull * 0xFFFFFFFFull,
          "options that overflow 32 bits");
    CHECK(family_plan(0, 0, 0, 0, 0).ok && family_plan(0, 0, 0, 0, 0).row_words == 2 && family_plan(0, 0, 0, 0, 0).grid == 0, "the empty rule");
    // the grid: one wave per query
    for (uint32_t nq : {1u, 3u, 4u, 5u, 1000u, 0xFFFFFFFFu}) {
        const FamilyPlan p = family_plan(40, 40, 1, 0, nq);
        CHECK(p.ok && (uint64_t)p.grid * kFamilyWavesPerWg >= nq && ((uint64_t)p.grid - 1) * kFamilyWavesPerWg < nq, "grid of %u queries", nq);
    }
    // the bound holds and a row of K entries suffices: a plain cascade over random lists, kept ids written into a row
    // of exactly 2 + 2 K words (the sanitizer watches the row's end)
    std::mt19937_64 rng(20241);
    for (int round = 0; round < 20000; round++) {
        const uint32_t fs_min = (uint32_t)(rng() % 9), fs_max = (uint32_t)(rng() % 9), req_full = (uint32_t)(rng() % 3), cover = (uint32_t)(rng() % 3);
        const FamilyPlan p = family_plan(fs_min, fs_max, req_full, cover, 1);
        CHECK(p.ok, "a small rule");
        std::vector<uint32_t> row(p.row_words, 0u);
        const size_t n = rng() % 200;
        uint32_t have = 0, have_full = 0, have_left = 0, have_right = 0;
        bool saturated_before = false;
        for (size_t i = 0; i < n; i++) {
            const uint64_t bits = rng();
            const Cand c{(bits & 3) != 0, (bits & 12) == 0, (bits & 48) == 0, (bits & 64) != 0, (bits & 128) != 0};
            const bool saturated = have >= (fs_min > fs_max ? fs_min : fs_max) && have_full >= req_full && have_left >= cover && have_right >= cover;
            CHECK(!saturated_before || saturated, "saturation is final");
            saturated_before = saturated;
            if (!c.eligible) continue;
            const bool min_reached = have >= fs_min, max_reached = have >= fs_max;
            const bool adds_to_full = req_full && have_full < req_full && c.full;
            const bool adds_to_range = (cover && have_right < cover && c.right) || (cover && have_left < cover && c.left);
            if (min_reached && (max_reached || !c.good) && !adds_to_full && !adds_to_range) continue;
            CHECK(!saturated, "a candidate kept behind the saturation point");
            CHECK(have < p.K, "a family of more than K = %u entries", p.K);
            row[2 + have] = (uint32_t)i;
            row[2 + p.K + have] = (uint32_t)bits;
            ++have;
            if (req_full && c.full) ++have_full;
            if (cover && c.right) ++have_right;
            if (cover && c.left) ++have_left;
        }
        row[0] = have;
    }
    printf("family_plan_check: ok\n");
    return 0;
}
