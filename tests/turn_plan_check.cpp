// Checks the planning code of a search call that orients its queries (sina_amd/csrc/turn_plan.h) against plain
// arithmetic, without a device.  Built and run by tests/test_turn_cpu.py (address + undefined-behaviour sanitizers);
// exits non-zero with a message on the first difference.  All inputs are seeded.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "turn_plan.h"

using namespace sina_hip;

static const char *g_case = "";
[[noreturn]] static void fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "turn_plan_check: %s: ", g_case);
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(1);
}
#define CHECK(cond, ...) \
    do {                 \
        if (!(cond)) fail(__VA_ARGS__); \
    } while (0)

using Rng = std::mt19937_64;
static uint32_t between(Rng &r, uint32_t lo, uint32_t hi) { return lo + (uint32_t)(r() % (hi - lo + 1)); }

static void check_order() {
    g_case = "variant order";
    CHECK(turn_variants(false) == 2 && turn_variants(true) == 4, "variants per query");
    const uint32_t want[4] = {0, 3, 1, 2};
    for (uint32_t x = 0; x < 4; x++) {
        CHECK(kTurnOrder[x] == want[x], "variant %u holds orientation %u", x, kTurnOrder[x]);
        CHECK(kTurnVariantOf[kTurnOrder[x]] == x, "kTurnVariantOf is not the inverse at %u", x);
    }
    for (uint32_t n : {2u, 4u}) {
        const uint32_t w = turn_order_word(n);
        for (uint32_t v = 0; v < 40; v++) {
            CHECK(turn_orientation_of(v, n) == want[v % n], "orientation of virtual query %u", v);
            CHECK(((w >> (2 * (v % n))) & 3u) == want[v % n], "order word, variant %u", v % n);
        }
        CHECK(w >> (2 * n) == 0, "order word has bits beyond its variants");
    }
}

static void check_bytes() {
    g_case = "complement and variants";
    for (uint32_t d = 0; d < 32; d++) {
        const uint8_t c = turn_complement((uint8_t)d);
        CHECK(((c >> 3) & 1) == (d & 1) && (c & 1) == ((d >> 3) & 1) && ((c >> 2) & 1) == ((d >> 1) & 1) && ((c >> 1) & 1) == ((d >> 2) & 1),
              "complement of %u is %u", d, c);
        CHECK((c & 16) == (d & 16) && (c & 0xE0) == 0 && turn_complement(c) == d, "case bit / involution at %u", d);
    }
    Rng r(41);
    for (int it = 0; it < 200; it++) {
        const uint32_t len = between(r, 1, 70);
        std::vector<uint8_t> q(len);
        for (auto &b : q) b = (uint8_t)between(r, 1, 31);
        for (uint32_t o = 0; o < 4; o++)
            for (uint32_t i = 0; i < len; i++) {
                uint8_t want = q[(o & 1) ? len - 1 - i : i];
                if (o & 2) want = turn_complement(want);
                CHECK(turn_variant_byte(q.data(), len, o, i) == want, "variant byte, o %u, i %u", o, i);
            }
    }
}

static void check_offsets() {
    g_case = "offsets";
    Rng r(42);
    for (int it = 0; it < 300; it++) {
        const uint32_t nq = between(r, 1, 40), n = (it & 1) ? 4 : 2;
        std::vector<uint64_t> qoff(nq + 1);
        qoff[0] = between(r, 0, 1000);  // (absolute offsets: a sub-range of a larger array)
        for (uint32_t q = 0; q < nq; q++) qoff[q + 1] = qoff[q] + (between(r, 0, 9) ? between(r, 0, 300) : 0);
        const std::vector<uint64_t> v = turn_offsets(qoff.data(), nq, n);
        CHECK(v.size() == (size_t)nq * n + 1 && v[0] == 0, "size / first");
        CHECK(v.back() == n * (qoff[nq] - qoff[0]), "last offset %llu", (unsigned long long)v.back());
        for (uint32_t q = 0; q < nq; q++)
            for (uint32_t x = 0; x < n; x++) {
                const size_t i = (size_t)q * n + x;
                CHECK(v[i + 1] - v[i] == qoff[q + 1] - qoff[q], "variant %u of query %u has another length", x, q);
                CHECK(v[i] == n * (qoff[q] - qoff[0]) + x * (qoff[q + 1] - qoff[q]), "variant %u of query %u starts elsewhere", x, q);
            }
        CHECK(turn_source_bytes(qoff[nq] - qoff[0]) >= ((qoff[nq] - qoff[0] + 3) / 4) * 4 && turn_source_bytes(0) >= 4, "source bytes");
        CHECK(turn_variant_bytes(qoff[nq] - qoff[0], n) >= v.back(), "variant bytes");
    }
}

// every range a whole number of queries, none empty, the ranges cover lo .. hi once and in order
static void check_cover(const std::vector<KmerRange> &rs, uint64_t lo, uint64_t hi, uint32_t n, const char *what) {
    uint64_t at = lo;
    for (const KmerRange &g : rs) {
        CHECK(g.bq != 0, "%s: empty range", what);
        CHECK(g.q0 % n == 0 && g.bq % n == 0, "%s: range %u + %u is no whole number of queries of %u variants", what, g.q0, g.bq, n);
        CHECK(g.q0 == at, "%s: range starts at %u, not at %llu", what, g.q0, (unsigned long long)at);
        at += g.bq;
    }
    CHECK(at == hi, "%s: ranges end at %llu, not at %llu", what, (unsigned long long)at, (unsigned long long)hi);
}

static void check_ranges() {
    g_case = "ranges";
    Rng r(43);
    const uint32_t maxes[] = {1, 41, 128, 129, 4096, 4097, 100000};
    const uint32_t refs[] = {1, 300, 65535, 65536, 70000, 2000000, 0xFFFFFFFFu};
    const uint64_t budgets[] = {0, 1, 24ull * 4097, 24ull * 4097 * 5, 1ull << 20, kBigSelBudget};
    for (int it = 0; it < 4000; it++) {
        const uint32_t n = (it & 1) ? 4 : 2, nq = between(r, 1, (it % 7 == 0) ? 70000 : 50), n_fast = between(r, 0, nq);
        const uint32_t n_refs = refs[r() % 7], max = std::min(maxes[r() % 7], n_refs);
        const uint64_t budget = budgets[r() % 6];
        const bool force_rows = r() % 3 == 0;
        const uint32_t knob = (r() % 3 == 0) ? between(r, 1, 5) : 0;
        const std::vector<KmerRange> rs = turn_ranges(nq, n_fast, n, max, n_refs, budget, force_rows, knob);
        check_cover(rs, 0, (uint64_t)nq * n, n, "turn_ranges");
        const bool cand = kmer_cand_gate(max, n_refs, force_rows);
        const uint32_t rows_per = kmer_rows_range(nq * n, max, n_refs, budget);
        for (const KmerRange &g : rs) {
            const bool is_long = g.q0 >= (uint64_t)n_fast * n;
            CHECK(g.q0 + g.bq <= (uint64_t)n_fast * n || is_long, "a range holds fast and long queries");
            CHECK(g.path == (is_long ? kKmerLong : (cand ? kKmerCand : kKmerRows)), "path");
            CHECK(g.big == (kmer_big_select(max) && !(cand && !is_long)), "big");
            // within kmer_ranges' budgets, or one query's variants
            const uint32_t limit = (g.path == kKmerCand) ? kCandRangeQueries : rows_per;
            CHECK(g.bq <= limit || g.bq == n, "range of %u virtual queries over the budget of %u", g.bq, limit);
            if (knob) CHECK(g.bq <= knob * n, "range of %u over the knob's %u queries", g.bq, knob);
            if (g.path == kKmerCand) {
                const std::vector<KmerRange> sub = turn_overflow_ranges(g, n, n_refs);
                check_cover(sub, g.q0, (uint64_t)g.q0 + g.bq, n, "turn_overflow_ranges");
                const uint32_t sub_per = kmer_rows_range(g.bq, kCandMaxM, n_refs, 0);
                for (const KmerRange &h : sub) {
                    CHECK(h.path == kKmerRows && !h.big, "overflow sub-range path");
                    CHECK(h.bq <= sub_per || h.bq == n, "overflow sub-range of %u over %u", h.bq, sub_per);
                }
            }
        }
    }
    // the at-least-one-query rule: a budget smaller than one query's variants
    g_case = "at least one query";
    for (uint32_t n : {2u, 4u}) {
        const std::vector<KmerRange> rs = turn_ranges(7, 7, n, 4097, 5000, 24ull * 4097, false);  // (the budget holds ONE virtual query)
        CHECK(kmer_rows_range(7 * n, 4097, 5000, 24ull * 4097) == 1, "the budget was meant to hold one virtual query");
        CHECK(rs.size() == 7, "%zu ranges", rs.size());
        for (const KmerRange &g : rs) CHECK(g.bq == n && g.big && g.path == kKmerRows, "range of %u", g.bq);
        // a score row of 8 GiB: kScoreMatrixBytes holds none, a range still holds one query
        const std::vector<KmerRange> wide = turn_ranges(3, 3, n, 129, 0xFFFFFFFFu, kBigSelBudget, false);
        CHECK(wide.size() == 3 && wide[0].bq == n, "wide rows: %zu ranges of %u", wide.size(), wide[0].bq);
        const KmerRange g{0, 3 * n, kKmerCand, false};
        const std::vector<KmerRange> sub = turn_overflow_ranges(g, n, 0xFFFFFFFFu);
        CHECK(sub.size() == 3 && sub[2].q0 == 2 * n && sub[2].bq == n, "wide rows, overflow: %zu sub-ranges", sub.size());
    }
    // today's calls: kmer_ranges is what it was (n = 1 gives the same cut)
    g_case = "kmer_ranges untouched";
    for (int it = 0; it < 500; it++) {
        const uint32_t nq = between(r, 1, 40000), n_fast = between(r, 0, nq), n_refs = refs[r() % 7], max = std::min(maxes[r() % 7], n_refs);
        const std::vector<KmerRange> a = kmer_ranges(nq, n_fast, max, n_refs, kBigSelBudget, false), b = turn_ranges(nq, n_fast, 1, max, n_refs, kBigSelBudget, false);
        CHECK(a.size() == b.size(), "range counts differ");
        for (size_t i = 0; i < a.size(); i++) CHECK(a[i].q0 == b[i].q0 && a[i].bq == b[i].bq && a[i].path == b[i].path && a[i].big == b[i].big, "range %zu differs", i);
    }
}

static void check_pick_and_grids() {
    g_case = "pick";
    const float cases[][5] = {{0, 0, 0, 0, 0}, {5, 5, 5, 5, 0}, {1, 4, 4, 1, 1}, {0, 0, 0, 2, 3}, {3, 0, 0, 3, 0}, {1, 2, 3, 4, 3},
                              {0, 0, 7, 0, 2}, {2, 9, 1, 9, 1}, {-1, -1, -1, -1, 0}};
    for (const auto &c : cases) CHECK(turn_pick(c) == (uint32_t)c[4], "pick of %g %g %g %g", c[0], c[1], c[2], c[3]);
    g_case = "grids";
    CHECK(kTurnPickThreads == 256 && kTurnPickQueriesPerWg * kTurnWave == kTurnPickThreads && kTurnOrientThreads % kTurnWave == 0, "threads");
    for (uint32_t bq : {1u, 3u, 4u, 5u, 16384u, 0x3FFFFFFFu}) {
        CHECK(turn_orient_grid(bq) == bq, "orient grid");
        const uint32_t g = turn_pick_grid(bq);
        CHECK((uint64_t)g * kTurnPickQueriesPerWg >= bq && (uint64_t)(g - 1) * kTurnPickQueriesPerWg < bq, "pick grid of %u", bq);
    }
    CHECK(kTurnMaxQueries * 4ull <= 0xFFFFFFFFull, "virtual queries overflow 32 bits");
}

int main() {
    check_order();
    check_bytes();
    check_offsets();
    check_ranges();
    check_pick_and_grids();
    printf("turn_plan_check: ok\n");
    return 0;
}
