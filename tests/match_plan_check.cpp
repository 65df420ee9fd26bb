// csrc/match_plan.h -- the grid of the match-count kernel -- against plain arithmetic, as a stand-alone program:
// tests/test_msc_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it once.  With three
// arguments (nq M n_cu) it prints that plan instead, for the test's Python mirror.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "match_plan.h"

using namespace sina_hip;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            fails++;                                                  \
        }                                                             \
    } while (0)

// the properties of one plan; `cover`: also walk the chunks of a query as the kernel does and count every candidate
static void check(uint32_t nq, uint32_t M, uint32_t n_cu, bool cover) {
    const MatchPlan p = match_plan(nq, M, n_cu);
    if (nq == 0 || M == 0 || nq > kMatchGridMax) {
        EXPECT(p.chunk == 0 && p.chunks == 0);
        return;
    }
    EXPECT(p.chunk >= 1 && p.chunk <= M);
    EXPECT(p.chunks == ((uint64_t)M + p.chunk - 1) / p.chunk);
    // the workgroup count stays within the grid limit
    EXPECT((uint64_t)nq * p.chunks <= kMatchGridMax);
    // no chunk below the floor except the last: a chunk below the floor is the query's only one
    EXPECT(p.chunk >= kMatchChunkFloor || p.chunks == 1);
    // plain arithmetic: per_query workgroups per query make the launch kMatchWgPerCu per CU; the chunk is the smallest
    // that needs no more than those, raised to the floor, raised to what the grid limit leaves, clipped to the row
    const uint64_t want = (uint64_t)kMatchWgPerCu * n_cu;
    const uint64_t per_query = (want + nq - 1) / nq, room = kMatchGridMax / nq;
    uint64_t expect = ((uint64_t)M + per_query - 1) / per_query;
    if (expect < kMatchChunkFloor) expect = kMatchChunkFloor;
    const bool grid_limited = ((uint64_t)M + expect - 1) / expect > room;
    if (grid_limited) expect = ((uint64_t)M + room - 1) / room;
    if (expect > M) expect = M;
    EXPECT(p.chunk == expect);
    // as large as possible while the launch has its workgroups: above the floor, a chunk one smaller would take more
    // than per_query workgroups per query, and this one does not
    if (p.chunk > kMatchChunkFloor && !grid_limited) {
        EXPECT(p.chunks <= per_query);
        EXPECT(((uint64_t)M + p.chunk - 2) / (p.chunk - 1) > per_query);
    }
    if (cover && M <= (1u << 20)) {
        std::vector<uint8_t> seen(M, 0);
        for (uint32_t ch = 0; ch < p.chunks; ch++) {
            const uint64_t i0 = (uint64_t)ch * p.chunk;
            EXPECT(i0 < M);  // (no idle chunk for a full row)
            const uint64_t i1 = i0 + p.chunk < M ? i0 + p.chunk : M;
            if (ch + 1 < p.chunks) EXPECT(i1 - i0 == p.chunk && (p.chunk >= kMatchChunkFloor));
            for (uint64_t i = i0; i < i1; i++) seen[i]++;
        }
        for (uint32_t i = 0; i < M; i++) EXPECT(seen[i] == 1);
    }
}

int main(int argc, char **argv) {
    if (argc == 4) {
        const MatchPlan p = match_plan((uint32_t)strtoul(argv[1], nullptr, 10), (uint32_t)strtoul(argv[2], nullptr, 10),
                                       (uint32_t)strtoul(argv[3], nullptr, 10));
        printf("%u %u\n", p.chunk, p.chunks);
        return 0;
    }
    static_assert(kMatchChunkFloor == 64, "DESIGN.md 3.4a");
    const uint32_t nqs[] = {0, 1, 2, 3, 7, 100, 511, 512, 1023, 1024, 1025, 16384, 100000, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    const uint32_t Ms[] = {0, 1, 2, 41, 63, 64, 65, 127, 128, 129, 410, 4096, 4097, 4100, 41000, 100000, 1u << 20, 0xFFFFFFFFu};
    const uint32_t cus[] = {1, 64, 256, 304};
    for (uint32_t nq : nqs)
        for (uint32_t M : Ms)
            for (uint32_t cu : cus) check(nq, M, cu, true);
    // what DESIGN.md 3.4a quotes, on 256 compute units: one tray of 41 000 candidates is 641 workgroups, not one
    MatchPlan p = match_plan(1, 41000, 256);
    EXPECT(p.chunk == 64 && p.chunks == 641);
    p = match_plan(1000, 41000, 256);  // two chunks per query would do: 20 500 candidates each
    EXPECT(p.chunk == 20500 && p.chunks == 2);
    p = match_plan(2000, 41000, 256);  // more queries than workgroups wanted: one workgroup per query
    EXPECT(p.chunk == 41000 && p.chunks == 1);
    p = match_plan(3, 65, 256);
    EXPECT(p.chunk == 64 && p.chunks == 2);
    p = match_plan(5, 41, 256);  // a row below the floor: its one chunk is the short last one
    EXPECT(p.chunk == 41 && p.chunks == 1);
    // the grid limit wins over the floor's neighbourhood: 2^31 - 1 queries leave one chunk each
    p = match_plan(0x7FFFFFFFu, 1000, 256);
    EXPECT(p.chunk == 1000 && p.chunks == 1);
    p = match_plan(1u << 30, 1000, 1u << 31);  // wants 8 chunks per query, the grid has room for one
    EXPECT(p.chunks == 1 && p.chunk == 1000);
    // the table: a nibble per column in whole words
    EXPECT(match_table_bytes(0) == 0 && match_table_bytes(1) == 4 && match_table_bytes(8) == 4 && match_table_bytes(9) == 8);
    EXPECT(match_table_bytes(50000) == 25000 && match_table_bytes(150000) == 75000);
    EXPECT(match_table_bytes(327680) == kMatchMaxLds && match_table_bytes(327681) > kMatchMaxLds);
    EXPECT(match_table_bytes(0xFFFFFFFFu) == 4ull * (1ull << 29));
    if (fails) return 1;
    printf("match_plan_check: ok\n");
    return 0;
}
