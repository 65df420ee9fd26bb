// csrc/rank_plan.h -- the grid of the rank kernel -- against plain arithmetic, as a stand-alone program:
// tests/test_rank_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it once.  With three or
// four arguments (nq M n_cu [forced]) it prints that plan instead, for the test's Python mirror.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rank_plan.h"

using namespace sina_hip;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            fails++;                                                  \
        }                                                             \
    } while (0)

// the properties of one plan; then the chunks of a query walked as the kernel walks them, every candidate counted
static void check(uint32_t nq, uint32_t M, uint32_t n_cu, uint32_t forced) {
    const RankPlan p = rank_plan(nq, M, n_cu, kRankChunkFloor, forced);
    if (nq == 0 || M == 0 || nq > kRankGridMax) {
        EXPECT(p.chunk == 0 && p.chunks == 0);
        return;
    }
    EXPECT(p.chunk >= 1 && p.chunk <= M);
    EXPECT(p.chunks == ((uint64_t)M + p.chunk - 1) / p.chunk);
    EXPECT((uint64_t)nq * p.chunks <= kRankGridMax);
    const uint64_t room = kRankGridMax / nq;
    uint64_t expect;
    bool grid_limited;
    if (forced) {
        expect = forced;
    } else {
        // plain arithmetic: per_query workgroups per query make the launch kRankWgPerCu per CU; the chunk is the
        // smallest that needs no more than those, raised to the floor
        const uint64_t want = (uint64_t)kRankWgPerCu * n_cu;
        const uint64_t per_query = (want + nq - 1) / nq;
        expect = ((uint64_t)M + per_query - 1) / per_query;
        if (expect < kRankChunkFloor) expect = kRankChunkFloor;
        EXPECT(p.chunk >= kRankChunkFloor || p.chunks == 1);  // a chunk below the floor is the query's only one
        if (expect > kRankChunkFloor && ((uint64_t)M + expect - 1) / expect <= room && expect <= M) {
            // as few chunks as still fill the device: one candidate fewer per chunk would take more workgroups than wanted
            EXPECT(((uint64_t)M + expect - 1) / expect <= per_query);
            EXPECT(expect == 1 || ((uint64_t)M + expect - 2) / (expect - 1) > per_query);
        }
    }
    grid_limited = ((uint64_t)M + expect - 1) / expect > room;
    if (grid_limited) expect = ((uint64_t)M + room - 1) / room;
    if (expect > M) expect = M;
    EXPECT(p.chunk == expect);
    EXPECT(rank_scratch_bytes(nq, p, 64) == (p.chunks == 1 ? 0ull : 8ull * 64 * nq * p.chunks));
    if (M <= (1u << 20)) {
        std::vector<uint8_t> seen(M, 0);
        for (uint32_t ch = 0; ch < p.chunks; ch++) {
            const uint64_t i0 = (uint64_t)ch * p.chunk;
            EXPECT(i0 < M);  // (no idle chunk for a full row)
            const uint64_t i1 = i0 + p.chunk < M ? i0 + p.chunk : M;
            if (ch + 1 < p.chunks) EXPECT(i1 - i0 == p.chunk);
            for (uint64_t i = i0; i < i1; i++) seen[i]++;
        }
        for (uint32_t i = 0; i < M; i++) EXPECT(seen[i] == 1);
    }
}

int main(int argc, char **argv) {
    if (argc == 4 || argc == 5) {
        const RankPlan p = rank_plan((uint32_t)strtoul(argv[1], nullptr, 10), (uint32_t)strtoul(argv[2], nullptr, 10),
                                     (uint32_t)strtoul(argv[3], nullptr, 10), kRankChunkFloor,
                                     argc == 5 ? (uint32_t)strtoul(argv[4], nullptr, 10) : 0u);
        printf("%u %u\n", p.chunk, p.chunks);
        return 0;
    }
    static_assert(kRankChunkFloor == 128 && kRankWgPerCu == 4 && kRankMaxResult == 64, "DESIGN.md 3.5a");
    const uint32_t nqs[] = {0, 1, 2, 3, 7, 64, 100, 511, 512, 1023, 1024, 1025, 9216, 16384, 100000, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    const uint32_t Ms[] = {0, 1, 2, 10, 11, 12, 13, 127, 128, 129, 255, 256, 257, 1000, 4096, 100000, 1u << 20, 0xFFFFFFFFu};
    const uint32_t cus[] = {1, 64, 256, 304};
    const uint32_t forceds[] = {0, 1, 3, 4, 1000, 0xFFFFFFFFu};
    for (uint32_t nq : nqs)
        for (uint32_t M : Ms)
            for (uint32_t cu : cus)
                for (uint32_t f : forceds) {
                    if (f && f < 1000 && M > (1u << 20)) continue;  // (a forced chunk is a test's: small rows)
                    check(nq, M, cu, f);
                }
    // the search stage's shape on 256 compute units: thousands of queries x 1000 candidates is one chunk per query
    RankPlan p = rank_plan(9216, 1000, 256);
    EXPECT(p.chunk == 1000 && p.chunks == 1);
    p = rank_plan(1024, 1000, 256);
    EXPECT(p.chunks == 1);
    p = rank_plan(512, 1000, 256);  // half as many queries as workgroups wanted: two chunks each
    EXPECT(p.chunk == 500 && p.chunks == 2);
    p = rank_plan(64, 100000, 256);  // search-all at 64 queries: 16 chunks per query
    EXPECT(p.chunk == 6250 && p.chunks == 16);
    p = rank_plan(1, 1000, 256);  // the floor decides: 8 chunks, not 1000
    EXPECT(p.chunk == 128 && p.chunks == 8);
    p = rank_plan(1, 10, 256);  // a row below the floor is one chunk
    EXPECT(p.chunk == 10 && p.chunks == 1);
    p = rank_plan(1, 10, 256, kRankChunkFloor, 3);  // ... unless a test cuts it
    EXPECT(p.chunk == 3 && p.chunks == 4);
    p = rank_plan(2, 13, 256, kRankChunkFloor, 4);
    EXPECT(p.chunk == 4 && p.chunks == 4);
    p = rank_plan(0x7FFFFFFFu, 1000, 256, kRankChunkFloor, 3);  // the grid limit wins over a forced chunk
    EXPECT(p.chunk == 1000 && p.chunks == 1);
    if (fails) return 1;
    printf("rank_plan_check: ok\n");
    return 0;
}
