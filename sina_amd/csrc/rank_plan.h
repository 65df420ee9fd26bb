// Grid of the rank kernel (rank.hip: the max_result best candidates of every query), as plain host code: no HIP, no
// context, no environment -- rank.hip cuts its launch with it and tests/rank_plan_check.cpp runs it without a device.
#pragma once

#include <cstdint>

namespace sina_hip {

// A workgroup builds its query's tables once (zeroing width / 8 bytes of LDS, two passes over the query with an LDS
// atomic per base) and then streams a chunk of that query's candidates; with more than one chunk per query a second
// launch merges the chunks' lists.  So: as few chunks as still give the launch kRankWgPerCu workgroups per compute
// unit, and never fewer than kRankChunkFloor candidates in a chunk.  Thousands of queries with 1000 candidates each
// -- the search stage's shape -- come out as one chunk per query and no merge launch.  (The floor is match_plan.h's
// doubled, for a table build about twice as long; no alternative has been measured.)
constexpr uint32_t kRankChunkFloor = 128;
constexpr uint32_t kRankWgPerCu = 4;
constexpr uint32_t kRankMaxResult = 64;                // rows per query: one per lane of a wave
constexpr uint64_t kRankGridMax = 0x7FFFFFFFull;       // workgroups of a one-dimensional grid
// words of a query's row where the ranking rides on an align call (rank_assembled_kernel): the number of rows, the
// flags, then kRankMaxResult ids and as many score bit patterns -- fixed width, whatever max_result is
constexpr uint32_t kRankRowWords = 2 + 2 * kRankMaxResult;

struct RankPlan {
    uint32_t chunk;   // candidates per workgroup (the last chunk of a query may be short); 0: the launch cannot be cut
    uint32_t chunks;  // workgroups per query: ceil(M / chunk); 1: the workgroup writes the final rows, no merge launch
};

// nq queries with up to M candidates each (a query with fewer leaves its later chunks idle).
// forced != 0: that chunk length whatever the device (SINA_HIP_TEST=rank_chunk=N), still within the grid limit.
inline RankPlan rank_plan(uint32_t nq, uint32_t M, uint32_t n_cu, uint32_t floor = kRankChunkFloor, uint32_t forced = 0) {
    RankPlan p{0, 0};
    if (nq == 0 || M == 0 || (uint64_t)nq > kRankGridMax) return p;
    uint64_t chunk;
    if (forced) {
        chunk = forced;
    } else {
        const uint64_t want_wg = (uint64_t)kRankWgPerCu * (n_cu ? n_cu : 1u);
        uint64_t per_query = (want_wg + nq - 1) / nq;  // chunks a query would need for the launch to reach want_wg
        if (per_query < 1) per_query = 1;
        chunk = ((uint64_t)M + per_query - 1) / per_query;
        if (chunk < floor) chunk = floor;
    }
    const uint64_t room = kRankGridMax / nq;  // chunks per query the grid limit leaves (>= 1)
    if (((uint64_t)M + chunk - 1) / chunk > room) chunk = ((uint64_t)M + room - 1) / room;
    if (chunk > M) chunk = M;
    p.chunk = (uint32_t)chunk;
    p.chunks = (uint32_t)(((uint64_t)M + chunk - 1) / chunk);
    return p;
}

// bytes of the chunks' key rows [nq][chunks][max_result] (0 with one chunk per query: nothing is kept)
inline uint64_t rank_scratch_bytes(uint32_t nq, const RankPlan &p, uint32_t max_result) {
    return p.chunks <= 1 ? 0ull : 8ull * nq * p.chunks * max_result;
}

}  // namespace sina_hip
