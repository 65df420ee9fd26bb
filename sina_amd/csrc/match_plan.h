// Grid of the match-count kernel (match.hip: one counter per (query, candidate) pair), as plain host code: no HIP,
// no context, no environment -- match.hip cuts its launch with it and tests/match_plan_check.cpp runs it without a
// device.
#pragma once

#include <cstdint>

namespace sina_hip {

// A workgroup builds its query's column table once and then streams a chunk of that query's candidates.  Chunks are
// as large as they can be while the launch still has kMatchWgPerCu workgroups per compute unit, and never smaller
// than kMatchChunkFloor candidates, which amortise the table build (zeroing width / 2 bytes of LDS, one atomic per query
// base).  DESIGN.md 3.4a has the floor's measured alternatives: 256 and more lose wherever the floor decides the grid,
// 16 gains 0.03 ms on a single tray of 41 000 candidates and nothing from four trays on.
constexpr uint32_t kMatchChunkFloor = 64;
constexpr uint32_t kMatchWgPerCu = 4;
constexpr uint64_t kMatchGridMax = 0x7FFFFFFFull;  // workgroups of a one-dimensional grid

struct MatchPlan {
    uint32_t chunk;   // candidates per workgroup (the last chunk of a query may be short); 0: the launch cannot be cut
    uint32_t chunks;  // workgroups per query: ceil(M / chunk)
};

// nq queries with up to M candidates each (M = the row length: a query with fewer leaves its later chunks idle).
// (floor: kMatchChunkFloor, or what tools/perf_msc.py tries beside it)
inline MatchPlan match_plan(uint32_t nq, uint32_t M, uint32_t n_cu, uint32_t floor = kMatchChunkFloor) {
    MatchPlan p{0, 0};
    if (nq == 0 || M == 0 || (uint64_t)nq > kMatchGridMax) return p;
    const uint64_t want_wg = (uint64_t)kMatchWgPerCu * (n_cu ? n_cu : 1u);
    uint64_t per_query = (want_wg + nq - 1) / nq;  // chunks a query would need for the launch to reach want_wg
    if (per_query < 1) per_query = 1;
    uint64_t chunk = ((uint64_t)M + per_query - 1) / per_query;
    if (chunk < floor) chunk = floor;
    const uint64_t room = kMatchGridMax / nq;  // chunks per query the grid limit leaves (>= 1)
    if (((uint64_t)M + chunk - 1) / chunk > room) chunk = ((uint64_t)M + room - 1) / room;
    if (chunk > M) chunk = M;
    p.chunk = (uint32_t)chunk;
    p.chunks = (uint32_t)(((uint64_t)M + chunk - 1) / chunk);
    return p;
}

// LDS the kernel's table takes for an alignment of `width` columns: one nibble per column in 32-bit words
inline uint64_t match_table_bytes(uint32_t width) { return 4ull * (((uint64_t)width + 7) / 8); }
// ... and what a workgroup may have of a CU's 160 KiB (the kernel keeps no other LDS)
constexpr uint64_t kMatchMaxLds = 160 * 1024;

}  // namespace sina_hip
