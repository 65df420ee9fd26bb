// Shape of the family cascade (family.hip: famfinder's filter cascade over the select's rows, one wave per query), as
// plain host code: no HIP, no context, no environment -- family.hip sizes its rows and cuts its launch with it, the
// host stages ask it whether a rule fits, and tests/family_plan_check.cpp runs it without a device.
#pragma once

#include <cstdint>

namespace sina_hip {

// The most entries a family can have under a rule: a candidate kept once `have` has reached both
// fs_min and fs_max raises a quota counter that is still below its quota, and the quotas are fs_req_full, and
// fs_cover_gene on either side.  64-bit: the options are 32-bit numbers of the user's.
inline uint64_t family_bound(uint32_t fs_min, uint32_t fs_max, uint32_t fs_req_full, uint32_t fs_cover_gene) {
    return (uint64_t)(fs_min > fs_max ? fs_min : fs_max) + fs_req_full + 2ull * fs_cover_gene;
}

// A rule whose bound exceeds kFamilyCascadeMaxK is refused, as a limit (the host cascade takes over): a row is
// 2 + 2 K words, 8 KiB at the cap, and every query of a round brings one down.  (The device's family builders take
// 128 members, ctx.h kFamilyMax: a family anywhere near the cap is not aligned on the device either.)
constexpr uint32_t kFamilyCascadeMaxK = 1024;

// Row of a query: word 0 the number kept, word 1 flags, K ids, K score bit patterns
constexpr uint32_t kFamilyFlagEnough = 1u, kFamilyFlagEmpty = 2u;
constexpr uint32_t family_row_words(uint32_t K) { return 2u + 2u * K; }

// One wave per query, kFamilyWavesPerWg queries per workgroup
constexpr uint32_t kFamilyWavesPerWg = 4;

struct FamilyPlan {
    bool ok;             // false: the rule's bound is over the cap
    uint32_t K;          // entries of a row
    uint32_t row_words;  // 2 + 2 K
    uint32_t grid;       // workgroups of nq queries
};

inline FamilyPlan family_plan(uint32_t fs_min, uint32_t fs_max, uint32_t fs_req_full, uint32_t fs_cover_gene, uint32_t nq) {
    FamilyPlan p{false, 0, 0, 0};
    const uint64_t K = family_bound(fs_min, fs_max, fs_req_full, fs_cover_gene);
    if (K > kFamilyCascadeMaxK) return p;
    p.ok = true;
    p.K = (uint32_t)K;
    p.row_words = family_row_words(p.K);
    p.grid = (uint32_t)(((uint64_t)nq + kFamilyWavesPerWg - 1) / kFamilyWavesPerWg);
    return p;
}

}  // namespace sina_hip
