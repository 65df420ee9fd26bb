// Device code the two pair-count kernels share (pairs.hip: pair_count_kernel counts over words the host uploaded,
// pair_count_assembled_kernel over the words assemble_kernel left in device memory): the look-up of what a sequence
// shows in a column, the classification of a pair of columns, and a wave's count over the compacted helix map.  One
// piece of code for both, so that the two routes give the same six counters by construction.  See pairs.hip for what
// the counters mean.
#pragma once

#include "common.h"

namespace sina_hip {

constexpr uint32_t kGap = 32;  // "no base in that column": beside the 5-bit masks 0..31

// What the sequence shows in column c: the five mask bits of the first word whose column is >= c if that column is c,
// else kGap.  (A column of 2^24 or more is beyond every word: the search ends at len.)  The words' columns must not
// descend.
__device__ __forceinline__ uint32_t mask_at(const uint32_t *W, uint32_t len, uint32_t c) {
    if (len == 0) return kGap;
    uint32_t base = 0, n = len;
    while (n > 1) {  // (lower_bound without a branch on the data: answer in [base, base + n])
        const uint32_t half = n >> 1;
        base = (W[base + half] & 0xFFFFFFu) < c ? base + half : base;
        n -= half;
    }
    const uint32_t w0 = W[base];
    const uint32_t at = base + ((w0 & 0xFFFFFFu) < c ? 1u : 0u);
    const uint32_t w = at < len ? W[at] : 0xFFFFFFFFu;  // (at <= len; at == len: no word at or after c)
    return (at < len && (w & 0xFFFFFFu) == c) ? ((w >> 24) & 31u) : kGap;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// One wave's count for one sequence (W[0 .. len): its packed words): the lanes stride over the map's n_ent entries,
// the wave adds the six counters up across lanes and lane 0 stores them at o[0 .. 6): num, AG, AU, CG, GG, GU.
// Every lane of the wave must call it (the sums shuffle across all 64).
__device__ __forceinline__ void pair_count_wave(const uint32_t *W, uint32_t len, const uint2 *ent, uint32_t n_ent, uint32_t lane,
                                                uint32_t *o) {
    uint32_t num = 0, ag = 0, au = 0, cg = 0, gg = 0, gu = 0;
    for (uint32_t e = lane; e < n_ent; e += 64) {
        const uint2 en = ent[e];
        const uint32_t l = mask_at(W, len, en.x), r = mask_at(W, len, en.y);
        // '.': a word without mask bits, either case
        const bool dot = (l != kGap && (l & 15u) == 0) || (r != kGap && (r & 15u) == 0);
        const bool counted = !dot && !(l == kGap && r == kGap);
        num += counted ? 1u : 0u;
        // the weighted classes: two upper-case bases of one bit each (A 1, G 2, C 4, U 8)
        const bool plain = counted && l < 16u && r < 16u && __popc(l) == 1 && __popc(r) == 1;
        const uint32_t both = l | r;
        ag += (plain && both == 3u) ? 1u : 0u;
        au += (plain && both == 9u) ? 1u : 0u;
        cg += (plain && both == 6u) ? 1u : 0u;
        gg += (plain && l == 2u && r == 2u) ? 1u : 0u;
        gu += (plain && both == 10u) ? 1u : 0u;
    }
    num = wave_sum(num);
    ag = wave_sum(ag);
    au = wave_sum(au);
    cg = wave_sum(cg);
    gg = wave_sum(gg);
    gu = wave_sum(gu);
    if (lane == 0) {
        o[0] = num;
        o[1] = ag;
        o[2] = au;
        o[3] = cg;
        o[4] = gg;
        o[5] = gu;
    }
}

}  // namespace sina_hip
