// Planning of the helix base-pair count (pairs.hip: six counters per aligned sequence), as plain host code: no HIP,
// no context, no environment -- pairs.hip compacts the helix map and cuts its launches with it and
// tests/pair_plan_check.cpp runs it without a device.
#pragma once

#include <cstdint>
#include <vector>

namespace sina_hip {

// The helix map as the kernel reads it: one entry (column, partner column) for every column that has a partner
// (pairs[i] != 0), ascending in the column; two words per entry.  The kernel's lanes stride over this list, so a
// 50 000-column map with 900 paired columns costs 900 entries, not 50 000 tests.
inline std::vector<uint32_t> pair_compact(const uint32_t *pairs, uint32_t n) {
    std::vector<uint32_t> ent;
    for (uint32_t i = 0; i < n; i++)
        if (pairs[i] != 0) {
            ent.push_back(i);
            ent.push_back(pairs[i]);
        }
    return ent;
}

// A launch takes a range of consecutive sequences: as many as keep the words uploaded for it within kPairRangeWords
// (256 MiB of staging and device memory) and the wave count within kPairRangeSeqs, one sequence at least -- a
// sequence larger than the limit opens a range of its own.  A sequence without words adds nothing and always joins.
constexpr uint64_t kPairRangeWords = 1ull << 26;
constexpr uint32_t kPairRangeSeqs = 1u << 22;

struct PairRange {
    uint32_t q0, q1;  // sequences [q0, q1) of the call
};

// q_off [nq + 1], ascending (absolute offsets: only differences count).  The ranges are not empty, follow each
// other without a gap and cover 0 .. nq.
inline std::vector<PairRange> pair_ranges(const uint64_t *q_off, uint32_t nq, uint64_t max_words = kPairRangeWords,
                                          uint32_t max_seqs = kPairRangeSeqs) {
    std::vector<PairRange> out;
    if (max_seqs == 0) max_seqs = 1;
    uint32_t q0 = 0;
    while (q0 < nq) {
        uint32_t q1 = q0 + 1;
        while (q1 < nq && q1 - q0 < max_seqs && (q_off[q1 + 1] - q_off[q0] <= max_words || q_off[q1 + 1] == q_off[q1])) q1++;
        out.push_back(PairRange{q0, q1});
        q0 = q1;
    }
    return out;
}

// the kernel runs one wave per sequence, kPairWaves of them in a workgroup
constexpr uint32_t kPairWaves = 4;
inline uint32_t pair_grid(uint32_t n_seqs) { return (n_seqs + kPairWaves - 1) / kPairWaves; }

// first sequence whose columns descend somewhere (equal neighbours are fine), or nq
inline uint32_t pair_first_descending(const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq) {
    for (uint32_t q = 0; q < nq; q++)
        for (uint64_t i = q_off[q] + 1; i < q_off[q + 1]; i++)
            if ((q_ab[i] & 0xFFFFFFu) < (q_ab[i - 1] & 0xFFFFFFu)) return q;
    return nq;
}

}  // namespace sina_hip
