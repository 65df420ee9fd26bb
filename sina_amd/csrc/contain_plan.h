// Planning of the containment kernel (contain.hip, find_bases_kernel: the lowest start of a query's bases in a
// reference's, one word per (query, reference) pair), as plain host code: no HIP, no context, no environment --
// contain.hip sizes and cuts its launches with it, the host pre-pass reads its answers with it and
// tests/contain_plan_check.cpp runs it without a device.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace sina_hip {

constexpr uint32_t kContainNone = 0xFFFFFFFFu;  // the answer of a pair without a hit (std::string::npos)
constexpr uint32_t kContainMaxBases = 65535;    // a query's bases; 0 is refused too

// one wave per pair, kContainPairsPerWg waves to a workgroup
constexpr uint32_t kContainWave = 64;
constexpr uint32_t kContainPairsPerWg = 4;
constexpr uint32_t kContainThreads = kContainWave * kContainPairsPerWg;
inline uint32_t contain_grid(uint32_t n_pairs) { return (n_pairs + kContainPairsPerWg - 1) / kContainPairsPerWg; }

// The filter's key: the first min(n, 8) four-bit codes of a sequence in one word, code j in bits 4j .. 4j + 3.
constexpr uint32_t kContainKeyBases = 8;
constexpr uint32_t contain_key_mask(uint32_t n) { return n >= kContainKeyBases ? 0xFFFFFFFFu : (1u << (4 * n)) - 1u; }
// The queries go up packed, eight codes to a word, every query on a word of its own: query q's words
inline uint64_t contain_query_words(uint64_t n_bases) { return (n_bases + 7) / 8; }
// host code of the packing (what the kernel reads back): n mask bytes -> contain_query_words(n) words
inline void contain_pack_query(const uint8_t *mask, uint64_t n, uint32_t *words) {
    for (uint64_t w = 0; w < contain_query_words(n); w++) {
        uint32_t v = 0;
        for (uint64_t j = 8 * w; j < n && j < 8 * w + 8; j++) v |= (uint32_t)(mask[j] & 0xFu) << (4 * (j - 8 * w));
        words[w] = v;
    }
}
// Staging of a launch range of n pairs: the pairs' reference ids and query numbers up, their answers down
inline size_t contain_pair_bytes(uint64_t n_pairs) { return 4 * (size_t)n_pairs; }

// A launch takes a range of consecutive pairs, kContainRangePairs at the most (4 MiB each way of staging, a grid of
// 2^18 workgroups); SINA_HIP_TEST=contain_pairs=N: N.
constexpr uint64_t kContainRangePairs = 1ull << 20;

struct ContainRange {
    uint64_t p0, p1;  // pairs [p0, p1) of the call
};
// The ranges are not empty, follow each other without a gap and cover 0 .. n_pairs.
inline std::vector<ContainRange> contain_ranges(uint64_t n_pairs, uint64_t max_pairs = kContainRangePairs) {
    std::vector<ContainRange> out;
    if (max_pairs == 0) max_pairs = 1;
    if (max_pairs > kContainRangePairs) max_pairs = kContainRangePairs;
    for (uint64_t p0 = 0; p0 < n_pairs; p0 += max_pairs) out.push_back(ContainRange{p0, p0 + max_pairs < n_pairs ? p0 + max_pairs : n_pairs});
    return out;
}

// Upper bound on the verify steps (64 bases compared per step) a pair of n query and R reference bases can take:
// every start a candidate, every candidate failing in its last step -- a homopolymer against a needle that differs
// in its last base.
inline uint64_t contain_worst_steps(uint64_t n, uint64_t R) { return n > R ? 0 : (R - n + 1) * ((n + 63) / 64); }

}  // namespace sina_hip
