// Device code the comparison kernels share (search.hip: compare_kernel writes every pair's counters; rank.hip:
// rank_kernel turns them into a score and keeps the best; identity.hip: family_identity_kernel keeps the best overlap
// score of an assembled query's family): the query's LDS tables, the classification of one candidate's bases against
// them and the cover rule's denominator.  See search.hip for what the counters mean and why column membership decides them.
#pragma once

#include "common.h"

namespace sina_hip {

constexpr int kCT = 256;  // threads per workgroup of both kernels

// LDS a workgroup's tables take for an alignment of `width` columns and a query of `max_la` bases
constexpr size_t compare_table_bytes(uint32_t width, uint32_t max_la) {
    const size_t nwords = ((size_t)width + 31) / 32;
    return 4 * nwords + 2 * (nwords + 2) + ((size_t)max_la + 15) + 16;
}
constexpr size_t kCompareMaxLds = 150 * 1024;

// The query A of a workgroup, in LDS
struct QueryTables {
    uint32_t *bitmap;  // [nwords] unfiltered columns of A
    uint16_t *wrank;   // [nwords + 1] bases before the word
    uint8_t *amask;    // [|A|] iupac mask by rank
    uint32_t nwords, width;
    uint32_t aF, aL, nA;  // first / last unfiltered column, number of unfiltered bases
    // number of unfiltered A bases in columns < p (p <= width)
    __device__ __forceinline__ uint32_t rank(uint32_t p) const {
        const uint32_t wd = p >> 5;
        if (wd >= nwords) return wrank[nwords];
        return (uint32_t)wrank[wd] + __popc(bitmap[wd] & ((1u << (p & 31)) - 1u));
    }
};

// Built by all kCT threads of the workgroup.  smem: compare_table_bytes() of LDS; s_tmp: [8], s_scal: [3] words of LDS.
__device__ __forceinline__ QueryTables build_query_tables(unsigned char *smem, uint32_t *s_tmp, uint32_t *s_scal, const uint32_t *A,
                                                           uint32_t la, uint32_t width, uint32_t lc_bit) {
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    QueryTables t;
    t.width = width;
    t.nwords = (width + 31) / 32;
    const uint32_t nwords = t.nwords;
    t.bitmap = reinterpret_cast<uint32_t *>(smem);
    t.wrank = reinterpret_cast<uint16_t *>(t.bitmap + nwords);
    t.amask = reinterpret_cast<uint8_t *>(t.wrank + nwords + 2);
    uint32_t *bitmap = t.bitmap;
    uint16_t *wrank = t.wrank;
    uint32_t &s_first = s_scal[0], &s_last = s_scal[1], &s_na = s_scal[2];

    for (uint32_t i = tid; i < nwords; i += kCT) bitmap[i] = 0;
    if (tid == 0) {
        s_first = 0xFFFFFFFFu;
        s_last = 0;
    }
    __syncthreads();
    for (uint32_t i = tid; i < la; i += kCT) {
        const uint32_t ab = A[i];
        if ((ab >> 24) & lc_bit) continue;
        const uint32_t pos = ab & 0xFFFFFFu;
        if (pos >= width) continue;  // (cannot happen for a sequence of this alignment)
        atomicOr(&bitmap[pos >> 5], 1u << (pos & 31));
        atomicMin(&s_first, pos);
        atomicMax(&s_last, pos);
    }
    __syncthreads();
    {   // exclusive prefix popcount over the bitmap words
        const uint32_t chunk = (nwords + kCT - 1) / kCT;
        const uint32_t b = min(nwords, tid * chunk), e = min(nwords, b + chunk);
        uint32_t s = 0;
        for (uint32_t i = b; i < e; i++) s += __popc(bitmap[i]);
        uint32_t x = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63) s_tmp[wave] = x;
        __syncthreads();
        uint32_t base = 0, total = 0;
        for (int w = 0; w < kCT / 64; w++) {
            if (w < wave) base += s_tmp[w];
            total += s_tmp[w];
        }
        uint32_t run = base + x - s;
        for (uint32_t i = b; i < e; i++) {
            wrank[i] = (uint16_t)run;
            run += __popc(bitmap[i]);
        }
        if (tid == 0) {
            wrank[nwords] = (uint16_t)total;
            s_na = total;
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < la; i += kCT) {
        const uint32_t ab = A[i];
        if ((ab >> 24) & lc_bit) continue;
        const uint32_t pos = ab & 0xFFFFFFu;
        if (pos >= width) continue;
        t.amask[t.rank(pos)] = (uint8_t)((ab >> 24) & 0xFu);
    }
    __syncthreads();
    t.aF = s_first;
    t.aL = s_last;
    t.nA = s_na;
    return t;
}

// One wave streams candidate B (lb packed bases; valid: the id was in range) against the tables and reduces: every
// lane returns the pair's six counters.
__device__ __forceinline__ sina_hip_match_counts classify_candidate(const QueryTables &t, const uint32_t *Bp, uint32_t lb, bool valid,
                                                                    uint32_t lc_bit, int iupac, int lane) {
    int32_t n_match = 0, n_mis = 0, n_onlyb = 0, n_ovb = 0;
    uint32_t bF = 0xFFFFFFFFu, bL = 0;
    if (valid && t.nA != 0) {
        for (uint32_t i = lane; i < lb; i += 64) {
            const uint32_t ab = Bp[i];
            if ((ab >> 24) & lc_bit) continue;
            const uint32_t pos = ab & 0xFFFFFFu;
            bF = min(bF, pos);
            bL = max(bL, pos);
            if (pos < t.aF || pos > t.aL) {
                n_ovb++;
            } else if ((t.bitmap[pos >> 5] >> (pos & 31)) & 1u) {
                const uint32_t ma = t.amask[t.rank(pos)], mb = (ab >> 24) & 0xFu;
                bool eq;
                if (iupac == SINA_CMP_IUPAC_OPTIMISTIC) eq = (ma & mb) != 0;       // aligned_base.h:153-155
                else if (iupac == SINA_CMP_IUPAC_PESSIMISTIC) eq = (__popc(ma) <= 1) && ma == mb;  // :163-165
                else eq = ma == mb;                                                  // :167-169
                if (eq) n_match++;
                else n_mis++;
            } else {
                n_onlyb++;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_match += __shfl_xor(n_match, off);
        n_mis += __shfl_xor(n_mis, off);
        n_onlyb += __shfl_xor(n_onlyb, off);
        n_ovb += __shfl_xor(n_ovb, off);
        bF = min(bF, (uint32_t)__shfl_xor((int)bF, off));
        bL = max(bL, (uint32_t)__shfl_xor((int)bL, off));
    }
    sina_hip_match_counts m;
    if (bF == 0xFFFFFFFFu || t.nA == 0) {  // one side has no unfiltered base
        m.only_a_overhang = m.only_b_overhang = m.only_a = m.only_b = m.match = m.mismatch = 0;
    } else {
        const int32_t in_a = (int32_t)(t.rank(bL + 1) - t.rank(bF));
        m.match = n_match;
        m.mismatch = n_mis;
        m.only_b = n_onlyb;
        m.only_b_overhang = n_ovb;
        m.only_a = in_a - (n_match + n_mis);
        m.only_a_overhang = (int32_t)t.nA - in_a;
    }
    return m;
}

// The denominator cseq_comparator::score divides the matches by, in int32 as there (SINA_CMP_COVER_* in
// CMP_COVER_TYPE's order); 0: the host's 0 / 0.
__device__ __forceinline__ int32_t cover_denominator(const sina_hip_match_counts &m, int cover) {
    const int32_t paired = m.match + m.mismatch;
    const int32_t a_alone = m.only_a + m.only_a_overhang, b_alone = m.only_b + m.only_b_overhang;
    switch (cover) {
    case SINA_CMP_COVER_ABS: return 1;
    case SINA_CMP_COVER_QUERY: return paired + a_alone;
    case SINA_CMP_COVER_TARGET: return paired + b_alone;
    case SINA_CMP_COVER_OVERLAP: return paired + m.only_a + m.only_b;
    case SINA_CMP_COVER_ALL: return paired + m.only_a + m.only_b + m.only_a_overhang + m.only_b_overhang;
    case SINA_CMP_COVER_AVERAGE: return paired + (m.only_a + m.only_b + m.only_a_overhang + m.only_b_overhang) / 2;
    case SINA_CMP_COVER_MIN: return paired + min(a_alone, b_alone);
    case SINA_CMP_COVER_MAX: return paired + max(a_alone, b_alone);
    default: return paired;  // SINA_CMP_COVER_NOGAP
    }
}

}  // namespace sina_hip
