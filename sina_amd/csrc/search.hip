// Search-stage sequence comparison on the GPU + sina_hip_compare.
//
// What it computes: for every (query, candidate reference) pair the six counters of
// match_counter as traverse() fills them (reference src/cseq_comparator.cpp:56-111,146-206):
// match / mismatch on columns where both sequences have an unfiltered base, only_a / only_b for
// bases inside the other sequence's column range without a partner, and the overhang counters for
// bases outside that range.  search_filter::operator() calls this once per k-mer candidate --
// 1000 times per query (src/search_filter.cpp:311-313).
//
// How it maps to the hardware: the reference walks both base lists in lock-step, but every
// counter is a function of column membership only:
//   * a base of B (candidate) at column p is an overhang if p lies outside [first, last] unfiltered
//     column of A (query), a match/mismatch if A has an unfiltered base at p, only_b otherwise;
//   * for A the same with roles swapped, and those three numbers follow from counts:
//     in-range(A) = rankA(lastB + 1) - rankA(firstB); only_a = in-range(A) - (match + mismatch);
//     overhang(A) = |A| - in-range(A);
//   * filtered (lower-case) bases behave as absent: in the lock-step walk a filtered base never
//     increments a counter, and its partner, if any, is counted exactly as an unpartnered base.
// One workgroup per query keeps A in LDS as a column bitmap + per-word popcount prefix (rank) +
// the base masks in rank order; each wave then streams one candidate at a time from HBM
// (coalesced 4-byte reads, every base read once) and reduces its counters with wave shuffles.
// HBM-bound: algorithmic bytes = 4 B x sum of candidate lengths (6 MB per query at 1000
// candidates x 1500 bases).
#include <algorithm>
#include <cstring>

#include "common.h"
#include "ctx.h"
#include "compare_dev.h"

namespace sina_hip {
namespace {

struct CompareArgs {
    const uint32_t *ref_ab;
    const uint64_t *ref_off;
    const uint32_t *q_ab;
    const uint64_t *q_off;
    const uint32_t *cand_ids;
    const uint64_t *cand_off;
    sina_hip_match_counts *out;
    uint32_t width, n_refs;
    int iupac, filter_lc;
};

// (the tables and the per-candidate classification: compare_dev.h, shared with rank.hip)
__global__ void __launch_bounds__(kCT) compare_kernel(CompareArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_tmp[8];
    __shared__ uint32_t s_scal[3];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t *A = a.q_ab + a.q_off[q];
    const uint32_t la = (uint32_t)(a.q_off[q + 1] - a.q_off[q]);
    const uint32_t lc_bit = a.filter_lc ? 0x10u : 0u;  // filtered <=> (mask byte & lc_bit) != 0
    const QueryTables t = build_query_tables(smem, s_tmp, s_scal, A, la, a.width, lc_bit);

    const uint64_t c0 = a.cand_off[q], c1 = a.cand_off[q + 1];
    for (uint64_t c = c0 + wave; c < c1; c += kCT / 64) {
        const uint32_t id = a.cand_ids[c];
        const bool valid = id < a.n_refs;
        const uint32_t *Bp = valid ? a.ref_ab + a.ref_off[id] : nullptr;
        const uint32_t lb = valid ? (uint32_t)(a.ref_off[id + 1] - a.ref_off[id]) : 0u;
        const sina_hip_match_counts m = classify_candidate(t, Bp, lb, valid, lc_bit, a.iupac, lane);
        if (lane == 0) a.out[c] = m;
    }
}

}  // namespace
}  // namespace sina_hip

using namespace sina_hip;

extern "C" int sina_hip_compare(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq,
                                const uint32_t *cand_ids, const uint64_t *cand_off, int iupac_rule,
                                int filter_lowercase, sina_hip_match_counts *out) {
    if (!c || !q_ab || !q_off || !cand_off || !out) SH_FAIL("compare: null argument");
    if (iupac_rule < 0 || iupac_rule > 2) SH_FAIL("compare: unknown iupac rule");
    std::lock_guard<std::mutex> lk(c->mu);
    sina_hip_hint_guard hints(c);
    if (!c->st->have_refs) SH_FAIL("compare: upload references first");
    if (nq == 0) return 0;
    SH_CHECK(hipSetDevice(c->device));
    const uint64_t nqa = q_off[nq] - q_off[0], ncand = cand_off[nq] - cand_off[0];
    if (ncand == 0) return 0;
    if (!cand_ids) SH_FAIL("compare: null candidate ids");
    uint32_t max_la = 0;
    std::vector<uint64_t> qrel(nq + 1), crel(nq + 1);
    for (uint32_t q = 0; q <= nq; q++) {
        qrel[q] = q_off[q] - q_off[0];
        crel[q] = cand_off[q] - cand_off[0];
        if (q < nq) max_la = std::max<uint32_t>(max_la, (uint32_t)(q_off[q + 1] - q_off[q]));
    }
    if (max_la > 65535) SH_FAIL("compare: query longer than 65535 bases");
    for (uint64_t i = 0; i < ncand; i++)
        if (cand_ids[cand_off[0] + i] >= c->st->n_refs) SH_FAIL("compare: reference id out of range");
    const size_t lds = compare_table_bytes(c->st->width, max_la);
    if (lds > kCompareMaxLds) SH_FAIL("compare: alignment too wide for the device comparison");
    hipStream_t s = c->stream;
    if (c->s_qab.reserve(4 * std::max<uint64_t>(nqa, 1)) || c->s_qoff.reserve(8 * ((uint64_t)nq + 1)) ||
        c->s_cand.reserve(4 * ncand) || c->s_coff.reserve(8 * ((uint64_t)nq + 1)) ||
        c->s_out.reserve(sizeof(sina_hip_match_counts) * ncand))
        return 1;
    SH_CHECK(hipMemcpyAsync(c->s_qab.p, q_ab + q_off[0], 4 * nqa, hipMemcpyHostToDevice, s));
    SH_CHECK(hipMemcpyAsync(c->s_qoff.p, qrel.data(), 8 * ((uint64_t)nq + 1), hipMemcpyHostToDevice, s));
    SH_CHECK(hipMemcpyAsync(c->s_cand.p, cand_ids + cand_off[0], 4 * ncand, hipMemcpyHostToDevice, s));
    SH_CHECK(hipMemcpyAsync(c->s_coff.p, crel.data(), 8 * ((uint64_t)nq + 1), hipMemcpyHostToDevice, s));
    CompareArgs a;
    a.ref_ab = c->st->ref_ab.as<uint32_t>();
    a.ref_off = c->st->ref_off.as<uint64_t>();
    a.q_ab = c->s_qab.as<uint32_t>();
    a.q_off = c->s_qoff.as<uint64_t>();
    a.cand_ids = c->s_cand.as<uint32_t>();
    a.cand_off = c->s_coff.as<uint64_t>();
    a.out = c->s_out.as<sina_hip_match_counts>();
    a.width = c->st->width;
    a.n_refs = c->st->n_refs;
    a.iupac = iupac_rule;
    a.filter_lc = filter_lowercase ? 1 : 0;
    if (allow_full_lds(reinterpret_cast<const void *>(compare_kernel))) return 1;
    SH_CHECK(hipEventRecord(c->ev[3], s));
    hipLaunchKernelGGL(compare_kernel, dim3(nq), dim3(kCT), lds, s, a);
    SH_CHECK(hipGetLastError());
    SH_CHECK(hipEventRecord(c->ev[4], s));
    // (wait for the kernel first: see HostBuf in common.h)
    SH_CHECK(hipStreamSynchronize(s));
    SH_CHECK(hipMemcpyAsync(out, c->s_out.p, sizeof(sina_hip_match_counts) * ncand, hipMemcpyDeviceToHost, s));
    SH_CHECK(hipStreamSynchronize(s));
    float ms = 0;
    SH_CHECK(hipEventElapsedTime(&ms, c->ev[3], c->ev[4]));
    uint64_t bases = 0;
    if (ensure_ref_off_host(c) == 0)
        for (uint64_t i = 0; i < ncand; i++) {
            const uint32_t id = cand_ids[cand_off[0] + i];
            bases += c->st->ref_off_host[id + 1] - c->st->ref_off_host[id];
        }
    std::lock_guard<std::mutex> slk(c->st->stats_mu);
    c->st->stats.compare_ms += ms;
    c->st->stats.compare_bases += bases;
    c->st->stats.compare_launches++;
    return 0;
}
