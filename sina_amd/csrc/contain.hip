// The aligner's exact-relative test on the GPU: find_bases_kernel + sina_hip_find_bases,
// sina_hip_find_bases_stats.  The kernel's counters are the context's use[kUseContain].
//
// What it computes: for a pair (query of n bases, reference of R bases) std::string::find's answer over the bases'
// four-bit codes -- the lowest start i in 0 .. R - n with query[j] == ref[i + j] for every j, kContainNone without one
// or with n > R.  Codes are compared for EQUALITY (upper-cased characters of two bases are equal exactly when their
// codes are: base_iupac is one-to-one on the code, T and U share one, bit 4 is the case): what boost::icontains asks
// at src/align.cpp:329-388, not what the DP's comp() asks.
//
// How it maps to the hardware: one wave per pair, kContainPairsPerWg waves to a workgroup; the waves of a workgroup
// share nothing (no LDS, no barrier: they leave when their pair is done).  The query comes packed, eight codes to a
// word (contain_plan.h), its first min(n, 8) codes are the key.  The wave sweeps the starts in ascending chunks of 64,
// a start per lane: one coalesced dword load of the reference's packed words per lane (plus seven lanes' overhang),
// the lane's own key of eight codes assembled from its neighbours' in three rounds of shuffles, __ballot of the lanes
// whose key is the query's.  Candidates are verified lowest first (__ffsll), all 64 lanes comparing query[j] with
// ref[i + j] for j = lane, lane + 64, ...; a __ballot of mismatches ends a candidate, the first candidate verified ends
// the pair: nothing behind the lowest hit is read.  Lane 0 stores the answer.  No atomics.
//
// Worst case: periodic text makes every start a candidate -- a homopolymer reference against a needle that differs in
// its last base -- and every candidate costs ceil(n / 64) verify steps before it fails: at most
// (R - n + 1) * ceil(n / 64) <= R * ceil(n / 64) steps per pair (contain_worst_steps), 9 000 for a 16S reference and a
// needle of half its length.  Memory: a pair reads at most 4 R bytes of the reference once per sweep; the verify's
// reads repeat out of the vector L1.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "ctx.h"
#include "contain_plan.h"

namespace sina_hip {
namespace {

struct ContainArgs {
    const uint32_t *ref_ab;   // the store's packed references
    const uint64_t *ref_off;
    const uint32_t *q_words;  // the call's queries, packed (contain_pack_query) ...
    const uint64_t *qw_off;   // ... query q's words at q_words + qw_off[q] ...
    const uint32_t *q_n;      // ... and its number of bases
    const uint32_t *ids;      // the range's pairs: the reference ...
    const uint32_t *pair_q;   // ... and the query of pair p
    uint32_t *out;            // [n_pairs]
    uint32_t n_pairs, n_refs;
};

// the value of virtual lane `lane + d` of a row of 128: x on lanes 0 .. 63, y behind them
__device__ __forceinline__ uint32_t row_down(uint32_t x, uint32_t y, int lane, int d) {
    const int src = (lane + d) & 63;
    const uint32_t xs = __shfl(x, src), ys = __shfl(y, src);
    return lane + d < 64 ? xs : ys;
}

__global__ void __launch_bounds__(kContainThreads) find_bases_kernel(ContainArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t pair = blockIdx.x * kContainPairsPerWg + (threadIdx.x >> 6);
    if (pair >= a.n_pairs) return;  // (the whole wave)
    const uint32_t qi = a.pair_q[pair], id = a.ids[pair];
    const uint32_t n = a.q_n[qi];
    const uint32_t *qw = a.q_words + a.qw_off[qi];
    uint32_t result = kContainNone;
    if (id < a.n_refs && n >= 1) {  // (the entry checked both)
        const uint64_t r0 = a.ref_off[id];
        const uint32_t R = (uint32_t)(a.ref_off[id + 1] - r0);
        const uint32_t *ref = a.ref_ab + r0;
        if (n <= R) {
            const uint32_t last = R - n;  // the last start
            const uint32_t kmask = contain_key_mask(n);
            const uint32_t qkey = qw[0] & kmask;
            for (uint32_t chunk = 0; chunk <= last && result == kContainNone; chunk += 64) {
                // codes of positions chunk + lane (x) and, on lanes 0 .. 6, chunk + 64 + lane (y); 0 past the end
                const uint32_t p0 = chunk + lane, p1 = chunk + 64 + lane;
                const uint32_t x1 = p0 < R ? (ref[p0] >> 24) & 0xFu : 0u;
                const uint32_t y1 = (lane < 7 && p1 < R) ? (ref[p1] >> 24) & 0xFu : 0u;
                // two, four, eight codes from the lane's position on: code j in bits 4j .. 4j + 3
                const uint32_t x2 = x1 | (row_down(x1, y1, lane, 1) << 4);
                const uint32_t y2 = y1 | (__shfl(y1, (lane + 1) & 63) << 4);  // (lanes 0 .. 5 count)
                const uint32_t x4 = x2 | (row_down(x2, y2, lane, 2) << 8);
                const uint32_t y4 = y2 | (__shfl(y2, (lane + 2) & 63) << 8);  // (lanes 0 .. 3 count)
                const uint32_t x8 = x4 | (row_down(x4, y4, lane, 4) << 16);
                unsigned long long cand = __ballot(p0 <= last && (x8 & kmask) == qkey);
                while (cand != 0) {  // (the same for every lane)
                    const uint32_t start = chunk + (uint32_t)(__ffsll((long long)cand) - 1);
                    cand &= cand - 1;
                    bool hit = true;
                    if (n > kContainKeyBases)  // (start + j <= last + n - 1 = R - 1)
                        for (uint32_t j0 = 0; j0 < n; j0 += 64) {
                            const uint32_t j = j0 + lane;
                            bool differs = false;
                            if (j < n) differs = ((qw[j >> 3] >> (4 * (j & 7))) & 0xFu) != ((ref[start + j] >> 24) & 0xFu);
                            if (__ballot(differs) != 0) {
                                hit = false;
                                break;
                            }
                        }
                    if (hit) {
                        result = start;
                        break;
                    }
                }
            }
        }
    }
    if (lane == 0) a.out[pair] = result;
}

}  // namespace
}  // namespace sina_hip

using namespace sina_hip;

extern "C" int sina_hip_find_bases(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *q_off, uint32_t nq, const uint32_t *cand_ids,
                                    const uint64_t *cand_off, uint32_t *out_at) {
    if (!c || !qmask || !q_off || !cand_ids || !cand_off || !out_at) SH_FAIL("find_bases: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    sina_hip_hint_guard hints(c);
    if (!c->st->have_refs) SH_FAIL("find_bases: upload references first");
    if (test_knob("contain_fail") == "1") SH_FAIL("find_bases: refused by the test knob contain_fail");
    if (nq == 0) return 0;
    for (uint32_t q = 0; q < nq; q++) {
        if (cand_off[q + 1] < cand_off[q]) SH_FAIL("find_bases: candidate offsets descend");
        if (q_off[q + 1] < q_off[q]) SH_FAIL("find_bases: query offsets descend");
        if (q_off[q + 1] == q_off[q]) SH_FAIL("find_bases: query of 0 bases");
        if (q_off[q + 1] - q_off[q] > kContainMaxBases) SH_FAIL("find_bases: query longer than 65535 bases");
    }
    const uint64_t n_pairs = cand_off[nq] - cand_off[0];
    for (uint64_t i = 0; i < n_pairs; i++)
        if (cand_ids[cand_off[0] + i] >= c->st->n_refs) SH_FAIL("find_bases: reference id out of range");
    if (n_pairs == 0) return 0;
    SH_CHECK(hipSetDevice(c->device));
    // the queries, packed: every query on words of its own
    std::vector<uint64_t> qw_off((size_t)nq + 1, 0);
    std::vector<uint32_t> q_n(nq);
    for (uint32_t q = 0; q < nq; q++) {
        q_n[q] = (uint32_t)(q_off[q + 1] - q_off[q]);
        qw_off[q + 1] = qw_off[q] + contain_query_words(q_n[q]);
    }
    std::vector<uint32_t> q_words((size_t)qw_off[nq]);
    for (uint32_t q = 0; q < nq; q++) contain_pack_query(qmask + q_off[q], q_n[q], q_words.data() + qw_off[q]);
    // the query of every pair
    std::vector<uint32_t> pair_q((size_t)n_pairs);
    for (uint32_t q = 0; q < nq; q++)
        std::fill(pair_q.begin() + (size_t)(cand_off[q] - cand_off[0]), pair_q.begin() + (size_t)(cand_off[q + 1] - cand_off[0]), q);
    const uint32_t *const ids = cand_ids + cand_off[0];
    const hipStream_t s = c->stream;
    if (c->s_qab.reserve(4 * q_words.size()) || c->s_qoff.reserve(8 * ((uint64_t)nq + 1)) || c->m_n.reserve(4 * (uint64_t)nq)) return 1;
    if (upload(c, 1, c->s_qab.p, q_words.data(), 4 * q_words.size(), s) || upload(c, 2, c->s_qoff.p, qw_off.data(), 8 * ((uint64_t)nq + 1), s) ||
        upload(c, 3, c->m_n.p, q_n.data(), 4 * (uint64_t)nq, s))
        return 1;
    // (SINA_HIP_TEST=contain_pairs=N: launch ranges of N pairs, so that a small call takes several)
    const std::string range_knob = test_knob("contain_pairs");
    const uint64_t max_pairs = range_knob.empty() ? kContainRangePairs : std::max<uint64_t>(1, strtoull(range_knob.c_str(), nullptr, 10));
    const bool have_off = ensure_ref_off_host(c) == 0;
    // (answers through a vector of the call's own: out_at stays untouched if a launch fails)
    std::vector<uint32_t> got((size_t)n_pairs);
    for (const ContainRange &r : contain_ranges(n_pairs, max_pairs)) {
        const uint64_t np = r.p1 - r.p0;
        if (c->s_cand.reserve(contain_pair_bytes(np)) || c->s_coff.reserve(contain_pair_bytes(np)) || c->s_out.reserve(contain_pair_bytes(np)))
            return 1;
        if (upload(c, 4, c->s_cand.p, ids + r.p0, contain_pair_bytes(np), s) ||
            upload(c, 6, c->s_coff.p, pair_q.data() + r.p0, contain_pair_bytes(np), s))
            return 1;
        ContainArgs a;
        a.ref_ab = c->st->ref_ab.as<uint32_t>();
        a.ref_off = c->st->ref_off.as<uint64_t>();
        a.q_words = c->s_qab.as<uint32_t>();
        a.qw_off = c->s_qoff.as<uint64_t>();
        a.q_n = c->m_n.as<uint32_t>();
        a.ids = c->s_cand.as<uint32_t>();
        a.pair_q = c->s_coff.as<uint32_t>();
        a.out = c->s_out.as<uint32_t>();
        a.n_pairs = (uint32_t)np;
        a.n_refs = c->st->n_refs;
        // (a thin kernel beside whatever is resident: on the context's own stream, like the show-dist kernel -- ctx.h)
        SH_CHECK(hipEventRecord(c->ev[6], s));
        hipLaunchKernelGGL(find_bases_kernel, dim3(contain_grid((uint32_t)np)), dim3(kContainThreads), 0, s, a);
        SH_CHECK(hipGetLastError());
        SH_CHECK(hipEventRecord(c->ev[7], s));
        if (download(c, 5, c->s_out.p, contain_pair_bytes(np), s)) return 1;
        SH_CHECK(wait_stream(c, s));
        float ms = 0;
        SH_CHECK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
        memcpy(got.data() + r.p0, c->h_stage[5].p, contain_pair_bytes(np));
        uint64_t bases = 0;
        if (have_off)
            for (uint64_t p = r.p0; p < r.p1; p++) bases += c->st->ref_off_host[ids[p] + 1] - c->st->ref_off_host[ids[p]];
        c->use[kUseContain].add(ms, np, bases, 1);
    }
    memcpy(out_at + cand_off[0], got.data(), 4 * got.size());
    return 0;
}

extern "C" int sina_hip_find_bases_stats(sina_hip_ctx *c, double *kernel_ms, uint64_t *pairs, uint64_t *ref_bases, uint64_t *launches) {
    if (!c || !kernel_ms || !pairs || !ref_bases || !launches) SH_FAIL("find_bases_stats: null argument");
    return read_use(c, kUseContain, kernel_ms, pairs, ref_bases, launches);
}
