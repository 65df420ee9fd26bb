// --show-dist on the GPU: show_dist_kernel + sina_hip_show_dist, sina_hip_show_dist_stats.  The tables
// and the classification are compare_dev.h's, shared with search.hip, rank.hip and identity.hip; the kernel's counters
// are the context's use[kUseShowDist].
//
// What it computes: the counters behind Log::printer::show_dist (src/log.cpp:279-325) for a query that arrived aligned:
// its input alignment `orig` against its finished alignment `aligned` (self, CMP_IUPAC_EXACT), `orig` against every
// member of its list of relatives (CMP_IUPAC_OPTIMISTIC) to find the closest -- what std::sort by
// result_item::operator< puts last: the largest score (float)match / denom under CMP_COVER_QUERY, equal scores by the
// reference's name --, and `aligned` against that closest relative.  A score is never negative, so it orders like its
// bit pattern; a key is (score bits << 32 | rank of the name), as in rank.hip.  A member with denom == 0 (the host's
// NaN) is left out and raises the row's flag: the caller walks that query itself.  The floats stay with the host.
//
// How it maps to the hardware: one workgroup of kCT threads per query.  Phase A builds orig's column bitmap, running
// counts and mask bytes in LDS (build_query_tables), then the four waves stride over the list's members and, one place
// behind the last member, `aligned`: each streams one sequence's packed words from HBM against the tables
// (classify_candidate) and keeps its best member's key, id and counters in registers.  The waves meet in LDS, the
// largest key wins.  Phase B builds the tables again, over `aligned` -- all of them: orig has bases in columns that
// aligned has not --, and one wave streams the winner.  Thread 0 stores the twenty words.  HBM-bound like its
// neighbours: 4 B x (sum of the members' lengths + the winner's again) in, 80 bytes out.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "ctx.h"
#include "compare_dev.h"
#include "showdist_plan.h"

namespace sina_hip {
namespace {

static_assert(kShowDistThreads == (uint32_t)kCT, "showdist_plan.h and compare_dev.h disagree on the workgroup");
static_assert(kShowDistMaxLds == kCompareMaxLds, "showdist_plan.h and compare_dev.h disagree on the LDS ceiling");
static_assert(show_dist_lds_bytes(1, 1, 0) == compare_table_bytes(1, 1) && show_dist_lds_bytes(33, 5, 17) == compare_table_bytes(33, 17) &&
                  show_dist_lds_bytes(524288, 65535, 10240) == compare_table_bytes(524288, 65535),
              "showdist_plan.h and compare_dev.h disagree on the tables' size");
static_assert(sizeof(sina_hip_match_counts) == 24, "a set of counters is six words of the row");

struct ShowDistArgs {
    const uint32_t *ref_ab;     // the store's packed references
    const uint64_t *ref_off;
    const uint32_t *q_ab;       // the range's packed words: every orig, then every aligned
    const uint64_t *o_off;      // [n + 1] orig of query q at q_ab + o_off[q]
    const uint64_t *a_off;      // [n + 1] aligned of query q at q_ab + a_off[q]
    const uint32_t *ids;        // the range's lists, concatenated ...
    const uint64_t *l_off;      // ... [n + 1]
    const uint32_t *name_rank;  // [n_refs] position of the reference's name in ascending order
    uint32_t *rows;             // [n][kShowDistRowWords]
    uint32_t n, width, n_refs;
};

__device__ __forceinline__ void store_counts(uint32_t *dst, const sina_hip_match_counts &m) {
    dst[0] = (uint32_t)m.only_a_overhang;
    dst[1] = (uint32_t)m.only_b_overhang;
    dst[2] = (uint32_t)m.only_a;
    dst[3] = (uint32_t)m.only_b;
    dst[4] = (uint32_t)m.match;
    dst[5] = (uint32_t)m.mismatch;
}

__global__ void __launch_bounds__(kCT) show_dist_kernel(ShowDistArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_tmp[8];
    __shared__ uint32_t s_scal[3];
    // a stored key is the key plus one: 0 says that the wave kept no member (rank.hip)
    __shared__ uint64_t s_key[kCT / 64];
    __shared__ uint32_t s_id[kCT / 64], s_nan[kCT / 64];
    __shared__ uint32_t s_cnt[kCT / 64][6];
    __shared__ uint32_t s_self[6];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    if (q >= a.n) return;
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t *orig = a.q_ab + a.o_off[q], *al = a.q_ab + a.a_off[q];
    const uint32_t lo = (uint32_t)(a.o_off[q + 1] - a.o_off[q]), la = (uint32_t)(a.a_off[q + 1] - a.a_off[q]);
    const uint64_t m0 = a.l_off[q];
    const uint32_t nm = (uint32_t)(a.l_off[q + 1] - m0);

    // ---- phase A: orig's tables; the members and, one place behind them, aligned (show-dist filters no lower case)
    uint64_t best = 0;
    uint32_t best_id = kShowDistNone, nan = 0;
    sina_hip_match_counts best_m{};
    {
        const QueryTables t = build_query_tables(smem, s_tmp, s_scal, orig, lo, a.width, 0u);
        for (uint32_t x = wave; x <= nm; x += kCT / 64) {
            if (x == nm) {  // (the whole wave)
                const sina_hip_match_counts m = classify_candidate(t, al, la, true, 0u, SINA_CMP_IUPAC_EXACT, lane);
                if (lane == 0) store_counts(s_self, m);
                continue;
            }
            const uint32_t id = a.ids[m0 + x];
            const bool valid = id < a.n_refs;  // (the entry checked the ids)
            const uint32_t *Bp = valid ? a.ref_ab + a.ref_off[id] : nullptr;
            const uint32_t lb = valid ? (uint32_t)(a.ref_off[id + 1] - a.ref_off[id]) : 0u;
            const sina_hip_match_counts m = classify_candidate(t, Bp, lb, valid, 0u, SINA_CMP_IUPAC_OPTIMISTIC, lane);
            if (!valid) continue;
            const int32_t denom = cover_denominator(m, SINA_CMP_COVER_QUERY);  // (cseq_comparator::score: compare_dev.h)
            if (denom == 0) {  // the host's 0 / 0
                nan = 1;
                continue;
            }
            const float score = __fdiv_rn((float)m.match, (float)denom);
            const uint64_t stored = (((uint64_t)__float_as_uint(score) << 32) | a.name_rank[id]) + 1;
            if (stored > best) {  // (an equal key is the same reference again: the same counters)
                best = stored;
                best_id = id;
                best_m = m;
            }
        }
    }
    // (every lane of a wave holds the wave's values: classify_candidate reduces across lanes)
    if (lane == 0) {
        s_key[wave] = best;
        s_id[wave] = best_id;
        s_nan[wave] = nan;
        store_counts(s_cnt[wave], best_m);
    }
    __syncthreads();  // ... and every wave is done with orig's tables
    int win = 0;
    for (int w = 1; w < kCT / 64; w++)
        if (s_key[w] > s_key[win]) win = w;
    const bool have = s_key[win] != 0;  // (the same for every thread of the workgroup)
    const uint32_t closest = have ? s_id[win] : kShowDistNone;

    // ---- phase B: aligned's tables, all of them again; one wave streams the winner
    sina_hip_match_counts after{};
    if (have) {
        const QueryTables t = build_query_tables(smem, s_tmp, s_scal, al, la, a.width, 0u);
        if (wave == 0) {
            const uint32_t *Bp = a.ref_ab + a.ref_off[closest];
            const uint32_t lb = (uint32_t)(a.ref_off[closest + 1] - a.ref_off[closest]);
            after = classify_candidate(t, Bp, lb, true, 0u, SINA_CMP_IUPAC_OPTIMISTIC, lane);
        }
    }
    if (tid == 0) {
        uint32_t *row = a.rows + (size_t)q * kShowDistRowWords;
        uint32_t flags = kShowDistFlagComputed;
        for (int w = 0; w < kCT / 64; w++) flags |= s_nan[w] ? kShowDistFlagNan : 0u;
        for (int i = 0; i < 6; i++) {
            row[kShowDistSelf + i] = s_self[i];
            row[kShowDistBefore + i] = have ? s_cnt[win][i] : 0u;
        }
        store_counts(row + kShowDistAfter, after);
        row[kShowDistClosest] = closest;
        row[kShowDistFlags] = flags;
    }
}

}  // namespace
}  // namespace sina_hip

using namespace sina_hip;

extern "C" int sina_hip_show_dist(sina_hip_ctx *c, const uint32_t *orig_ab, const uint64_t *orig_off, const uint32_t *al_ab,
                                   const uint64_t *al_off, uint32_t nq, const uint32_t *ref_ids, const uint64_t *ref_off, uint32_t *rows) {
    if (!c) SH_FAIL("show_dist: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    sina_hip_hint_guard hints(c);
    if (nq == 0) return 0;
    if (!orig_ab || !orig_off || !al_ab || !al_off || !ref_off || !rows) SH_FAIL("show_dist: null argument");
    if (!c->st->have_refs) SH_FAIL("show_dist: upload references first");
    if (!c->st->have_name_order) SH_FAIL("show_dist: upload the name order first");
    for (uint32_t q = 0; q < nq; q++) {
        if (ref_off[q + 1] < ref_off[q]) SH_FAIL("show_dist: list offsets descend");
        if (ref_off[q + 1] - ref_off[q] > 0x7FFFFFFFull) SH_FAIL("show_dist: list longer than 2^31 - 1 ids");
    }
    const uint64_t pairs_all = ref_off[nq] - ref_off[0];
    if (pairs_all != 0 && !ref_ids) SH_FAIL("show_dist: null argument");
    for (uint64_t i = 0; i < pairs_all; i++)
        if (ref_ids[ref_off[0] + i] >= c->st->n_refs) SH_FAIL("show_dist: reference id out of range");
    if (match_check_queries("show_dist (orig)", orig_ab, orig_off, nq) || match_check_queries("show_dist (aligned)", al_ab, al_off, nq))
        return 1;
    uint32_t max_lo = 0, max_la = 0;
    for (uint32_t q = 0; q < nq; q++) {
        max_lo = std::max<uint32_t>(max_lo, (uint32_t)(orig_off[q + 1] - orig_off[q]));
        max_la = std::max<uint32_t>(max_la, (uint32_t)(al_off[q + 1] - al_off[q]));
    }
    const size_t lds = show_dist_lds_bytes(c->st->width, max_lo, max_la);
    if (lds > kShowDistMaxLds) SH_FAIL_LIMIT("show_dist: alignment too wide for the device comparison");
    SH_CHECK(hipSetDevice(c->device));
    if (allow_full_lds(reinterpret_cast<const void *>(show_dist_kernel))) return 1;
    const hipStream_t s = c->stream;
    // (SINA_HIP_TEST=showdist_range=N: launch ranges of N queries, so that a small call takes several)
    const std::string range_knob = test_knob("showdist_range");
    const uint32_t max_queries =
        range_knob.empty() ? kShowDistRangeQueries : std::max<uint32_t>(1, (uint32_t)strtoul(range_knob.c_str(), nullptr, 10));
    // (results through a vector of the call's own: rows stay untouched if a launch fails)
    std::vector<uint32_t> got((size_t)nq * kShowDistRowWords);
    std::vector<uint64_t> rel, lrel;
    for (const ShowDistRange &r : show_dist_ranges(orig_off, al_off, ref_off, nq, kShowDistRangeWords, max_queries)) {
        const uint32_t n = r.q1 - r.q0;
        const uint64_t wo = orig_off[r.q1] - orig_off[r.q0], wa = al_off[r.q1] - al_off[r.q0];
        const uint64_t nl = ref_off[r.q1] - ref_off[r.q0];
        rel.resize(2 * ((size_t)n + 1));
        lrel.resize((size_t)n + 1);
        for (uint32_t q = 0; q <= n; q++) {
            rel[q] = orig_off[r.q0 + q] - orig_off[r.q0];
            rel[(size_t)n + 1 + q] = wo + (al_off[r.q0 + q] - al_off[r.q0]);
            lrel[q] = ref_off[r.q0 + q] - ref_off[r.q0];
        }
        if (c->s_qab.reserve(4 * std::max<uint64_t>(wo + wa, 1)) || c->s_qoff.reserve(16 * ((uint64_t)n + 1)) ||
            c->s_cand.reserve(4 * std::max<uint64_t>(nl, 1)) || c->s_coff.reserve(8 * ((uint64_t)n + 1)) ||
            c->s_out.reserve(show_dist_row_bytes(n)))
            return 1;
        if (upload(c, 1, c->s_qab.p, orig_ab + orig_off[r.q0], 4 * wo, s) ||
            upload(c, 6, c->s_qab.as<uint32_t>() + wo, al_ab + al_off[r.q0], 4 * wa, s) ||
            upload(c, 2, c->s_qoff.p, rel.data(), 16 * ((uint64_t)n + 1), s) ||
            upload(c, 3, c->s_cand.p, nl ? ref_ids + ref_off[r.q0] : nullptr, 4 * nl, s) ||
            upload(c, 4, c->s_coff.p, lrel.data(), 8 * ((uint64_t)n + 1), s))
            return 1;
        ShowDistArgs a;
        a.ref_ab = c->st->ref_ab.as<uint32_t>();
        a.ref_off = c->st->ref_off.as<uint64_t>();
        a.q_ab = c->s_qab.as<uint32_t>();
        a.o_off = c->s_qoff.as<uint64_t>();
        a.a_off = c->s_qoff.as<uint64_t>() + n + 1;
        a.ids = c->s_cand.as<uint32_t>();
        a.l_off = c->s_coff.as<uint64_t>();
        a.name_rank = c->st->name_rank.as<uint32_t>();
        a.rows = c->s_out.as<uint32_t>();
        a.n = n;
        a.width = c->st->width;
        a.n_refs = c->st->n_refs;
        // (a thin kernel beside whatever is resident: on the context's own stream, like the pair count -- ctx.h)
        SH_CHECK(hipEventRecord(c->ev[6], s));
        hipLaunchKernelGGL(show_dist_kernel, dim3(show_dist_grid(n)), dim3(kCT), lds, s, a);
        SH_CHECK(hipGetLastError());
        SH_CHECK(hipEventRecord(c->ev[7], s));
        if (download(c, 5, c->s_out.p, show_dist_row_bytes(n), s)) return 1;
        SH_CHECK(wait_stream(c, s));
        float ms = 0;
        SH_CHECK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
        memcpy(got.data() + (size_t)r.q0 * kShowDistRowWords, c->h_stage[5].p, show_dist_row_bytes(n));
        c->use[kUseShowDist].add(ms, n, nl, 1);
    }
    memcpy(rows, got.data(), 4 * got.size());
    return 0;
}

extern "C" int sina_hip_show_dist_stats(sina_hip_ctx *c, double *kernel_ms, uint64_t *sequences, uint64_t *pairs, uint64_t *launches) {
    if (!c || !kernel_ms || !sequences || !pairs || !launches) SH_FAIL("show_dist_stats: null argument");
    return read_use(c, kUseShowDist, kernel_ms, sequences, pairs, launches);
}
