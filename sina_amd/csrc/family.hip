// Famfinder's filter cascade on the GPU: family_meta_kernel, family_cascade_kernel, their launcher
// and sina_hip_family_cascade.
//
// What it computes: match_pass of host/famfinder.cpp (src/famfinder.cpp:497-612), restated -- for every query the
// candidates of its ranked list that the cascade keeps, in the list's order, and whether the cascade has enough.
// A query's row is 2 + 2 K words (family_plan.h): the number kept, flags, K ids, K score bit patterns.
//
// How it maps to the hardware: one wave per query, 64 candidates per step.  A lane loads its candidate's id, score and
// match count (coalesced) and its reference's three meta words (one 12-byte record of the store's table) and evaluates
// the tests that need no state.  Six ballots turn them into 64-bit masks; the stateful part -- four counters and the
// quota tests -- is a loop over the set bits of the eligible mask in scalar registers.  While fs_min is not reached the
// next fs_min - have eligible candidates are kept in one step (a lane's rank among the eligible, one more ballot).
// The kept mask tells every kept lane its place in the row.  The loop over steps ends at the list's end or where
// nothing more can be kept (every quota met): latency-bound, a few hundred bytes per step.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "ctx.h"
#include "family_plan.h"
#include "match_plan.h"

namespace sina_hip {
namespace {

constexpr int kFT = 64 * (int)kFamilyWavesPerWg;  // threads per workgroup

// size, first and last column of every reference, as reference_store::ref_meta has them (a reference without bases:
// three zeros)
__global__ void family_meta_kernel(const uint32_t *ref_ab, const uint64_t *ref_off, uint32_t n_refs, uint32_t *meta) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_refs) return;
    const uint64_t b = ref_off[id], e = ref_off[id + 1];
    meta[3 * (size_t)id] = (uint32_t)(e - b);
    meta[3 * (size_t)id + 1] = e > b ? ref_ab[b] & 0xFFFFFFu : 0u;
    meta[3 * (size_t)id + 2] = e > b ? ref_ab[e - 1] & 0xFFFFFFu : 0u;
}

struct FamilyArgs {
    const uint32_t *meta;      // [n_refs][3]
    const uint32_t *ids;       // [nq][stride]
    const float *scores;       // [nq][stride]
    const uint16_t *match;     // [nq][stride]; null: no identity test (fs_msc_max >= 1)
    const uint32_t *n;         // [nq] candidates of the query; 0xFFFFFFFF (the candidate-list path's overflow mark) = 0
    const uint64_t *q_off;     // [nq + 1] the queries' base counts as differences
    const uint32_t *self_ids;  // the queries' self lists at self_off[q] .. self_off[q + 1]; null: no leave-out
    const uint64_t *self_off;
    uint32_t *rows;            // [nq][2 + 2 K], zeroed
    unsigned long long *scanned;  // candidates the steps covered, summed over the launch
    uint32_t nq, stride, n_refs, K;
    uint32_t fs_min, fs_max, fs_req_full, fs_full_len, fs_min_len, fs_cover_gene;
    float fs_msc, fs_msc_max;
};

__global__ void __launch_bounds__(kFT) family_cascade_kernel(FamilyArgs a) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * kFamilyWavesPerWg + wave;
    if (q >= a.nq) return;
    uint32_t n = a.n[q];
    if (n == 0xFFFFFFFFu) n = 0;
    if (n > a.stride) n = a.stride;
    const uint32_t query_bases = (uint32_t)(a.q_off[q + 1] - a.q_off[q]);
    const uint64_t s0 = a.self_ids ? a.self_off[q] : 0, s1 = a.self_ids ? a.self_off[q + 1] : 0;
    const uint32_t *ids = a.ids + (size_t)q * a.stride;
    const float *scores = a.scores + (size_t)q * a.stride;
    const uint16_t *match = a.match ? a.match + (size_t)q * a.stride : nullptr;
    uint32_t *row = a.rows + (size_t)q * family_row_words(a.K);
    const uint32_t range_begin = 0, range_end = 0;
    const uint32_t need = max(a.fs_min, a.fs_max);
    const uint64_t below = (1ull << lane) - 1;  // the lanes before mine

    // the cascade's state: wave-uniform, out of ballots and kernel arguments only
    uint32_t have = 0, have_full = 0, have_left = 0, have_right = 0, scanned = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        // nothing more can be kept: min and max reached, every quota met
        if (have >= need && have_full >= a.fs_req_full && have_left >= a.fs_cover_gene && have_right >= a.fs_cover_gene) break;
        const uint32_t i = base + lane;
        const bool in = i < n;
        uint32_t id = 0, mt = 0;
        float sc = 0.f;
        if (in) {
            id = ids[i];
            sc = scores[i];
            if (match) mt = match[i];
        }
        const bool known = in && id < a.n_refs;
        uint32_t size = 0, first_pos = 0, last_pos = 0;
        if (known) {
            const uint32_t *m = a.meta + 3 * (size_t)id;
            size = m[0];
            first_pos = m[1];
            last_pos = m[2];
        }
        bool eligible = known && size >= a.fs_min_len;
        for (uint64_t s = s0; s < s1; s++) eligible = eligible && id != a.self_ids[s];
        if (match) {
            const float identity = query_bases ? __fdiv_rn((float)mt, (float)query_bases) : 0.f;
            eligible = eligible && !(identity > a.fs_msc_max);
        }
        const uint64_t m_eligible = __ballot(eligible), m_full = __ballot(size >= a.fs_full_len),
                       m_left = __ballot(size && first_pos <= range_begin), m_right = __ballot(size && last_pos >= range_end),
                       m_good = __ballot(sc < a.fs_msc) /* sic */, m_past = __ballot(!in);

        const uint32_t have_before = have;
        uint64_t kept = 0, rest = m_eligible;
        if (have < a.fs_min) {  // below fs_min every eligible candidate is kept: the next fs_min - have of them at once
            const uint32_t rank = (uint32_t)__popcll(m_eligible & below);
            kept = __ballot(eligible && rank < a.fs_min - have);
            rest = m_eligible & ~kept;
            have += (uint32_t)__popcll(kept);
            if (a.fs_req_full) have_full += (uint32_t)__popcll(kept & m_full);
            if (a.fs_cover_gene) {
                have_right += (uint32_t)__popcll(kept & m_right);
                have_left += (uint32_t)__popcll(kept & m_left);
            }
        }
        while (rest) {
            if (have >= need && have_full >= a.fs_req_full && have_left >= a.fs_cover_gene && have_right >= a.fs_cover_gene) break;
            const uint32_t b = (uint32_t)__builtin_ctzll(rest);
            rest &= rest - 1;
            const bool is_full = (m_full >> b) & 1, is_left = (m_left >> b) & 1, is_right = (m_right >> b) & 1;
            const bool score_good = (m_good >> b) & 1;
            const bool min_reached = have >= a.fs_min, max_reached = have >= a.fs_max;
            const bool adds_to_full = a.fs_req_full && have_full < a.fs_req_full && is_full;
            const bool adds_to_range = (a.fs_cover_gene && have_right < a.fs_cover_gene && is_right) ||
                                       (a.fs_cover_gene && have_left < a.fs_cover_gene && is_left);
            if (min_reached && (max_reached || !score_good) && !adds_to_full && !adds_to_range) continue;
            kept |= 1ull << b;
            ++have;
            if (a.fs_req_full && is_full) ++have_full;
            if (a.fs_cover_gene && is_right) ++have_right;
            if (a.fs_cover_gene && is_left) ++have_left;
        }
        if ((kept >> lane) & 1) {
            const uint32_t at = have_before + (uint32_t)__popcll(kept & below);
            if (at < a.K) {  // (always: have <= K)
                row[2 + at] = id;
                row[2 + a.K + at] = __float_as_uint(sc);
            }
        }
        scanned += 64u - (uint32_t)__popcll(m_past);
    }
    if (lane == 0) {
        const bool enough = !(have < a.fs_max || have_full < a.fs_req_full || have_left < a.fs_cover_gene || have_right < a.fs_cover_gene);
        row[0] = have;
        row[1] = (enough ? kFamilyFlagEnough : 0u) | (n == 0 ? kFamilyFlagEmpty : 0u);
        if (scanned) atomicAdd(a.scanned, (unsigned long long)scanned);
    }
}

// the store's meta table, built once per store content by whichever context gets here first
int ensure_family_meta(sina_hip_ctx *c) {
    sina_hip_store *st = c->st;
    if (st->fam_meta_ready.load(std::memory_order_acquire)) return 0;
    std::lock_guard<std::mutex> lk(st->aux_mu);
    if (st->fam_meta_ready.load(std::memory_order_relaxed)) return 0;
    if (st->fam_meta.reserve_exact(12 * std::max<uint64_t>(st->n_refs, 1))) return 1;
    if (st->n_refs) {
        hipLaunchKernelGGL(family_meta_kernel, dim3((st->n_refs + 255) / 256), dim3(256), 0, c->stream, st->ref_ab.as<uint32_t>(),
                           st->ref_off.as<uint64_t>(), st->n_refs, st->fam_meta.as<uint32_t>());
        SH_CHECK(hipGetLastError());
        SH_CHECK(hipStreamSynchronize(c->stream));
    }
    st->fam_meta_ready.store(true, std::memory_order_release);
    return 0;
}

}  // namespace

int family_rule_plan(const char *who, const sina_hip_family_rule *r, uint32_t nq, FamilyPlan *plan) {
    *plan = family_plan(r->fs_min, r->fs_max, r->fs_req_full, r->fs_cover_gene, nq);
    if (!plan->ok) SH_FAIL_LIMIT(std::string(who) + ": the rule allows a family of more than 1024 entries (kFamilyCascadeMaxK)");
    return 0;
}

void family_empty_row(const sina_hip_family_rule *r, uint32_t row_words, uint32_t *row) {
    memset(row, 0, 4 * (size_t)row_words);
    const bool enough = !(0 < r->fs_max || 0 < r->fs_req_full || 0 < r->fs_cover_gene);
    row[1] = (enough ? kFamilyFlagEnough : 0u) | kFamilyFlagEmpty;
}

int family_launch(sina_hip_ctx *c, const uint32_t *d_ids, const float *d_scores, const uint16_t *d_match, const uint32_t *d_n,
                  uint32_t stride, const uint64_t *d_qoff, uint32_t nq, const sina_hip_family_rule *r, const FamilyPlan &plan,
                  const uint32_t *d_self_ids, const uint64_t *d_self_off, const uint32_t *h_n, uint32_t *out_rows) {
    if (nq == 0) return 0;
    if (ensure_family_meta(c)) return 1;
    hipStream_t s = c->stream;
    const size_t row_bytes = 4 * (size_t)plan.row_words * nq;
    if (c->f_rows.reserve(row_bytes) || c->f_cnt.reserve(8)) return 1;
    SH_CHECK(hipMemsetAsync(c->f_rows.p, 0, row_bytes, s));
    SH_CHECK(hipMemsetAsync(c->f_cnt.p, 0, 8, s));
    FamilyArgs a;
    a.meta = c->st->fam_meta.as<uint32_t>();
    a.ids = d_ids;
    a.scores = d_scores;
    a.match = r->fs_msc_max < 1 ? d_match : nullptr;
    a.n = d_n;
    a.q_off = d_qoff;
    a.self_ids = d_self_ids;
    a.self_off = d_self_off;
    a.rows = c->f_rows.as<uint32_t>();
    a.scanned = c->f_cnt.as<unsigned long long>();
    a.nq = nq;
    a.stride = stride;
    a.n_refs = c->st->n_refs;
    a.K = plan.K;
    a.fs_min = r->fs_min;
    a.fs_max = r->fs_max;
    a.fs_req_full = r->fs_req_full;
    a.fs_full_len = r->fs_full_len;
    a.fs_min_len = r->fs_min_len;
    a.fs_cover_gene = r->fs_cover_gene;
    a.fs_msc = r->fs_msc;
    a.fs_msc_max = r->fs_msc_max;
    SH_CHECK(hipEventRecord(c->ev[6], s));
    hipLaunchKernelGGL(family_cascade_kernel, dim3(plan.grid), dim3(kFT), 0, s, a);
    SH_CHECK(hipGetLastError());
    SH_CHECK(hipEventRecord(c->ev[7], s));
    if (download(c, 9, c->f_rows.p, row_bytes, s) || download(c, 10, c->f_cnt.p, 8, s)) return 1;
    SH_CHECK(wait_stream(c, s));
    float ms = 0;
    SH_CHECK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
    memcpy(out_rows, c->h_stage[9].p, row_bytes);
    unsigned long long scanned = 0;
    memcpy(&scanned, c->h_stage[10].p, 8);
    uint64_t listed = 0;
    for (uint32_t q = 0; q < nq; q++) listed += h_n[q] == 0xFFFFFFFFu ? 0u : std::min(h_n[q], stride);
    c->use[kUseFamily].add(ms, listed, scanned, 1, nq);
    return 0;
}

int family_check_self(const char *who, sina_hip_ctx *c, const uint32_t *self_ids, const uint64_t *self_off, uint32_t nq) {
    if (!self_ids) return 0;
    for (uint32_t q = 0; q < nq; q++)
        if (self_off[q + 1] < self_off[q]) SH_FAIL(std::string(who) + ": self offsets descend");
    for (uint64_t i = self_off[0]; i < self_off[nq]; i++)
        if (self_ids[i] >= c->st->n_refs) SH_FAIL(std::string(who) + ": self id out of range");
    return 0;
}

}  // namespace sina_hip

using namespace sina_hip;

extern "C" int sina_hip_family_row_words(const sina_hip_family_rule *r, uint32_t *words) {
    if (!r || !words) SH_FAIL("family_row_words: null argument");
    FamilyPlan plan;
    if (family_rule_plan("family_row_words", r, 0, &plan)) return 1;
    *words = plan.row_words;
    return 0;
}

extern "C" int sina_hip_family_cascade(sina_hip_ctx *c, const uint32_t *cand_ids, const float *cand_scores, const uint16_t *cand_match,
                                        const uint64_t *cand_off, const uint32_t *q_bases, uint32_t nq, const sina_hip_family_rule *r,
                                        const uint32_t *self_ids, const uint64_t *self_off, uint32_t *out_rows) {
    if (!c || !cand_ids || !cand_scores || !cand_off || !q_bases || !r || !out_rows || (!self_ids) != (!self_off))
        SH_FAIL("family_cascade: null argument");
    const bool msc = r->fs_msc_max < 1;
    if (msc && !cand_match) SH_FAIL("family_cascade: null argument (the rule asks for match counts)");
    std::lock_guard<std::mutex> lk(c->mu);
    sina_hip_hint_guard hints(c);
    if (!c->st->have_refs) SH_FAIL("family_cascade: upload references first");
    FamilyPlan plan;
    if (family_rule_plan("family_cascade", r, nq, &plan)) return 1;
    if (msc && match_table_bytes(c->st->width) > kMatchMaxLds) SH_FAIL_LIMIT("family_cascade: alignment too wide for the device match count");
    if (nq == 0) return 0;
    uint64_t max_n = 0;
    for (uint32_t q = 0; q < nq; q++) {
        if (cand_off[q + 1] < cand_off[q]) SH_FAIL("family_cascade: candidate offsets descend");
        max_n = std::max<uint64_t>(max_n, cand_off[q + 1] - cand_off[q]);
    }
    if (max_n >= 0xFFFFFFFFull) SH_FAIL("family_cascade: candidate list too long");
    for (uint64_t i = cand_off[0]; i < cand_off[nq]; i++)
        if (cand_ids[i] >= c->st->n_refs) SH_FAIL("family_cascade: reference id out of range");
    if (family_check_self("family_cascade", c, self_ids, self_off, nq)) return 1;
    SH_CHECK(hipSetDevice(c->device));
    // the lists as rows of one length (what the kernel addresses), padded with zeros; n[q] the list's length
    const uint32_t stride = (uint32_t)std::max<uint64_t>(max_n, 1);
    const size_t cells = (size_t)nq * stride;
    std::vector<uint32_t> ids(cells, 0u), n(nq);
    std::vector<float> sc(cells, 0.f);
    std::vector<uint16_t> mt(msc ? cells : 0, (uint16_t)0);
    std::vector<uint64_t> qoff(nq + 1, 0), srel(nq + 1, 0);
    for (uint32_t q = 0; q < nq; q++) {
        n[q] = (uint32_t)(cand_off[q + 1] - cand_off[q]);
        memcpy(ids.data() + (size_t)q * stride, cand_ids + cand_off[q], 4 * (size_t)n[q]);
        memcpy(sc.data() + (size_t)q * stride, cand_scores + cand_off[q], 4 * (size_t)n[q]);
        if (msc) memcpy(mt.data() + (size_t)q * stride, cand_match + cand_off[q], 2 * (size_t)n[q]);
        qoff[q + 1] = qoff[q] + q_bases[q];
        if (self_ids) srel[q + 1] = self_off[q + 1] - self_off[0];
    }
    const uint64_t n_self = self_ids ? srel[nq] : 0;
    hipStream_t s = c->stream;
    if (c->s_cand.reserve(4 * cells) || c->f_scores.reserve(4 * cells) || c->m_out.reserve(2 * std::max<size_t>(mt.size(), 1)) ||
        c->m_n.reserve(4 * (uint64_t)nq) || c->s_qoff.reserve(8 * ((uint64_t)nq + 1)) || c->f_self_ids.reserve(4 * std::max<uint64_t>(n_self, 1)) ||
        c->f_self_off.reserve(8 * ((uint64_t)nq + 1)))
        return 1;
    if (upload(c, 1, c->s_cand.p, ids.data(), 4 * cells, s) || upload(c, 2, c->f_scores.p, sc.data(), 4 * cells, s) ||
        upload(c, 3, c->m_out.p, mt.data(), 2 * mt.size(), s) || upload(c, 4, c->m_n.p, n.data(), 4 * (uint64_t)nq, s) ||
        upload(c, 5, c->s_qoff.p, qoff.data(), 8 * ((uint64_t)nq + 1), s))
        return 1;
    if (self_ids && (upload(c, 6, c->f_self_ids.p, self_ids + self_off[0], 4 * n_self, s) ||
                     upload(c, 7, c->f_self_off.p, srel.data(), 8 * ((uint64_t)nq + 1), s)))
        return 1;
    // (rows through a vector of the call's own: out_rows stays untouched if the launch fails)
    std::vector<uint32_t> rows((size_t)nq * plan.row_words);
    if (family_launch(c, c->s_cand.as<uint32_t>(), c->f_scores.as<float>(), c->m_out.as<uint16_t>(), c->m_n.as<uint32_t>(), stride,
                      c->s_qoff.as<uint64_t>(), nq, r, plan, self_ids ? c->f_self_ids.as<uint32_t>() : nullptr,
                      self_ids ? c->f_self_off.as<uint64_t>() : nullptr, n.data(), rows.data()))
        return 1;
    memcpy(out_rows, rows.data(), 4 * rows.size());
    return 0;
}

extern "C" int sina_hip_family_stats(sina_hip_ctx *c, double *kernel_ms, uint64_t *queries, uint64_t *candidates_listed,
                                      uint64_t *candidates_scanned, uint64_t *launches) {
    if (!c || !kernel_ms || !queries || !candidates_listed || !candidates_scanned || !launches) SH_FAIL("family_stats: null argument");
    if (read_use(c, kUseFamily, kernel_ms, candidates_listed, candidates_scanned, launches)) return 1;
    std::lock_guard<std::mutex> lk(c->mu);
    *queries = c->use[kUseFamily].c;
    return 0;
}
