// The host driver of a k-mer search call: argument checks, long queries put last, the walk over the launch ranges
// kmer_plan.h cuts the call into, staging, statistics, the hand-over of a range's candidates to the match-count and
// rank kernels -- and the C ABI's search entry points.  The kernels and their launchers are kmer.hip's, the index and
// the dense bitmaps kmer_index.hip's.
#include <cstring>
#include <memory>

#include "common.h"
#include "ctx.h"
#include "match_plan.h"
#include "family_plan.h"
#include "compare_dev.h"

namespace sina_hip {
namespace {

constexpr uint32_t kMaxQueryLen = SINA_HIP_MAX_QUERY_LEN, kMaxLongQueryLen = SINA_HIP_MAX_LONG_QUERY_LEN;

// sina_hip_kmer_topk_rank: the rules under which every range's candidates are ranked where the select left them
// (rank.hip)
struct RankReq {
    int iupac, filter_lc, cover;
    uint32_t N;
    uint32_t *out_flag;  // [nq]
};
// kmer_rows_resident: every range's final select rows stay on the device, in the caller's call-sized buffers
struct KeepReq {
    uint32_t *d_ids, *d_n;  // [nq][max], [nq] device memory
    uint32_t *h_n;          // [nq] the lengths again, on the host
};
// sina_hip_kmer_topk_family: every range's candidates go through the family cascade where the select (and, for an
// identity limit, the match count) left them (family.hip), and nothing but the cascade's rows comes to the host
struct FamilyReq {
    const sina_hip_family_rule *rule;
    FamilyPlan plan;
    const uint32_t *self_ids;  // the queries' self lists at self_off[q] .. self_off[q + 1] (host, absolute); null: none
    const uint64_t *self_off;
    uint32_t *out_rows;        // [nq][plan.row_words]
    bool msc() const { return rule->fs_msc_max < 1; }
};
// One search call.  out_ids / out_scores: [nq * row()], out_n: [nq].
// q_ab / out_match (sina_hip_kmer_topk_match; else null): the queries' packed aligned bases, one per mask byte, and
// where every range's match counts go (match.hip), [nq * max] like out_ids
// rk (sina_hip_kmer_topk_rank; else null): out_ids / out_scores are rows of the rank kernel, out_n its counts, and no
// id or k-mer score of the select is copied out
// keep (kmer_rows_resident; else null): nothing comes to the host but the lengths; out_ids / out_scores / out_n are null
// fam (sina_hip_kmer_topk_family; else null): the cascade's rows come to the host; out_ids / out_scores / out_n are null
struct KmerRequest {
    const uint8_t *qmask;
    const uint64_t *qoff;
    uint32_t nq, max;
    uint32_t *out_ids;
    float *out_scores;
    uint32_t *out_n;
    const uint32_t *q_ab = nullptr;
    uint16_t *out_match = nullptr;
    const RankReq *rk = nullptr;
    const KeepReq *keep = nullptr;
    const FamilyReq *fam = nullptr;
    uint32_t row() const { return rk ? rk->N : max; }  // entries of an output row
    uint32_t qlen(uint32_t q) const { return (uint32_t)(qoff[q + 1] - qoff[q]); }
};

// A range's kernels -- count, and select if wanted -- on the store's heavy FIFO (ctx.h); returns when they have ended.
// The context's buffers the launchers use are brought to the range's size first.
int run_kernels(sina_hip_ctx *c, KmerLaunch &l, bool want_select) {
    hipStream_t s = c->stream;
    const bool cand = l.path == kKmerCand;
    const size_t nq = l.nq, out_bytes = want_select ? nq * l.max * 4 : 0;
    if (reserve_kmer_big_select(c, &l)) return 1;
    if ((!cand && c->k_scores.reserve(nq * kmer_row_stride(c->st->n_refs) * 2 + 64)) || c->k_tmp2.reserve(8) || c->k_tmp0.reserve(4 * nq) ||
        (cand && c->k_tmp1.reserve(8 * nq * kCandCap)) || c->k_out_ids.reserve(out_bytes) || c->k_out_scores.reserve(out_bytes) ||
        c->k_out_n.reserve(want_select ? nq * 4 : 0))
        return 1;
    SH_CHECK(hipMemsetAsync(c->k_tmp2.p, 0, 8, s));
    if (ensure_dense(c)) return 1;
    heavy_launch hl(c, s, kHeavyKmer);  // (count + select: device-filling kernels, ctx.h)
    const hipStream_t hs = hl.stream();
    SH_CHECK(hipEventRecord(c->ev[3], hs));
    if (launch_kmer_count(c, l, hs)) return 1;
    SH_CHECK(hipEventRecord(c->ev[4], hs));
    if (want_select && launch_kmer_select(c, l, hs)) return 1;
    SH_CHECK(hipEventRecord(c->ev[5], hs));
    return hl.done();
}

// One launch range: kernels, results back through pinned staging, statistics; *overflow = a candidate list of the
// range did not hold its query's candidates (nothing was copied out then: the caller repeats the range with rows)
int run_range(sina_hip_ctx *c, const KmerRequest &r, const KmerRange &g, uint32_t max_qlen, bool *overflow) {
    hipStream_t s = c->stream;
    const uint32_t q0 = g.q0, bq = g.bq, max = r.max;
    KmerLaunch l{c->qmask.as<uint8_t>(), c->k_qoff.as<uint64_t>() + q0, bq, max, max_qlen, g.path, g.big};
    if (run_kernels(c, l, true)) return 1;
    // (the kernels have finished: run_kernels waits for the heavy stream)
    if ((!r.rk && !r.keep && !r.fam && (download(c, 9, c->k_out_ids.p, (size_t)bq * max * 4, s) || download(c, 10, c->k_out_scores.p, (size_t)bq * max * 4, s))) ||
        download(c, 11, c->k_out_n.p, (size_t)bq * 4, s) || download(c, 0, c->k_tmp2.p, 8, s))
        return 1;
    SH_CHECK(wait_stream(c, s));
    *overflow = false;
    if (g.path == kKmerCand) {
        const uint32_t *n = static_cast<const uint32_t *>(c->h_stage[11].p);
        for (uint32_t q = 0; q < bq && !*overflow; q++) *overflow = n[q] == 0xFFFFFFFFu;
    }
    unsigned long long visited = 0;
    memcpy(&visited, c->h_stage[0].p, 8);
    float ms = 0, ms2 = 0;
    SH_CHECK(hipEventElapsedTime(&ms, c->ev[3], c->ev[4]));
    SH_CHECK(hipEventElapsedTime(&ms2, c->ev[4], c->ev[5]));
    {
        std::lock_guard<std::mutex> slk(c->st->stats_mu);
        c->st->stats.kmer_count_ms += ms;
        c->st->stats.kmer_select_ms += ms2;
        c->st->stats.kmer_launches++;
        if (!*overflow) {
            c->st->stats.postings += visited;
            c->st->stats.kmer_queries += bq;
        }
    }
    if (*overflow) return 0;
    if (g.path == kKmerLong) c->path_queries[kPathLong] += bq;
    if (g.big) c->path_queries[kPathBigSelect] += bq;
    if (r.keep) {  // the range's select is final: its rows to their place in the call's, before the next range's select writes over them
        SH_CHECK(hipMemcpyAsync(r.keep->d_ids + (size_t)q0 * max, c->k_out_ids.p, (size_t)bq * max * 4, hipMemcpyDeviceToDevice, s));
        SH_CHECK(hipMemcpyAsync(r.keep->d_n + q0, c->k_out_n.p, (size_t)bq * 4, hipMemcpyDeviceToDevice, s));
        memcpy(r.keep->h_n + q0, c->h_stage[11].p, (size_t)bq * 4);
        return 0;
    }
    if (r.fam) {  // the range's select is final: the match counts if the rule has an identity limit, then the cascade
        const uint32_t *h_n = static_cast<const uint32_t *>(c->h_stage[11].p);
        if (r.fam->msc()) {
            const size_t row_bytes = (size_t)bq * max * 2;
            if (c->m_out.reserve(row_bytes)) return 1;
            SH_CHECK(hipMemsetAsync(c->m_out.p, 0, row_bytes, s));
            if (match_launch(c, c->s_qab.as<uint32_t>(), l.qoff, bq, c->k_out_ids.as<uint32_t>(), c->k_out_n.as<uint32_t>(), max,
                             c->m_out.as<uint16_t>(), nullptr, h_n))
                return 1;
        }
        return family_launch(c, c->k_out_ids.as<uint32_t>(), c->k_out_scores.as<float>(), c->m_out.as<uint16_t>(), c->k_out_n.as<uint32_t>(),
                             max, l.qoff, bq, r.fam->rule, family_plan(r.fam->rule->fs_min, r.fam->rule->fs_max, r.fam->rule->fs_req_full,
                                                                       r.fam->rule->fs_cover_gene, bq),
                             r.fam->self_ids ? c->f_self_ids.as<uint32_t>() : nullptr,
                             r.fam->self_ids ? c->f_self_off.as<uint64_t>() + q0 : nullptr, h_n,
                             r.fam->out_rows + (size_t)q0 * r.fam->plan.row_words);
    }
    if (r.rk) {  // the range's select is final: its candidates ranked, ids and lengths read where they lie
        uint32_t max_la = 0;
        for (uint32_t q = q0; q < q0 + bq; q++) max_la = std::max(max_la, r.qlen(q));
        return rank_launch(c, c->s_qab.as<uint32_t>(), l.qoff, bq, c->k_out_ids.as<uint32_t>(), nullptr, c->k_out_n.as<uint32_t>(), max,
                           max, max_la, r.rk->iupac, r.rk->filter_lc, r.rk->cover, r.rk->N, r.out_ids + (size_t)q0 * r.rk->N,
                           r.out_scores + (size_t)q0 * r.rk->N, r.out_n + q0, r.rk->out_flag + q0);
    }
    memcpy(r.out_ids + (size_t)q0 * max, c->h_stage[9].p, (size_t)bq * max * 4);
    memcpy(r.out_scores + (size_t)q0 * max, c->h_stage[10].p, (size_t)bq * max * 4);
    memcpy(r.out_n + q0, c->h_stage[11].p, (size_t)bq * 4);
    if (r.out_match) {  // the range's select is final: its candidates' match counts, ids and lengths read where they lie
        const size_t row_bytes = (size_t)bq * max * 2;
        if (c->m_out.reserve(row_bytes)) return 1;
        SH_CHECK(hipMemsetAsync(c->m_out.p, 0, row_bytes, s));
        if (match_launch(c, c->s_qab.as<uint32_t>(), l.qoff, bq, c->k_out_ids.as<uint32_t>(), c->k_out_n.as<uint32_t>(), max,
                         c->m_out.as<uint16_t>(), static_cast<const uint32_t *>(c->h_stage[9].p),
                         static_cast<const uint32_t *>(c->h_stage[11].p)) ||
            download(c, 5, c->m_out.p, row_bytes, s))
            return 1;
        SH_CHECK(wait_stream(c, s));
        memcpy(r.out_match + (size_t)q0 * max, c->h_stage[5].p, row_bytes);
    }
    return 0;
}

// A call behind its checks (c->mu held, 1 <= max <= n_refs): the queries' masks, offsets and packed bases to the
// device, then range by range as kmer_plan.h cuts them -- queries 0 .. n_fast - 1 are at most kMaxQueryLen bases long,
// queries n_fast .. nq - 1 longer
int kmer_topk_run(sina_hip_ctx *c, const KmerRequest &r, uint32_t n_fast) {
    const uint32_t nq = r.nq, n_refs = c->st->n_refs;
    const uint64_t *qoff = r.qoff;
    uint32_t max_qlen = 1;
    for (uint32_t q = 0; q < n_fast; q++) max_qlen = std::max(max_qlen, r.qlen(q));
    hipStream_t s = c->stream;
    const uint64_t nqm = qoff[nq] - qoff[0];
    if (c->qmask.reserve(std::max<uint64_t>(nqm, 1)) || c->k_qoff.reserve(8 * ((uint64_t)nq + 1))) return 1;
    std::vector<uint64_t> rel(nq + 1);
    for (uint32_t q = 0; q <= nq; q++) rel[q] = qoff[q] - qoff[0];
    if (upload(c, 7, c->qmask.p, r.qmask + qoff[0], nqm, s) || upload(c, 8, c->k_qoff.p, rel.data(), 8 * ((uint64_t)nq + 1), s))
        return 1;
    if ((r.out_match || r.rk || (r.fam && r.fam->msc())) && (c->s_qab.reserve(4 * std::max<uint64_t>(nqm, 1)) || upload(c, 1, c->s_qab.p, r.q_ab + qoff[0], 4 * nqm, s))) return 1;
    if (r.fam && r.fam->self_ids) {  // the call's self lists, offsets from the first query's
        const uint64_t *so = r.fam->self_off;
        std::vector<uint64_t> srel(nq + 1);
        for (uint32_t q = 0; q <= nq; q++) srel[q] = so[q] - so[0];
        if (c->f_self_ids.reserve(4 * std::max<uint64_t>(srel[nq], 1)) || c->f_self_off.reserve(8 * ((uint64_t)nq + 1)) ||
            upload(c, 2, c->f_self_ids.p, r.fam->self_ids + so[0], 4 * srel[nq], s) || upload(c, 3, c->f_self_off.p, srel.data(), 8 * ((uint64_t)nq + 1), s))
            return 1;
    }
    // (SINA_HIP_TEST=big_sel_bytes=N: a test's budget of the big select; kmer_rows=1: no candidate lists)
    uint64_t budget = kBigSelBudget;
    if (const std::string e_ = test_knob("big_sel_bytes"); !e_.empty()) budget = std::min<uint64_t>(kBigSelBudget, strtoull(e_.c_str(), nullptr, 10));
    const bool force_rows = atoi(test_knob("kmer_rows").c_str()) != 0;
    for (const KmerRange &g : kmer_ranges(nq, n_fast, r.max, n_refs, budget, force_rows)) {
        bool overflow = false;
        if (run_range(c, r, g, max_qlen, &overflow)) return 1;
        if (!overflow) continue;  // else a giant group of equal scores somewhere in the range: the score rows and the full select
        for (const KmerRange &h : kmer_overflow_ranges(g, n_refs))
            if (run_range(c, r, h, max_qlen, &overflow)) return 1;
    }
    return 0;
}

// A batch with long queries runs in the order kmer_fast_first gives, on buffers of the call's own ...
struct Reordered {
    std::vector<uint64_t> off;
    std::vector<uint8_t> mask;
    std::vector<uint32_t> ab, ids, n, fl;
    std::vector<float> sc;
    std::vector<uint16_t> mt;
    std::vector<uint32_t> self_ids, rows;  // the family request's self lists, in the new order, and its rows
    std::vector<uint64_t> self_off;
    RankReq rk;
    FamilyReq fam;
    KmerRequest req;  // the request over these buffers
};
// ... which gather_queries fills with the request's queries (the packed bases move with their queries) ...
void gather_queries(const KmerRequest &r, const std::vector<uint32_t> &order, Reordered *g) {
    const uint32_t nq = r.nq;
    g->off.assign(nq + 1, 0);
    for (uint32_t x = 0; x < nq; x++) g->off[x + 1] = g->off[x] + r.qlen(order[x]);
    g->mask.resize(g->off[nq]);
    g->ab.resize(r.q_ab ? g->off[nq] : 0);
    for (uint32_t x = 0; x < nq; x++) {
        memcpy(g->mask.data() + g->off[x], r.qmask + r.qoff[order[x]], g->off[x + 1] - g->off[x]);
        if (r.q_ab) memcpy(g->ab.data() + g->off[x], r.q_ab + r.qoff[order[x]], 4 * (g->off[x + 1] - g->off[x]));
    }
    if (r.fam) {
        g->fam = *r.fam;
        g->rows.resize((size_t)nq * r.fam->plan.row_words);
        g->fam.out_rows = g->rows.data();
        if (r.fam->self_ids) {
            g->self_off.assign(nq + 1, 0);
            for (uint32_t x = 0; x < nq; x++) {
                const uint64_t b = r.fam->self_off[order[x]], e = r.fam->self_off[order[x] + 1];
                g->self_ids.insert(g->self_ids.end(), r.fam->self_ids + b, r.fam->self_ids + e);
                g->self_off[x + 1] = g->self_ids.size();
            }
            g->self_ids.push_back(0);  // (never empty: data() is the list's address)
            g->fam.self_ids = g->self_ids.data();
            g->fam.self_off = g->self_off.data();
        }
        g->req = KmerRequest{g->mask.data(), g->off.data(), nq, r.max, nullptr, nullptr, nullptr, r.q_ab ? g->ab.data() : nullptr};
        g->req.fam = &g->fam;
        return;
    }
    g->ids.resize((size_t)nq * r.row());
    g->sc.resize((size_t)nq * r.row());
    g->n.resize(nq);
    g->fl.resize(r.rk ? nq : 0);
    g->mt.resize(r.out_match ? (size_t)nq * r.max : 0);
    if (r.rk) g->rk = RankReq{r.rk->iupac, r.rk->filter_lc, r.rk->cover, r.rk->N, g->fl.data()};
    g->req = KmerRequest{g->mask.data(), g->off.data(), nq, r.max, g->ids.data(), g->sc.data(), g->n.data(),
                         r.q_ab ? g->ab.data() : nullptr, r.out_match ? g->mt.data() : nullptr, r.rk ? &g->rk : nullptr};
}
// ... and scatter_results empties into the caller's rows, in the caller's order
void scatter_results(const Reordered &g, const std::vector<uint32_t> &order, const KmerRequest &r) {
    const uint32_t row = r.row(), max = r.max;
    if (r.fam) {
        const size_t w = r.fam->plan.row_words;
        for (uint32_t x = 0; x < r.nq; x++) memcpy(r.fam->out_rows + order[x] * w, g.rows.data() + x * w, 4 * w);
        return;
    }
    for (uint32_t x = 0; x < r.nq; x++) {
        if (r.out_match) memcpy(r.out_match + (size_t)order[x] * max, g.mt.data() + (size_t)x * max, (size_t)max * 2);
        memcpy(r.out_ids + (size_t)order[x] * row, g.ids.data() + (size_t)x * row, (size_t)row * 4);
        memcpy(r.out_scores + (size_t)order[x] * row, g.sc.data() + (size_t)x * row, (size_t)row * 4);
        r.out_n[order[x]] = g.n[x];
        if (r.rk) r.rk->out_flag[order[x]] = g.fl[x];
    }
}

// any: queries of up to kMaxLongQueryLen bases (sina_hip_kmer_topk_any), the longer ones behind the others for
// kmer_topk_run and back into the caller's order
int kmer_topk_checked(sina_hip_ctx *c, const KmerRequest &in, bool any) {
    if (!c || !in.qmask || !in.qoff || (!in.fam && (!in.out_ids || !in.out_scores || !in.out_n))) SH_FAIL("kmer_topk: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    sina_hip_hint_guard hints(c);
    if (index_ready(c)) return 1;
    KmerRequest r = in;
    const uint32_t nq = r.nq;
    if (r.out_match && match_table_bytes(c->st->width) > kMatchMaxLds)
        SH_FAIL_LIMIT("kmer_topk_match: alignment too wide for the device match count");
    if (r.fam) {
        if (r.fam->msc() && match_table_bytes(c->st->width) > kMatchMaxLds)
            SH_FAIL_LIMIT("kmer_topk_family: alignment too wide for the device match count");
        if (family_check_self("kmer_topk_family", c, r.fam->self_ids, r.fam->self_off, nq)) return 1;
    }
    if (r.rk) {
        if (rank_check_rules("kmer_topk_rank", c, r.rk->iupac, r.rk->cover, r.rk->N)) return 1;
        uint32_t max_la = 0;
        for (uint32_t q = 0; q < nq; q++) max_la = std::max(max_la, r.qlen(q));
        if (compare_table_bytes(c->st->width, max_la) > kCompareMaxLds)
            SH_FAIL_LIMIT("kmer_topk_rank: alignment too wide for the device comparison");
        if (kmer_big_select(std::min(r.max, c->st->n_refs)))
            SH_FAIL_LIMIT("kmer_topk_rank: more than 4096 candidates per query");
    }
    if (nq == 0) return 0;
    SH_CHECK(hipSetDevice(c->device));
    if (r.max > c->st->n_refs) r.max = c->st->n_refs;
    if (r.max == 0 && r.fam) {
        for (uint32_t q = 0; q < nq; q++) family_empty_row(r.fam->rule, r.fam->plan.row_words, r.fam->out_rows + (size_t)q * r.fam->plan.row_words);
        return 0;
    }
    if (r.max == 0) {
        memset(r.out_n, 0, sizeof(uint32_t) * nq);
        if (r.rk) memset(r.rk->out_flag, 0, sizeof(uint32_t) * nq);
        return 0;
    }
    uint32_t n_long = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const uint64_t len = r.qoff[q + 1] - r.qoff[q];
        if (!any && len > (uint64_t)kMaxQueryLen) SH_FAIL("kmer_topk: query longer than SINA_HIP_MAX_QUERY_LEN bases");
        if (len > (uint64_t)kMaxLongQueryLen) SH_FAIL_LIMIT("kmer_topk_any: query longer than SINA_HIP_MAX_LONG_QUERY_LEN bases");
        n_long += len > (uint64_t)kMaxQueryLen;
    }
    if (n_long == 0) return kmer_topk_run(c, r, nq);
    uint32_t n_fast = 0;
    const std::vector<uint32_t> order = kmer_fast_first(r.qoff, nq, &n_fast);
    Reordered g;
    gather_queries(r, order, &g);
    if (kmer_topk_run(c, g.req, n_fast)) return 1;
    scatter_results(g, order, r);
    return 0;
}

int kmer_scores_checked(sina_hip_ctx *c, const uint8_t *qmask, uint32_t qlen, int16_t *scores, bool any) {
    if (!c || !qmask || !scores) SH_FAIL("kmer_scores: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (index_ready(c)) return 1;
    if (!any && qlen > kMaxQueryLen) SH_FAIL("kmer_scores: query longer than SINA_HIP_MAX_QUERY_LEN bases");
    if (qlen > kMaxLongQueryLen) SH_FAIL_LIMIT("kmer_scores_any: query longer than SINA_HIP_MAX_LONG_QUERY_LEN bases");
    SH_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint64_t rel[2] = {0, qlen};
    if (c->qmask.reserve(std::max<uint32_t>(qlen, 1)) || c->k_qoff.reserve(16)) return 1;
    SH_CHECK(hipMemcpyAsync(c->qmask.p, qmask, qlen, hipMemcpyHostToDevice, s));
    SH_CHECK(hipMemcpyAsync(c->k_qoff.p, rel, 16, hipMemcpyHostToDevice, s));
    // one query's score row -- the plan's one range of it, score rows forced -- and no select
    uint32_t n_fast = 0;
    kmer_fast_first(rel, 1, &n_fast);
    const KmerRange g = kmer_ranges(1, n_fast, 1, c->st->n_refs, 0, true)[0];
    KmerLaunch l{c->qmask.as<uint8_t>(), c->k_qoff.as<uint64_t>(), g.bq, 1, std::max<uint32_t>(qlen, 1), g.path, g.big};
    if (run_kernels(c, l, false)) return 1;
    if (g.path == kKmerLong) c->path_queries[kPathLong]++;
    SH_CHECK(hipMemcpyAsync(scores, c->k_scores.p, (size_t)c->st->n_refs * 2, hipMemcpyDeviceToHost, s));
    SH_CHECK(hipStreamSynchronize(s));
    return 0;
}

// the mask bytes the count kernel reads of packed aligned bases, one per packed word, and the queries' offsets from
// the first query's first base (q_ab + q_off[0] is what they index)
struct PackedMasks {
    std::vector<uint8_t> mask;
    std::vector<uint64_t> rel;
    PackedMasks(const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq) : mask(q_off[nq] - q_off[0] + 1), rel(nq + 1) {
        for (uint64_t i = q_off[0]; i < q_off[nq]; i++) mask[i - q_off[0]] = (uint8_t)(q_ab[i] >> 24);
        for (uint32_t q = 0; q <= nq; q++) rel[q] = q_off[q] - q_off[0];
    }
};

}  // namespace

int kmer_rows_resident(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t max, uint32_t *d_ids,
                       uint32_t *d_n, uint32_t *h_n) {
    if (index_ready(c)) return 1;
    if (nq == 0 || max == 0 || max > c->st->n_refs) SH_FAIL("kmer_rows_resident: nothing to search, or more rows than references");
    const KeepReq keep{d_ids, d_n, h_n};
    KmerRequest r{qmask, qoff, nq, max, nullptr, nullptr, nullptr};
    r.keep = &keep;
    return kmer_topk_run(c, r, nq);
}

}  // namespace sina_hip

using namespace sina_hip;

extern "C" {

int sina_hip_kmer_topk(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t max,
                       uint32_t *out_ids, float *out_scores, uint32_t *out_n) {
    return kmer_topk_checked(c, KmerRequest{qmask, qoff, nq, max, out_ids, out_scores, out_n}, false);
}
int sina_hip_kmer_topk_any(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t max,
                           uint32_t *out_ids, float *out_scores, uint32_t *out_n) {
    return kmer_topk_checked(c, KmerRequest{qmask, qoff, nq, max, out_ids, out_scores, out_n}, true);
}
int sina_hip_kmer_topk_match(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t max,
                             uint32_t *out_ids, float *out_scores, uint32_t *out_n, uint16_t *out_match) {
    if (!c || !q_ab || !q_off || !out_ids || !out_scores || !out_n || !out_match) SH_FAIL("kmer_topk_match: null argument");
    if (match_check_queries("kmer_topk_match", q_ab, q_off, nq)) return 1;
    const PackedMasks pm(q_ab, q_off, nq);
    return kmer_topk_checked(c, KmerRequest{pm.mask.data(), pm.rel.data(), nq, max, out_ids, out_scores, out_n, q_ab + q_off[0], out_match}, true);
}
int sina_hip_kmer_topk_rank(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t kmer_candidates,
                            int iupac_rule, int filter_lowercase, int cover_rule, uint32_t max_result, uint32_t *out_ids,
                            float *out_scores, uint32_t *out_n, uint32_t *out_flag) {
    if (!c || !q_ab || !q_off || !out_ids || !out_scores || !out_n || !out_flag) SH_FAIL("kmer_topk_rank: null argument");
    if (match_check_queries("kmer_topk_rank", q_ab, q_off, nq)) return 1;
    const PackedMasks pm(q_ab, q_off, nq);
    // (results through vectors of the call's own: the outputs stay untouched if a range fails)
    std::vector<uint32_t> ids((size_t)nq * std::max(max_result, 1u)), n(nq), fl(nq);
    std::vector<float> sc(ids.size());
    const RankReq rk{iupac_rule, filter_lowercase ? 1 : 0, cover_rule, max_result, fl.data()};
    if (kmer_topk_checked(c, KmerRequest{pm.mask.data(), pm.rel.data(), nq, kmer_candidates, ids.data(), sc.data(), n.data(), q_ab + q_off[0], nullptr, &rk}, true))
        return 1;
    memcpy(out_ids, ids.data(), 4 * (size_t)nq * max_result);
    memcpy(out_scores, sc.data(), 4 * (size_t)nq * max_result);
    memcpy(out_n, n.data(), 4 * (size_t)nq);
    memcpy(out_flag, fl.data(), 4 * (size_t)nq);
    return 0;
}
int sina_hip_kmer_topk_family(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t max,
                              const sina_hip_family_rule *rule, const uint32_t *self_ids, const uint64_t *self_off, uint32_t *out_rows) {
    if (!c || !q_ab || !q_off || !rule || !out_rows || (!self_ids) != (!self_off)) SH_FAIL("kmer_topk_family: null argument");
    FamilyReq fam{rule, FamilyPlan(), self_ids, self_off, nullptr};
    if (family_rule_plan("kmer_topk_family", rule, nq, &fam.plan)) return 1;
    if (fam.msc() && match_check_queries("kmer_topk_family", q_ab, q_off, nq)) return 1;
    for (uint32_t q = 0; q < nq; q++)
        if (q_off[q + 1] < q_off[q]) SH_FAIL("kmer_topk_family: query offsets descend");
    // the mask bytes the count kernel reads, bits 24..31 of every word (PackedMasks' bytes; an uninitialised block and
    // restrict pointers: on the default path, 41 candidates per query, this loop is most of what the entry adds)
    const uint64_t n_bases = q_off[nq] - q_off[0];
    const std::unique_ptr<uint8_t[]> mask(new uint8_t[n_bases + 1]);
    {
        const uint32_t *__restrict src = q_ab + q_off[0];
        uint8_t *__restrict dst = mask.get();
        for (uint64_t i = 0; i < n_bases; i++) dst[i] = (uint8_t)(src[i] >> 24);
    }
    std::vector<uint64_t> rel(nq + 1);
    for (uint32_t q = 0; q <= nq; q++) rel[q] = q_off[q] - q_off[0];
    // (rows through a vector of the call's own: out_rows stays untouched if a range fails)
    std::vector<uint32_t> rows((size_t)nq * fam.plan.row_words);
    fam.out_rows = rows.data();
    KmerRequest r{mask.get(), rel.data(), nq, max, nullptr, nullptr, nullptr, q_ab + q_off[0]};
    r.fam = &fam;
    if (kmer_topk_checked(c, r, true)) return 1;
    memcpy(out_rows, rows.data(), 4 * rows.size());
    return 0;
}
int sina_hip_kmer_scores(sina_hip_ctx *c, const uint8_t *qmask, uint32_t qlen, int16_t *scores) {
    return kmer_scores_checked(c, qmask, qlen, scores, false);
}
int sina_hip_kmer_scores_any(sina_hip_ctx *c, const uint8_t *qmask, uint32_t qlen, int16_t *scores) {
    return kmer_scores_checked(c, qmask, qlen, scores, true);
}
int sina_hip_long_queries(sina_hip_ctx *c, uint64_t *n) {
    if (!c || !n) SH_FAIL("long_queries: null argument");
    return read_path_queries(c, kPathLong, n);
}

int sina_hip_big_select_queries(sina_hip_ctx *c, uint64_t *n) {
    if (!c || !n) SH_FAIL("big_select_queries: null argument");
    return read_path_queries(c, kPathBigSelect, n);
}

}  // extern "C"
