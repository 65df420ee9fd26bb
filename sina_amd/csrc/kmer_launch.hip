// The host driver of a k-mer search call and the C ABI's search entry points.  The driver: argument checks, long
// queries put last, the walk over the launch ranges kmer_plan.h cuts the call into, staging, statistics.  What a call
// does with a range's final select rows is its sink's (KmerSink): copied out (plain), counted (match), ranked (rank),
// kept on the device (keep) or put through the family cascade (family) -- the driver asks the sink and never which
// one it is.  The copies that bring a call's queries into the order it runs in and its rows back are kmer_plan.h's, over
// the inputs and columns the sink lists.  The kernels and their launchers are kmer.hip's, match.hip's, rank.hip's and
// family.hip's, the index and the dense bitmaps kmer_index.hip's.
// A call with a turn request (sina_hip_kmer_topk_turn) searches the n tried orientations of every query
// as n virtual queries: the queries go up once, turn.hip's orient kernel writes the variants where a search's queries
// lie, the ranges -- whole queries, turn_plan.h -- run through the same launchers, and where a range's select is final
// turn.hip's pick kernel leaves the winners' rows, which is what the sink sees: a range of real queries.
#include <cstring>
#include <memory>

#include "common.h"
#include "ctx.h"
#include "match_plan.h"
#include "family_plan.h"
#include "turn_plan.h"
#include "compare_dev.h"

namespace sina_hip {
namespace {

constexpr uint32_t kMaxQueryLen = SINA_HIP_MAX_QUERY_LEN, kMaxLongQueryLen = SINA_HIP_MAX_LONG_QUERY_LEN;

struct KmerSink;
// One search call: the queries' mask bytes, their offsets (host, absolute), their packed aligned bases, one per mask
// byte (read only where the sink needs them on the device), and what becomes of every range's select rows
struct KmerRequest {
    const uint8_t *qmask;
    const uint64_t *qoff;
    uint32_t nq, max;
    const uint32_t *q_ab;
    KmerSink *sink;
    uint32_t turn_n = 0;  // a turn request: the orientations tried per query (turn_plan.h: 2 or 4); 0: none
    uint32_t qlen(uint32_t q) const { return (uint32_t)(qoff[q + 1] - qoff[q]); }
};

// What a call does with a launch range's final select rows (c->k_out_ids / k_out_scores / k_out_n), and what the
// driver has to know of it.  Asked once per call and once per range, never per query.
struct KmerSink {
    virtual ~KmerSink() = default;
    // the limits of this kind of call, before anything runs (r.max: not yet clipped to the references there are)
    virtual int check(sina_hip_ctx *, const KmerRequest &) const { return 0; }
    // the packed aligned bases on the device, in c->s_qab?
    virtual bool needs_bases() const { return false; }
    // uploads of the sink's own for the whole call, behind the queries'
    virtual int upload(sina_hip_ctx *, uint32_t /*nq*/, hipStream_t) { return 0; }
    // a range's ids and scores to pinned staging (h_stage[9], [10]) before range()?
    virtual bool downloads_rows() const { return false; }
    // the caller's rows untouched unless the whole call succeeded?  (else they are written range by range)
    virtual bool all_or_nothing() const { return false; }
    // the call's candidates per query once they are clipped to the references there are: the width of its rows
    virtual void set_max(uint32_t /*max*/) {}
    // The inputs of its own that move with a query, and the rows it writes per query.  The driver may point them at
    // storage of the call's own for the time the call runs.
    virtual std::vector<KmerRagged *> inputs() { return {}; }
    virtual std::vector<KmerColumn *> columns() { return {}; }
    // the rows of nq queries of a call for no candidate at all (max == 0)
    virtual void empty(uint32_t nq) = 0;
    // Queries q0 .. q0 + bq - 1 of request r: their select is final (l: its launch; h_n: the lengths on the host, in
    // h_stage[11]).  Returns when the sink's rows of them are written.
    virtual int range(sina_hip_ctx *c, const KmerRequest &r, const KmerLaunch &l, uint32_t q0, uint32_t bq, const uint32_t *h_n) = 0;
};

// the range's candidates' match counts into c->m_out, ids and lengths read where they lie (h_ids: null or staged)
int range_match_counts(sina_hip_ctx *c, const KmerLaunch &l, uint32_t bq, const uint32_t *h_ids, const uint32_t *h_n) {
    const size_t row_bytes = (size_t)bq * l.max * 2;
    if (c->m_out.reserve(row_bytes)) return 1;
    SH_CHECK(hipMemsetAsync(c->m_out.p, 0, row_bytes, c->stream));
    return match_launch(c, c->s_qab.as<uint32_t>(), l.qoff, bq, c->k_out_ids.as<uint32_t>(), c->k_out_n.as<uint32_t>(), l.max,
                        c->m_out.as<uint16_t>(), h_ids, h_n);
}

// sina_hip_kmer_topk, _any: ids [nq][max], scores [nq][max] and lengths [nq] to the host
struct PlainSink : KmerSink {
    KmerColumn ids, scores, n;
    PlainSink(uint32_t *out_ids, float *out_scores, uint32_t *out_n) : ids{out_ids, 0}, scores{out_scores, 0}, n{out_n, 4} {}
    bool downloads_rows() const override { return true; }
    void set_max(uint32_t max) override { ids.bytes = scores.bytes = (size_t)max * 4; }
    std::vector<KmerColumn *> columns() override { return {&ids, &scores, &n}; }
    void empty(uint32_t nq) override { memset(n.base, 0, sizeof(uint32_t) * nq); }
    int range(sina_hip_ctx *c, const KmerRequest &, const KmerLaunch &l, uint32_t q0, uint32_t bq, const uint32_t *h_n) override {
        memcpy(ids.row<uint32_t>(q0), c->h_stage[9].p, (size_t)bq * l.max * 4);
        memcpy(scores.row<float>(q0), c->h_stage[10].p, (size_t)bq * l.max * 4);
        memcpy(n.row<uint32_t>(q0), h_n, (size_t)bq * 4);
        return 0;
    }
};
// sina_hip_kmer_topk_match: the same, and every candidate's match count (match.hip), [nq][max] like the ids
struct MatchSink : PlainSink {
    KmerColumn match;
    MatchSink(uint32_t *out_ids, float *out_scores, uint32_t *out_n, uint16_t *out_match) : PlainSink(out_ids, out_scores, out_n), match{out_match, 0} {}
    int check(sina_hip_ctx *c, const KmerRequest &) const override {
        if (match_table_bytes(c->st->width) > kMatchMaxLds) SH_FAIL_LIMIT("kmer_topk_match: alignment too wide for the device match count");
        return 0;
    }
    bool needs_bases() const override { return true; }
    void set_max(uint32_t max) override {
        PlainSink::set_max(max);
        match.bytes = (size_t)max * 2;
    }
    std::vector<KmerColumn *> columns() override { return {&ids, &scores, &n, &match}; }
    int range(sina_hip_ctx *c, const KmerRequest &r, const KmerLaunch &l, uint32_t q0, uint32_t bq, const uint32_t *h_n) override {
        const size_t row_bytes = (size_t)bq * l.max * 2;
        if (PlainSink::range(c, r, l, q0, bq, h_n) || range_match_counts(c, l, bq, static_cast<const uint32_t *>(c->h_stage[9].p), h_n) ||
            download(c, 5, c->m_out.p, row_bytes, c->stream))
            return 1;
        SH_CHECK(wait_stream(c, c->stream));
        memcpy(match.row<uint16_t>(q0), c->h_stage[5].p, row_bytes);
        return 0;
    }
};
// sina_hip_kmer_topk_turn: the chosen orientation's rows, and what the pick kernel left of the choice in pinned staging
// (h_stage[6]: [5] words per query, the orientation and the four top-1 scores' bits): turn [nq] bytes, top1 [nq][4]
struct TurnSink : PlainSink {
    KmerColumn turn, top1;
    TurnSink(uint8_t *out_turn, float *out_top1, uint32_t *out_ids, float *out_scores, uint32_t *out_n)
        : PlainSink(out_ids, out_scores, out_n), turn{out_turn, 1}, top1{out_top1, 16} {}
    std::vector<KmerColumn *> columns() override { return {&ids, &scores, &n, &turn, &top1}; }
    void empty(uint32_t nq) override {
        PlainSink::empty(nq);
        memset(turn.base, 0, nq);
        memset(top1.base, 0, (size_t)16 * nq);
    }
    int range(sina_hip_ctx *c, const KmerRequest &r, const KmerLaunch &l, uint32_t q0, uint32_t bq, const uint32_t *h_n) override {
        if (PlainSink::range(c, r, l, q0, bq, h_n)) return 1;
        const uint32_t *meta = static_cast<const uint32_t *>(c->h_stage[6].p);
        for (uint32_t q = 0; q < bq; q++) {
            *turn.row<uint8_t>(q0 + q) = (uint8_t)meta[(size_t)5 * q];
            memcpy(top1.row<float>(q0 + q), meta + (size_t)5 * q + 1, 16);
        }
        return 0;
    }
};
// sina_hip_kmer_topk_rank: every range's candidates ranked where the select left them (rank.hip) -- ids and scores are
// the rank kernel's rows of N, n its counts, and no id or k-mer score of the select is copied out
struct RankSink : KmerSink {
    int iupac, filter_lc, cover;
    uint32_t N;
    KmerColumn ids, scores, n, flag;
    RankSink(int iupac_, int filter_lc_, int cover_, uint32_t N_, uint32_t *out_ids, float *out_scores, uint32_t *out_n, uint32_t *out_flag)
        : iupac(iupac_), filter_lc(filter_lc_), cover(cover_), N(N_), ids{out_ids, (size_t)N_ * 4}, scores{out_scores, (size_t)N_ * 4},
          n{out_n, 4}, flag{out_flag, 4} {}
    int check(sina_hip_ctx *c, const KmerRequest &r) const override {
        if (rank_check_rules("kmer_topk_rank", c, iupac, cover, N)) return 1;
        if (compare_table_bytes(c->st->width, longest(r, 0, r.nq)) > kCompareMaxLds)
            SH_FAIL_LIMIT("kmer_topk_rank: alignment too wide for the device comparison");
        if (kmer_big_select(std::min(r.max, c->st->n_refs))) SH_FAIL_LIMIT("kmer_topk_rank: more than 4096 candidates per query");
        return 0;
    }
    bool needs_bases() const override { return true; }
    bool all_or_nothing() const override { return true; }
    std::vector<KmerColumn *> columns() override { return {&ids, &scores, &n, &flag}; }
    void empty(uint32_t nq) override {
        memset(n.base, 0, sizeof(uint32_t) * nq);
        memset(flag.base, 0, sizeof(uint32_t) * nq);
    }
    int range(sina_hip_ctx *c, const KmerRequest &r, const KmerLaunch &l, uint32_t q0, uint32_t bq, const uint32_t *) override {
        return rank_launch(c, c->s_qab.as<uint32_t>(), l.qoff, bq, c->k_out_ids.as<uint32_t>(), nullptr, c->k_out_n.as<uint32_t>(), l.max,
                           l.max, longest(r, q0, bq), iupac, filter_lc, cover, N, ids.row<uint32_t>(q0), scores.row<float>(q0),
                           n.row<uint32_t>(q0), flag.row<uint32_t>(q0));
    }
    static uint32_t longest(const KmerRequest &r, uint32_t q0, uint32_t bq) {
        uint32_t max_la = 0;
        for (uint32_t q = q0; q < q0 + bq; q++) max_la = std::max(max_la, r.qlen(q));
        return max_la;
    }
};
// kmer_rows_resident: every range's rows stay on the device, in the caller's call-sized buffers d_ids [nq][max] and
// d_n [nq]; nothing comes to the host but the lengths, h_n [nq]
struct KeepSink : KmerSink {
    uint32_t *d_ids, *d_n, *h_n;
    KeepSink(uint32_t *d_ids_, uint32_t *d_n_, uint32_t *h_n_) : d_ids(d_ids_), d_n(d_n_), h_n(h_n_) {}
    void empty(uint32_t) override {}  // (kmer_rows_resident refuses max == 0)
    // the range's rows to their place in the call's, before the next range's select writes over them
    int range(sina_hip_ctx *c, const KmerRequest &, const KmerLaunch &l, uint32_t q0, uint32_t bq, const uint32_t *range_n) override {
        SH_CHECK(hipMemcpyAsync(d_ids + (size_t)q0 * l.max, c->k_out_ids.p, (size_t)bq * l.max * 4, hipMemcpyDeviceToDevice, c->stream));
        SH_CHECK(hipMemcpyAsync(d_n + q0, c->k_out_n.p, (size_t)bq * 4, hipMemcpyDeviceToDevice, c->stream));
        memcpy(h_n + q0, range_n, (size_t)bq * 4);
        return 0;
    }
};
// sina_hip_kmer_topk_family: every range's candidates go through the family cascade where the select (and, for an
// identity limit, the match count) left them (family.hip), and nothing but the cascade's rows [nq][plan.row_words]
// comes to the host.  self: the queries' self lists (ids of 4 bytes; base null: none).
struct FamilySink : KmerSink {
    const sina_hip_family_rule *rule;
    FamilyPlan plan;
    KmerRagged self;
    KmerColumn rows;
    FamilySink(const sina_hip_family_rule *rule_, const FamilyPlan &plan_, const uint32_t *self_ids, const uint64_t *self_off, uint32_t *out_rows)
        : rule(rule_), plan(plan_), self{self_ids, self_off, 4}, rows{out_rows, (size_t)plan_.row_words * 4} {}
    bool msc() const { return rule->fs_msc_max < 1; }
    int check(sina_hip_ctx *c, const KmerRequest &r) const override {
        if (msc() && match_table_bytes(c->st->width) > kMatchMaxLds)
            SH_FAIL_LIMIT("kmer_topk_family: alignment too wide for the device match count");
        return family_check_self("kmer_topk_family", c, static_cast<const uint32_t *>(self.base), self.off, r.nq);
    }
    bool needs_bases() const override { return msc(); }
    int upload(sina_hip_ctx *c, uint32_t nq, hipStream_t s) override {  // the call's self lists, offsets from the first query's
        if (!self.base) return 0;
        std::vector<uint64_t> srel(nq + 1);
        for (uint32_t q = 0; q <= nq; q++) srel[q] = self.off[q] - self.off[0];
        return c->f_self_ids.reserve(4 * std::max<uint64_t>(srel[nq], 1)) || c->f_self_off.reserve(8 * ((uint64_t)nq + 1)) ||
               sina_hip::upload(c, 2, c->f_self_ids.p, static_cast<const uint32_t *>(self.base) + self.off[0], 4 * srel[nq], s) ||
               sina_hip::upload(c, 3, c->f_self_off.p, srel.data(), 8 * ((uint64_t)nq + 1), s);
    }
    bool all_or_nothing() const override { return true; }
    std::vector<KmerRagged *> inputs() override { return self.base ? std::vector<KmerRagged *>{&self} : std::vector<KmerRagged *>{}; }
    std::vector<KmerColumn *> columns() override { return {&rows}; }
    void empty(uint32_t nq) override {
        for (uint32_t q = 0; q < nq; q++) family_empty_row(rule, plan.row_words, rows.row<uint32_t>(q));
    }
    // the match counts if the rule has an identity limit, then the cascade
    int range(sina_hip_ctx *c, const KmerRequest &, const KmerLaunch &l, uint32_t q0, uint32_t bq, const uint32_t *h_n) override {
        if (msc() && range_match_counts(c, l, bq, nullptr, h_n)) return 1;
        return family_launch(c, c->k_out_ids.as<uint32_t>(), c->k_out_scores.as<float>(), c->m_out.as<uint16_t>(), c->k_out_n.as<uint32_t>(),
                             l.max, l.qoff, bq, rule, family_plan(rule->fs_min, rule->fs_max, rule->fs_req_full, rule->fs_cover_gene, bq),
                             self.base ? c->f_self_ids.as<uint32_t>() : nullptr, self.base ? c->f_self_off.as<uint64_t>() + q0 : nullptr, h_n,
                             rows.row<uint32_t>(q0));
    }
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

// The winners' rows in place of the select's, for as long as this lives: a sink reads a range's rows in c->k_out_ids,
// k_out_scores and k_out_n, and of a call that orients its queries those are the pick kernel's
struct PickedRows {
    sina_hip_ctx *c;
    explicit PickedRows(sina_hip_ctx *c_) : c(c_) { swap(); }
    ~PickedRows() { swap(); }
    PickedRows(const PickedRows &) = delete;
    PickedRows &operator=(const PickedRows &) = delete;
    void swap() {
        std::swap(c->k_out_ids, c->t_ids);
        std::swap(c->k_out_scores, c->t_scores);
        std::swap(c->k_out_n, c->t_n);
    }
};

// A range of a call that orients its queries, its select final (g, lv: the range and its launch, of virtual queries):
// the pick, the stagings that precede the sink's step -- of the picked rows -- the kernel's record, and the sink's step
// on a range of real queries
int turn_range(sina_hip_ctx *c, const KmerRequest &r, const KmerLaunch &lv, const KmerRange &g) {
    hipStream_t s = c->stream;
    const uint32_t n = r.turn_n, q0 = g.q0 / n, bq = g.bq / n, max = r.max;
    SH_CHECK(hipEventRecord(c->ev[6], s));
    if (turn_pick_launch(c, c->k_out_ids.as<uint32_t>(), c->k_out_scores.as<float>(), c->k_out_n.as<uint32_t>(), bq, n, max, s)) return 1;
    SH_CHECK(hipEventRecord(c->ev[7], s));
    const PickedRows picked(c);
    if ((r.sink->downloads_rows() && (download(c, 9, c->k_out_ids.p, (size_t)bq * max * 4, s) || download(c, 10, c->k_out_scores.p, (size_t)bq * max * 4, s))) ||
        download(c, 11, c->k_out_n.p, (size_t)bq * 4, s) || download(c, 6, c->t_meta.p, (size_t)bq * 20, s))
        return 1;
    SH_CHECK(wait_stream(c, s));
    float ms = 0;
    SH_CHECK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
    const uint32_t *meta = static_cast<const uint32_t *>(c->h_stage[6].p);
    uint64_t turned = 0;
    for (uint32_t q = 0; q < bq; q++) turned += meta[(size_t)5 * q] != 0;
    c->use[kUseTurn].add(ms, bq, turned, 1);
    const KmerLaunch l{c->t_src.as<uint8_t>(), c->t_qoff.as<uint64_t>() + q0, bq, max, lv.max_qlen, g.path, g.big};
    return r.sink->range(c, r, l, q0, bq, static_cast<const uint32_t *>(c->h_stage[11].p));
}

// One launch range: kernels, the lengths (and what the sink wants of the rows) back through pinned staging,
// statistics, the sink's step; *overflow = a candidate list of the range did not hold its query's candidates (the sink
// saw nothing of it then: the caller repeats the range with rows)
int run_range(sina_hip_ctx *c, const KmerRequest &r, const KmerRange &g, uint32_t max_qlen, bool *overflow) {
    hipStream_t s = c->stream;
    const uint32_t q0 = g.q0, bq = g.bq, max = r.max;
    const uint32_t per_query = r.turn_n ? r.turn_n : 1u;  // (a turn request: the range is of virtual queries, its rows are staged behind the pick)
    KmerLaunch l{c->qmask.as<uint8_t>(), c->k_qoff.as<uint64_t>() + q0, bq, max, max_qlen, g.path, g.big};
    if (run_kernels(c, l, true)) return 1;
    // (the kernels have finished: run_kernels waits for the heavy stream)
    if ((r.sink->downloads_rows() && !r.turn_n && (download(c, 9, c->k_out_ids.p, (size_t)bq * max * 4, s) || download(c, 10, c->k_out_scores.p, (size_t)bq * max * 4, s))) ||
        download(c, 11, c->k_out_n.p, (size_t)bq * 4, s) || download(c, 0, c->k_tmp2.p, 8, s))
        return 1;
    SH_CHECK(wait_stream(c, s));
    const uint32_t *h_n = static_cast<const uint32_t *>(c->h_stage[11].p);
    *overflow = false;
    if (g.path == kKmerCand)
        for (uint32_t q = 0; q < bq && !*overflow; q++) *overflow = h_n[q] == 0xFFFFFFFFu;
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
    if (g.path == kKmerLong) c->path_queries[kPathLong] += bq / per_query;
    if (g.big) c->path_queries[kPathBigSelect] += bq / per_query;
    if (r.turn_n) return turn_range(c, r, l, g);
    return r.sink->range(c, r, l, q0, bq, h_n);  // the range's select is final
}

// A call that orients its queries, behind its checks as kmer_topk_run's: the queries up once, as they are; their
// variants made where a search's queries lie; the ranges of virtual queries, whole queries each (turn_plan.h)
int kmer_turn_run(sina_hip_ctx *c, const KmerRequest &r, uint32_t n_fast) {
    const uint32_t nq = r.nq, n = r.turn_n, n_refs = c->st->n_refs;
    const uint64_t *qoff = r.qoff;
    uint32_t max_qlen = 1;
    for (uint32_t q = 0; q < n_fast; q++) max_qlen = std::max(max_qlen, r.qlen(q));
    hipStream_t s = c->stream;
    const uint64_t nqm = qoff[nq] - qoff[0];
    std::vector<uint64_t> rel(nq + 1);
    for (uint32_t q = 0; q <= nq; q++) rel[q] = qoff[q] - qoff[0];
    const std::vector<uint64_t> voff = turn_offsets(qoff, nq, n);
    if (c->t_src.reserve(turn_source_bytes(nqm)) || c->t_qoff.reserve(8 * rel.size()) || c->qmask.reserve(turn_variant_bytes(nqm, n)) ||
        c->k_qoff.reserve(8 * voff.size()))
        return 1;
    if (upload(c, 7, c->t_src.p, r.qmask + qoff[0], nqm, s) || upload(c, 4, c->t_qoff.p, rel.data(), 8 * rel.size(), s) ||
        upload(c, 8, c->k_qoff.p, voff.data(), 8 * voff.size(), s))
        return 1;
    if (r.sink->upload(c, nq, s)) return 1;
    // (a thin kernel beside whatever is resident: on the context's own stream)
    SH_CHECK(hipEventRecord(c->ev[6], s));
    if (turn_orient_launch(c, c->t_src.as<uint32_t>(), nqm, c->t_qoff.as<uint64_t>(), nq, n, c->qmask.as<uint8_t>(), s)) return 1;
    SH_CHECK(hipEventRecord(c->ev[7], s));
    SH_CHECK(wait_stream(c, s));
    float ms = 0;
    SH_CHECK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
    c->use[kUseTurn].add(ms, 0, 0, 1);
    // (SINA_HIP_TEST=turn_range=N: at most N queries per launch range, so that a small call takes several; the others
    // as kmer_topk_run reads them)
    uint64_t budget = kBigSelBudget;
    if (const std::string e_ = test_knob("big_sel_bytes"); !e_.empty()) budget = std::min<uint64_t>(kBigSelBudget, strtoull(e_.c_str(), nullptr, 10));
    const bool force_rows = atoi(test_knob("kmer_rows").c_str()) != 0;
    const uint32_t range_queries = (uint32_t)std::min<uint64_t>(strtoull(test_knob("turn_range").c_str(), nullptr, 10), kTurnMaxQueries);
    for (const KmerRange &g : turn_ranges(nq, n_fast, n, r.max, n_refs, budget, force_rows, range_queries)) {
        bool overflow = false;
        if (run_range(c, r, g, max_qlen, &overflow)) return 1;
        if (!overflow) continue;  // (kmer_topk_run: the score rows and the full select, a query's variants kept together)
        for (const KmerRange &h : turn_overflow_ranges(g, n, n_refs))
            if (run_range(c, r, h, max_qlen, &overflow)) return 1;
    }
    return 0;
}

// A call behind its checks (c->mu held, 1 <= max <= n_refs): the queries' masks and offsets, the packed bases and
// whatever else the sink needs to the device, then range by range as kmer_plan.h cuts them -- queries 0 .. n_fast - 1
// are at most kMaxQueryLen bases long, queries n_fast .. nq - 1 longer
int kmer_topk_run(sina_hip_ctx *c, const KmerRequest &r, uint32_t n_fast) {
    if (r.turn_n) return kmer_turn_run(c, r, n_fast);
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
    if (r.sink->needs_bases() && (c->s_qab.reserve(4 * std::max<uint64_t>(nqm, 1)) || upload(c, 1, c->s_qab.p, r.q_ab + qoff[0], 4 * nqm, s))) return 1;
    if (r.sink->upload(c, nq, s)) return 1;
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

// Storage of the call's own in place of the caller's, for as long as this lives: the sink's columns, zeroed, and -- for
// a call that runs in another order than the caller's -- its inputs gathered into that order (kmer_plan.h)
struct OwnRows {
    std::vector<KmerRagged *> ins;
    std::vector<KmerColumn *> cols;
    std::vector<KmerRagged> caller_ins;
    std::vector<KmerColumn> caller_cols;
    std::vector<std::vector<uint64_t>> off;
    std::vector<std::vector<uint8_t>> data;
    OwnRows(KmerRequest *r, const uint32_t *order) : ins(r->sink->inputs()), cols(r->sink->columns()) {
        const uint32_t nq = r->nq;
        if (order) {
            const KmerRagged mask{r->qmask, r->qoff, 1}, ab{r->q_ab, r->qoff, 4};
            r->qoff = own_offsets(mask, order, nq);
            r->qmask = own(mask, order, nq);
            if (r->sink->needs_bases()) r->q_ab = reinterpret_cast<const uint32_t *>(own(ab, order, nq));
            for (KmerRagged *in : ins) {
                caller_ins.push_back(*in);
                const uint64_t *in_off = own_offsets(*in, order, nq);
                *in = KmerRagged{own(*in, order, nq), in_off, in->elem};
            }
        }
        for (KmerColumn *col : cols) {
            caller_cols.push_back(*col);
            data.emplace_back((size_t)nq * col->bytes);
            col->base = data.back().data();
        }
    }
    // the rows to the caller's, row x to the caller's row order[x] (null: x)
    void scatter(const uint32_t *order, uint32_t nq) const {
        for (size_t i = 0; i < cols.size(); i++) kmer_scatter(*cols[i], caller_cols[i], order, nq);
    }
    ~OwnRows() {
        for (size_t i = 0; i < caller_ins.size(); i++) *ins[i] = caller_ins[i];
        for (size_t i = 0; i < caller_cols.size(); i++) *cols[i] = caller_cols[i];
    }
    OwnRows(const OwnRows &) = delete;
    OwnRows &operator=(const OwnRows &) = delete;

private:
    const uint64_t *own_offsets(const KmerRagged &in, const uint32_t *order, uint32_t nq) {
        off.push_back(kmer_gather_offsets(in.off, order, nq));
        return off.back().data();
    }
    // (after own_offsets of the same offsets)
    const uint8_t *own(const KmerRagged &in, const uint32_t *order, uint32_t nq) {
        data.push_back(kmer_gather(in, order, nq, off.back().data()));
        return data.back().data();
    }
};

// A call behind its checks, on the rows it works on.  On the caller's own, written range by range, where the queries
// run in the caller's order and the sink does not ask for more; else on columns of the call's own, which reach the
// caller's rows -- slot x the row of query order[x]; order null: of query x -- only if all of it succeeded.
int kmer_topk_on_rows(sina_hip_ctx *c, const KmerRequest &in, const std::vector<uint32_t> *order, uint32_t n_fast) {
    const auto answer = [&](const KmerRequest &r) {
        if (r.max) return kmer_topk_run(c, r, n_fast);
        r.sink->empty(r.nq);
        return 0;
    };
    if (!order && !in.sink->all_or_nothing()) return answer(in);
    KmerRequest r = in;
    const uint32_t *o = order ? order->data() : nullptr;
    const OwnRows own(&r, o);
    if (answer(r)) return 1;
    own.scatter(o, r.nq);
    return 0;
}

// any: queries of up to kMaxLongQueryLen bases (sina_hip_kmer_topk_any), the longer ones behind the others for
// kmer_topk_run and back into the caller's order
int kmer_topk_checked(sina_hip_ctx *c, const KmerRequest &in, bool any) {
    if (!c || !in.qmask || !in.qoff) SH_FAIL("kmer_topk: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    sina_hip_hint_guard hints(c);
    if (index_ready(c)) return 1;
    KmerRequest r = in;
    const uint32_t nq = r.nq;
    if (r.sink->check(c, r)) return 1;
    if (r.turn_n && r.sink->needs_bases()) SH_FAIL("kmer_topk: a call that orients its queries takes no sink that reads their packed bases");
    if (r.turn_n && nq > kTurnMaxQueries) SH_FAIL_LIMIT("kmer_topk_turn: more than 2^30 - 1 queries");
    if (nq == 0) return 0;
    SH_CHECK(hipSetDevice(c->device));
    if (r.max > c->st->n_refs) r.max = c->st->n_refs;
    r.sink->set_max(r.max);
    if (r.max == 0) return kmer_topk_on_rows(c, r, nullptr, nq);  // (no candidate: nothing is searched, no query too long)
    uint32_t n_long = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const uint64_t len = r.qoff[q + 1] - r.qoff[q];
        if (!any && len > (uint64_t)kMaxQueryLen) SH_FAIL("kmer_topk: query longer than SINA_HIP_MAX_QUERY_LEN bases");
        if (len > (uint64_t)kMaxLongQueryLen) SH_FAIL_LIMIT("kmer_topk_any: query longer than SINA_HIP_MAX_LONG_QUERY_LEN bases");
        n_long += len > (uint64_t)kMaxQueryLen;
    }
    if (n_long == 0) return kmer_topk_on_rows(c, r, nullptr, nq);
    uint32_t n_fast = 0;
    const std::vector<uint32_t> order = kmer_fast_first(r.qoff, nq, &n_fast);
    return kmer_topk_on_rows(c, r, &order, n_fast);
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

// A call that takes its queries as packed aligned bases: the mask bytes the count kernel reads, bits 24..31 of every
// word, and the queries' offsets from the first query's first base (q_ab + q_off[0] is what they index).  An
// uninitialised block and restrict pointers: on the family entry's default path, 41 candidates per query, this loop
// is most of what the entry costs (a zero-filled vector lost 2.6 ms per 4096 queries there).
struct PackedMasks {
    std::unique_ptr<uint8_t[]> mask;
    std::vector<uint64_t> rel;
    const uint32_t *bases;
    PackedMasks(const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq)
        : mask(new uint8_t[q_off[nq] - q_off[0] + 1]), rel(nq + 1), bases(q_ab + q_off[0]) {
        const uint64_t n_bases = q_off[nq] - q_off[0];
        const uint32_t *__restrict src = bases;
        uint8_t *__restrict dst = mask.get();
        for (uint64_t i = 0; i < n_bases; i++) dst[i] = (uint8_t)(src[i] >> 24);
        for (uint32_t q = 0; q <= nq; q++) rel[q] = q_off[q] - q_off[0];
    }
    KmerRequest request(uint32_t max, KmerSink *sink) const { return KmerRequest{mask.get(), rel.data(), (uint32_t)rel.size() - 1, max, bases, sink}; }
};

}  // namespace

int kmer_rows_resident(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t max, uint32_t *d_ids,
                       uint32_t *d_n, uint32_t *h_n) {
    if (index_ready(c)) return 1;
    if (nq == 0 || max == 0 || max > c->st->n_refs) SH_FAIL("kmer_rows_resident: nothing to search, or more rows than references");
    KeepSink keep(d_ids, d_n, h_n);
    return kmer_topk_run(c, KmerRequest{qmask, qoff, nq, max, nullptr, &keep}, nq);
}

}  // namespace sina_hip

using namespace sina_hip;

extern "C" {

int sina_hip_kmer_topk(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t max,
                       uint32_t *out_ids, float *out_scores, uint32_t *out_n) {
    if (!out_ids || !out_scores || !out_n) SH_FAIL("kmer_topk: null argument");
    PlainSink plain(out_ids, out_scores, out_n);
    return kmer_topk_checked(c, KmerRequest{qmask, qoff, nq, max, nullptr, &plain}, false);
}
int sina_hip_kmer_topk_any(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t max,
                           uint32_t *out_ids, float *out_scores, uint32_t *out_n) {
    if (!out_ids || !out_scores || !out_n) SH_FAIL("kmer_topk: null argument");
    PlainSink plain(out_ids, out_scores, out_n);
    return kmer_topk_checked(c, KmerRequest{qmask, qoff, nq, max, nullptr, &plain}, true);
}
int sina_hip_kmer_topk_turn(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t max, int all,
                            uint8_t *out_turn, float *out_top1, uint32_t *out_ids, float *out_scores, uint32_t *out_n) {
    if (!out_turn || !out_top1 || !out_ids || !out_scores || !out_n) SH_FAIL("kmer_topk_turn: null argument");
    if (max == 0) SH_FAIL("kmer_topk_turn: max must be 1 or more");
    if (test_knob("turn_fail") == "1") SH_FAIL("kmer_topk_turn: refused by the test knob turn_fail");
    TurnSink turn(out_turn, out_top1, out_ids, out_scores, out_n);
    KmerRequest r{qmask, qoff, nq, max, nullptr, &turn};
    r.turn_n = turn_variants(all != 0);
    return kmer_topk_checked(c, r, true);
}
int sina_hip_kmer_topk_match(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t max,
                             uint32_t *out_ids, float *out_scores, uint32_t *out_n, uint16_t *out_match) {
    if (!c || !q_ab || !q_off || !out_ids || !out_scores || !out_n || !out_match) SH_FAIL("kmer_topk_match: null argument");
    if (match_check_queries("kmer_topk_match", q_ab, q_off, nq)) return 1;
    const PackedMasks pm(q_ab, q_off, nq);
    MatchSink match(out_ids, out_scores, out_n, out_match);
    return kmer_topk_checked(c, pm.request(max, &match), true);
}
int sina_hip_kmer_topk_rank(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t kmer_candidates,
                            int iupac_rule, int filter_lowercase, int cover_rule, uint32_t max_result, uint32_t *out_ids,
                            float *out_scores, uint32_t *out_n, uint32_t *out_flag) {
    if (!c || !q_ab || !q_off || !out_ids || !out_scores || !out_n || !out_flag) SH_FAIL("kmer_topk_rank: null argument");
    if (match_check_queries("kmer_topk_rank", q_ab, q_off, nq)) return 1;
    const PackedMasks pm(q_ab, q_off, nq);
    RankSink rank(iupac_rule, filter_lowercase ? 1 : 0, cover_rule, max_result, out_ids, out_scores, out_n, out_flag);
    return kmer_topk_checked(c, pm.request(kmer_candidates, &rank), true);
}
int sina_hip_kmer_topk_family(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t max,
                              const sina_hip_family_rule *rule, const uint32_t *self_ids, const uint64_t *self_off, uint32_t *out_rows) {
    if (!c || !q_ab || !q_off || !rule || !out_rows || (!self_ids) != (!self_off)) SH_FAIL("kmer_topk_family: null argument");
    FamilyPlan plan;
    if (family_rule_plan("kmer_topk_family", rule, nq, &plan)) return 1;
    FamilySink family(rule, plan, self_ids, self_off, out_rows);
    if (family.msc() && match_check_queries("kmer_topk_family", q_ab, q_off, nq)) return 1;
    for (uint32_t q = 0; q < nq; q++)
        if (q_off[q + 1] < q_off[q]) SH_FAIL("kmer_topk_family: query offsets descend");
    const PackedMasks pm(q_ab, q_off, nq);
    return kmer_topk_checked(c, pm.request(max, &family), true);
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
