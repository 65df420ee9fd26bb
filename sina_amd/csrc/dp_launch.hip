// The host driver of the DP kernel: what a launch runs with (plan_dp, prune_plan, weights), one launch in named steps
// (run_dp_device), and the launch loop of the entries that align against device-built templates
// (align_family_batches).  No kernel lives here; the planning arithmetic is dp_plan.h.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "ctx.h"
#include "compare_dev.h"

namespace sina_hip {

// dp_geom_for (dp_plan.h) with the test hook read: SINA_HIP_TEST="geom=T,B" (used if it covers the batch's longest query)
bool pick_geom(uint32_t maxL, DpGeom *g) {
    int t = 0, b = 0;
    if (const std::string ov = test_knob("geom"); ov.empty() || sscanf(ov.c_str(), "%d,%d", &t, &b) != 2) t = b = 0;
    return dp_geom_for(maxL, t, b, g);
}

int plan_dp(sina_hip_ctx *c, uint32_t maxL, DpPlan *pl) {
    DpGeom g;
    if (!pick_geom(maxL, &g)) SH_FAIL_LIMIT("align: query longer than SINA_HIP_MAX_QUERY_LEN bases");
    dp_ring_plan(g, c->lds_budget, pl);
    if (pl->W < 1) SH_FAIL("align: LDS cannot hold one DP row");
    return 0;
}

// SINA_HIP_DP_PRUNE=0 switches the DP kernel's certified row skip off (every row of every strip is swept);
// SINA_HIP_TEST="rho=<x>" fixes the launches' guess of optimum / bound (tests: 2 = too bold for any query, every
// query takes the second attempt; 0.01 = nearly no bound).  Read per launch.
PrunePlan prune_plan(const sina_hip_align_params *p, float wmax, float wmin, uint32_t maxL, bool profile_batch) {
    const char *off = getenv("SINA_HIP_DP_PRUNE");
    DpGeom g;
    const bool single_strip = pick_geom(maxL, &g) && g.T <= 64;
    return prune_plan_for(p->match_score, p->mismatch_score, p->gap_penalty, p->gap_ext_penalty, weighted_scheme(p),
                          p->insertion == SINA_INSERTION_FORBID, profile_batch, wmax, wmin, maxL, off && off[0] == '0', single_strip);
}

int upload_weights(sina_hip_ctx *c, const sina_hip_align_params *p, uint32_t n_sets) {
    if (weighted_scheme(p)) {
        const size_t bytes = sizeof(float) * (size_t)p->n_weights * std::max<uint32_t>(n_sets, 1);
        if (c->weights.reserve(bytes)) return 1;
        SH_CHECK(hipMemcpyAsync(c->weights.p, p->weights, bytes, hipMemcpyHostToDevice, c->stream));
    }
    return 0;
}

// A set id out of range would read beyond the uploaded vectors: looked for before anything runs.  Not a limit of the
// path (no other entry takes such a call): a plain error.
int check_weight_sets(const char *who, const sina_hip_align_params *p, const uint32_t **weight_set, uint32_t *n_sets, uint32_t nq) {
    const std::string w(who);
    if (*n_sets == 0) SH_FAIL(w + ": n_sets must be at least 1");
    if (*weight_set != nullptr) {  // (else every query takes the first vector)
        if (!weighted_scheme(p)) SH_FAIL(w + ": weight sets need positional weights (p->weights, p->n_weights)");
        for (uint32_t q = 0; q < nq; q++)
            if ((*weight_set)[q] >= *n_sets)
                SH_FAIL(w + ": weight set " + std::to_string((*weight_set)[q]) + " of query " + std::to_string(q) +
                        " is not below n_sets = " + std::to_string(*n_sets));
    }
    if (*weight_set == nullptr || *n_sets == 1) {  // (one vector for all: the call of the entry without the suffix)
        *weight_set = nullptr;
        *n_sets = 1;
    }
    return 0;
}

namespace {

int reserve_launch_buffers(sina_hip_ctx *c, const DpPlan &pl, const DpLaunch &l, const LaunchSums &sums) {
    if (c->spill.reserve(std::max<uint64_t>(sums.spill_rows, 1) * 8 * (uint64_t)pl.geom.Lp()) ||
        c->edge.reserve(std::max<uint64_t>(1, (uint64_t)(pl.geom.T / 64 - 1) * sums.edge_entries) * sizeof(EdgeRec)) ||
        c->res.reserve(sizeof(DpResult) * l.bq) || c->out.reserve(sizeof(sina_hip_align_out) * l.bq) ||
        c->out_pos.reserve(4 * std::max<uint64_t>(l.nqm, 1)))
        return 1;
    for (InplaceCount &ic : c->inplace)
        if (ic.reserve(l.bq)) return 1;
    if (c->shift.reserve(l.bq) || reserve_rank_assembled(c, l.bq)) return 1;
    if (l.want_dbg_value && c->dbg.reserve(4 * sums.tb_cells)) return 1;
    return 0;
}

// longest queries first (workgroups start in index order; see mesh_dp_kernel)
int upload_order(sina_hip_ctx *c, const DpLaunch &l) {
    std::vector<uint32_t> order(l.bq);
    for (uint32_t q = 0; q < l.bq; q++) order[q] = q;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        return (uint64_t)l.qd[x].N * l.qd[x].L > (uint64_t)l.qd[y].N * l.qd[y].L;
    });
    if (c->order.reserve(4 * (size_t)l.bq)) return 1;
    return upload(c, 0, c->order.p, order.data(), 4 * (size_t)l.bq, c->stream);
}

// The kernels' arguments -- all but the bound (choose_bound), the plane and the dry signal (launch_dp_and_walk).
int fill_args(sina_hip_ctx *c, const DpPlan &pl, const PrunePlan &pp, const sina_hip_align_params *p, const DpLaunch &l,
              const LaunchSums &sums, DpArgs *a, BtArgs *b) {
    const bool weighted = weighted_scheme(p), forbid = p->insertion == SINA_INSERTION_FORBID;
    a->qd = c->qd.as<QDesc>();
    a->order = c->order.as<uint32_t>();
    a->rec = c->rec.as<uint4>();
    a->pred = c->pred.as<uint32_t>();
    a->node_pos = c->node_pos.as<uint32_t>();
    a->succ_minpos = c->succ_minpos.as<uint32_t>();
    a->qmask = c->qmask.as<uint8_t>();
    a->dbg_value = l.want_dbg_value ? c->dbg.as<float>() : nullptr;
    a->spill = c->spill.as<float>();
    a->edge = c->edge.as<EdgeRec>();
    a->edge_stride = sums.edge_entries;
    a->res = c->res.as<DpResult>();
    a->weights = weighted ? c->weights.as<float>() : nullptr;
    a->n_weights = weighted ? p->n_weights : 0;
    if (weighted && l.wset != nullptr) {  // (indexed like qd: the launch's own reordering goes through `order`)
        if (c->wset.reserve(4 * (size_t)l.bq)) return 1;
        if (upload(c, 9, c->wset.p, l.wset, 4 * (size_t)l.bq, c->stream)) return 1;
        a->wset = c->wset.as<uint32_t>();
    }
    a->ms = -p->match_score;  // scoring_scheme_*(-match, -mismatch, gap, gapext), align.cpp:406-414
    a->mms = -p->mismatch_score;
    a->gp = p->gap_penalty;
    a->gpe = p->gap_ext_penalty;
    a->prof16 = l.profile_batch ? c->prof16.as<float>() : nullptr;
    c->last_bq = l.bq;
    c->last_prune_step = pp.on ? pp.amax : 0u;
    a->reach = pp.on ? c->rgain.as<uint2>() : nullptr;
    a->prune = pp.on;
    a->prune_amax = pp.amax;
    a->below_init = (!weighted && !forbid && dp_below_init(sums.max_n, a->gp, a->gpe)) ? 1 : 0;
    b->qd = a->qd;
    b->rec = a->rec;
    b->pred = a->pred;
    b->pred4 = c->pred4.as<uint2>();
    b->node_pos = a->node_pos;
    b->res = a->res;
    b->weights = a->weights;
    b->n_weights = a->n_weights;
    b->wset = a->wset;
    b->out = c->out.as<sina_hip_align_out>();
    b->out_pos = c->out_pos.as<uint32_t>();
    b->nq = l.bq;
    b->width = l.width;
    b->Lp = (uint32_t)pl.geom.Lp();
    b->ms = a->ms;
    b->overhang = p->overhang;
    b->lazy_sidx = forbid ? 0 : 1;
    b->qmask = a->qmask;
    b->lowercase = p->lowercase;
    b->self16 = l.profile_batch ? c->self16.as<float>() : nullptr;
    b->asm_cap = sums.max_l;
    // (assemble = 2 outside an entry that opened the shift log -- the plane debug entries -- would have nowhere to
    // write its events: refused, not run as assemble = 1)
    if (p->assemble == SINA_ASSEMBLE_SHIFT && !c->shift.active) SH_FAIL("align: this entry takes no assemble = 2 (no shift log is staged)");
    b->shift_log = p->assemble == SINA_ASSEMBLE_SHIFT ? c->shift.rows.as<uint32_t>() : nullptr;
    return 0;
}

// Certified row skip (mesh_dp.hip): the guess the launch's queries start with -- what the store has learnt from the
// queries before, or SINA_HIP_TEST=rho=<x> -- and whether its waves run the scout pass.
int choose_bound(sina_hip_ctx *c, const DpPlan &pl, const PrunePlan &pp, const sina_hip_align_params *p, const DpLaunch &l,
                 DpArgs *a) {
    const bool weighted = weighted_scheme(p), forbid = p->insertion == SINA_INSERTION_FORBID;
    hipStream_t s = c->stream;
    bool rho_fixed = false;
    if (pp.on) {
        if (const std::string r = test_knob("rho"); !r.empty()) {
            a->prune_rho = (float)atof(r.c_str());
            rho_fixed = a->prune_rho > 0.f;
        }
        if (!rho_fixed) {  // (the guess a launch without a scout starts from; one WITH a scout takes the guard, below)
            std::lock_guard<std::mutex> slk(c->st->stats_mu);
            a->prune_rho = c->st->prune_rho;
        }
    }
    // The scout pass (mesh_dp.hip, chain_scout_wave): every query's own bound U -- the cost of a real path, its alignment
    // against the chain of its family's first member -- instead of the store's guess alone.  It is the first thing the
    // query's DP wave does: no launch, no event and nothing for the host to wait for.  A fixed guess
    // (SINA_HIP_TEST=rho=) or SINA_HIP_TEST=scout=0 leaves it out, and so does a caller that brought its own DAGs
    // (sina_hip_align_graphs: no family to take a chain from).
    a->scout_bias = (float)atof(test_knob("scout_add").c_str());
    c->last_scout = false;
    if (const std::string fixed = test_knob("scout_set"); !fixed.empty() && pp.on && !rho_fixed) {
        // (test hook: every query's scout value is this number -- lets a caller-built DAG, which has no family to take
        // a chain from, run under a chosen bound: tests/test_gpu_prune.py)
        std::vector<float> vals(l.bq, (float)atof(fixed.c_str()));
        if (c->scout_u.reserve(4 * (size_t)l.bq)) return 1;
        if (upload(c, 7, c->scout_u.p, vals.data(), 4 * (size_t)l.bq, s)) return 1;
        a->scout_u = c->scout_u.as<float>();
        c->last_scout = true;
    } else if (scout_allowed(l.chain_ncap != 0, weighted, forbid, pp.on != 0, rho_fixed, a->below_init != 0, a->gp, a->gpe, pl.geom.T,
                             test_knob("scout") == "0", atoi(test_knob("generic").c_str()) != 0)) {
        if (c->scout_u.reserve(4 * (size_t)l.bq)) return 1;
        a->scout_u = c->scout_u.as<float>();
        a->chain_rows = c->scout.as<uint16_t>();
        a->chain_sizes = c->g_sizes.as<uint32_t>();
        a->chain_ncap = l.chain_ncap;
        c->last_scout = true;
        std::lock_guard<std::mutex> slk(c->st->stats_mu);
        c->st->stats.scout_launches++;  // (DP launches whose waves ran the pass; it has no time of its own: scout_ms stays 0)
    }
    if (a->scout_u != nullptr && !rho_fixed) {
        std::lock_guard<std::mutex> slk(c->st->stats_mu);
        a->prune_rho = c->st->prune_rho_guard;
    }
    return 0;
}

// The in-place counts of a call that counts them (ctx.h, align_call): right behind the assembly, on its stream, over
// the words it left -- the pair count, then the family identity, then the search stage's ranking.  Like launch_assemble they take no part in the FIFO's
// dry signal -- the DP kernel gives that --, and each records its own event behind its kernel: from the event before
// it (ev[2], the walk's and the assembly's end, or the event of the count that ran before) to that one is its own time
// (account_launch).
// Ordering: the identity kernel reads g_fam_ids / g_fam_off as the chunk's build uploaded them, and the next chunk's
// build uploads over them.  That upload is issued by this host thread, and only after run_dp_device has returned for the
// chunk's last range: in the chained branch heavy_launch::done() has the host wait for an event recorded on the FIFO
// stream BEHIND this kernel, in the other branch the kernel goes to stream_dp and fetch_results waits for that stream
// -- either way the kernel has ended before the range's results are down, and the context's mutex keeps every other
// call off these buffers meanwhile.  The uploads between the build and the chunk's last range (qd, qmask, wset,
// order, scout values) go to other buffers.
static int launch_inplace_counts(sina_hip_ctx *c, const BtArgs &b, const DpLaunch &l, hipStream_t s) {
    InplaceCount &pc = c->inplace[kInplacePairs], &id = c->inplace[kInplaceIdentity], &rk = c->inplace[kInplaceRank];
    if (pc.active) {
        if (launch_pair_count_assembled(b, c->st->pair_ent.p, c->st->n_pair_ent, pc.rows.as<uint32_t>(), s)) return 1;
        SH_CHECK(hipEventRecord(c->ev[pc.ev], s));
    }
    if (id.active) {
        if (launch_family_identity(c, b, l.fam_ncap, b.asm_cap, id.rows.as<uint32_t>(), s)) return 1;
        SH_CHECK(hipEventRecord(c->ev[id.ev], s));
    }
    if (rk.active) {  // (reads the call's candidate rows: searched, and copied on c->stream, before this launch was queued)
        if (launch_rank_assembled(c, b, l.q_base, b.asm_cap, rk.rows.as<uint32_t>(), s)) return 1;
        SH_CHECK(hipEventRecord(c->ev[rk.ev], s));
    }
    return 0;
}

// Queues the DP kernel, the walk and the assembly; *dp_no: this launch's number among the store's DP launches (~0: none).
// With chained launches the walk and the assembly are queued right behind their DP kernel on the same FIFO stream: they
// start the moment it ends, run beside the launch that started in its drain (the other FIFO stream), and the launch
// after that -- often the next DP launch -- is ordered behind them by the stream itself.  A walk the host launches on the
// context's stream once it has seen the kernel end can be late: if its hardware queue shares a dispatch pipe with the
// FIFO's it starts 5 ms late, beside the NEXT DP launch, takes 17 ms there instead of 3 and stretches that launch by 10
// (profiles/r04_bt_delay.txt).  A launch that is not chained walks on stream_dp.
int launch_dp_and_walk(sina_hip_ctx *c, const DpPlan &pl, const sina_hip_align_params *p, const DpLaunch &l, DpArgs &a, const BtArgs &b,
                       uint64_t *dp_no) {
    const bool weighted = weighted_scheme(p), forbid = p->insertion == SINA_INSERTION_FORBID;
    bool bt_done = false;
    hipStream_t s = c->stream_dp;
    {
        // the DP kernel: on the store's heavy stream, behind the uploads queued on c->stream; the result copies
        // then follow it on the context's stream_dp
        SH_CHECK(hipEventRecord(c->ev[8], c->stream));
        SH_CHECK(hipStreamWaitEvent(s, c->ev[8], 0));
        heavy_launch hl(c, s, kHeavyDp);
        SH_CHECK(hipEventRecord(c->ev[0], hl.stream()));
        a.dry = hl.dry();
        if (launch_mesh_dp(pl.geom, weighted, forbid, a, b.nq, pl.lds, hl.stream(), &c->last_kernel)) return 1;
        SH_CHECK(hipEventRecord(c->ev[1], hl.stream()));
        if (hl.lk.owns_lock() && c->st->dp_end[0]) {  // (under the queue's lock: launch order = dp_seq order)
            *dp_no = c->st->dp_seq++;
            SH_CHECK(hipEventRecord(c->st->dp_end[*dp_no % 8], hl.stream()));
            c->st->dp_end_no[*dp_no % 8].store(*dp_no, std::memory_order_release);
        }
        if (hl.chained) {
            if (launch_backtrack(b, hl.stream())) return 1;
            if (p->assemble && launch_assemble(b, hl.stream())) return 1;
            SH_CHECK(hipEventRecord(c->ev[2], hl.stream()));
            if (p->assemble && launch_inplace_counts(c, b, l, hl.stream())) return 1;
            bt_done = true;
        }
        if (hl.done()) return 1;
    }
    if (!bt_done) {
        if (launch_backtrack(b, s)) return 1;
        if (p->assemble && launch_assemble(b, s)) return 1;
        SH_CHECK(hipEventRecord(c->ev[2], s));
        if (p->assemble && launch_inplace_counts(c, b, l, s)) return 1;
    }
    return 0;
}

// (h_out_pos was sized for the whole call by the entry point; this range's columns go to their place in it -- and so
// do its rows of the in-place counts, InplaceCount::copy, if the call counts them)
int fetch_results(sina_hip_ctx *c, const DpLaunch &l) {
    hipStream_t s = c->stream_dp;
    if (c->h_out.reserve(sizeof(sina_hip_align_out) * l.bq) || c->h_res.reserve(sizeof(DpResult) * l.bq)) return 1;
    unsigned char *staged_pos = static_cast<unsigned char *>(c->h_out_pos.p) + 4 * l.out_pos_base;
    SH_CHECK(hipMemcpyAsync(c->h_out.p, c->out.p, sizeof(sina_hip_align_out) * l.bq, hipMemcpyDeviceToHost, s));
    SH_CHECK(hipMemcpyAsync(c->h_res.p, c->res.p, sizeof(DpResult) * l.bq, hipMemcpyDeviceToHost, s));
    SH_CHECK(hipMemcpyAsync(staged_pos, c->out_pos.p, 4 * l.nqm, hipMemcpyDeviceToHost, s));
    for (InplaceCount &ic : c->inplace)
        if (ic.copy(l.q_base, l.bq, s)) return 1;
    if (c->shift.copy(l.q_base, l.bq, s)) return 1;
    SH_CHECK(wait_stream(c, s));
    memcpy(l.out, c->h_out.p, sizeof(sina_hip_align_out) * l.bq);
    if (l.out_pos) memcpy(l.out_pos, staged_pos, 4 * l.nqm);
    return 0;
}

// folds the launch into the store's statistics and its two guesses of optimum / bound
int account_launch(sina_hip_ctx *c, const DpPlan &pl, const sina_hip_align_params *p, const DpLaunch &l, uint64_t cells, uint64_t dp_no) {
    float ms = 0;
    SH_CHECK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    // ... of which this launch shared the device with the DP launch before it (chained launches, ctx.h)
    float shared = 0;
    // (the ring has eight slots and this thread reads it outside the queue's lock: a slot that has been re-recorded by
    // launch dp_no + 7 meanwhile is not the predecessor's any more -- its number says so -- and counts as no overlap,
    // as does a predecessor that has not ended yet: a short launch can end before the drain of the one before it)
    if (dp_no != ~0ull && dp_no > 0 && c->st->dp_end_no[(dp_no - 1) % 8].load(std::memory_order_acquire) == dp_no - 1) {
        float to_prev_end = 0;
        const hipError_t e = hipEventElapsedTime(&to_prev_end, c->ev[0], c->st->dp_end[(dp_no - 1) % 8]);
        if (e == hipSuccess && c->st->dp_end_no[(dp_no - 1) % 8].load(std::memory_order_acquire) == dp_no - 1)
            shared = std::min(ms, std::max(0.f, to_prev_end));
        else (void)hipGetLastError();
    }
    SweepSummary sw = summarise_sweep(l.qd, c->h_res.as<DpResult>(), l.bq, 64u * (uint32_t)pl.geom.B);
    std::lock_guard<std::mutex> slk(c->st->stats_mu);
    sina_hip_stats &st = c->st->stats;
    st.dp_ms += ms;
    st.dp_busy_ms += ms - shared;
    SH_CHECK(hipEventElapsedTime(&ms, c->ev[1], c->ev[2]));
    st.backtrack_ms += ms;
    // (the context's own counters: its caller holds its mutex.  An in-place kernel's time runs from the last event
    // recorded before it -- the assembly's, or the count's that ran before -- to its own)
    int ev_before = 2;
    for (const InplaceCount &ic : c->inplace) {
        if (!ic.active) continue;
        SH_CHECK(hipEventElapsedTime(&ms, c->ev[ev_before], c->ev[ic.ev]));
        c->use[ic.kernel].add(ms, 0, 0, 1);
        ev_before = ic.ev;
    }
    // (their volumes: the assembled queries, and for the identity those queries' family pairs)
    auto assembled = [&](uint32_t q) { return l.out[q].status == 0 && l.out[q].assembled != 0; };
    if (c->inplace[kInplacePairs].active)
        for (uint32_t q = 0; q < l.bq; q++) c->use[kUsePairsInplace].a += assembled(q) ? 1u : 0u;
    if (c->inplace[kInplaceIdentity].active)
        for (uint32_t q = 0; q < l.bq; q++)
            if (assembled(q)) {
                c->use[kUseIdentityInplace].a++;
                c->use[kUseIdentityInplace].b += l.fam_off ? l.fam_off[q + 1] - l.fam_off[q] : 0;
            }
    if (c->inplace[kInplaceRank].active)  // (the rows are down: fetch_results; a ranked query's candidates were all scored)
        for (uint32_t q = 0; q < l.bq; q++) {
            const uint32_t *row = c->inplace[kInplaceRank].h_rows.as<uint32_t>() + (RankRider::row_bytes / 4) * (l.q_base + q);
            if (!(row[1] & 2u)) continue;
            const uint32_t n = c->rider.h_n[l.q_base + q];
            c->use[kUseRankInplace].a++;
            c->use[kUseRankInplace].b += n == 0xFFFFFFFFu ? 0u : std::min(n, c->rider.stride);
        }
    if (p->assemble) {  // (sina_hip_assemble_stats)
        c->asm_use.queries += l.bq;
        for (uint32_t q = 0; q < l.bq; q++) {
            if (!assembled(q)) continue;
            c->asm_use.assembled++;
            const uint32_t runs = c->shift.active ? c->shift.row(l.q_base + q)[0] : 0u;
            c->asm_use.shifted_queries += runs != 0 ? 1u : 0u;
            c->asm_use.shifted_runs += runs;
        }
    }
    st.dp_cells += cells;
    st.dp_launches++;
    st.dp_rows += sw.rows_nominal;
    st.dp_rows_swept += sw.rows_swept;
    st.dp_cells_swept += sw.cells_swept;
    st.dp_queries_pruned += sw.n_pruned;
    st.dp_second_attempts += sw.n_second;
    st.dp_full_sweeps += sw.n_full;
    update_rho(&c->st->prune_rho, &c->st->prune_rho_guard, sw.ratios);
    st.dp_prune_rho = c->st->prune_rho;
    return 0;
}

}  // namespace

// Whether this call ranks, and if it does its candidates.  What the store or the call lacks never fails the call: it
// then runs as without the switch and stages nothing.  (A call with a query beyond the fast k-mer count kernel's
// length -- sina_hip_align_graphs_any alone takes one -- does not rank either: its queries go the caller's own way.)
int align_call::begin_rank(const sina_hip_align_params *p, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq) {
    InplaceCount &rk = c->inplace[kInplaceRank];
    const sina_hip_store *st = c->st;
    RankRider &rr = c->rider;
    if (!rk.on || !p || !p->assemble || !qmask || !qoff || nq == 0) return 0;
    if (!st->have_refs || st->n_refs == 0 || !st->have_name_order || !st->have_index || st->k != rr.k || st->nofast != rr.nofast) return 0;
    const uint32_t stride = std::min(rr.cands, st->n_refs);
    if (stride == 0 || kmer_big_select(stride)) return 0;
    uint32_t max_l = 0;
    for (uint32_t q = 0; q < nq; q++) {
        if (qoff[q + 1] <= qoff[q] || qoff[q + 1] - qoff[q] > (uint64_t)SINA_HIP_MAX_QUERY_LEN) return 0;
        max_l = std::max<uint32_t>(max_l, (uint32_t)(qoff[q + 1] - qoff[q]));
    }
    if (compare_table_bytes(st->width, max_l) > kCompareMaxLds) return 0;
    SH_CHECK(hipSetDevice(c->device));
    rr.stride = stride;
    rr.h_n.assign(nq, 0);
    if (rr.ids.reserve(4 * (size_t)nq * stride) || rr.n.reserve(4 * (size_t)nq)) return 1;
    if (kmer_rows_resident(c, qmask, qoff, nq, stride, rr.ids.as<uint32_t>(), rr.n.as<uint32_t>(), rr.h_n.data())) return 1;
    return rk.begin(true, nq);
}

int run_dp_device(sina_hip_ctx *c, const DpPlan &pl, const PrunePlan &pp, const sina_hip_align_params *p, const DpLaunch &l) {
    const bool forbid = p->insertion == SINA_INSERTION_FORBID;
    const LaunchSums sums = launch_sums(l.qd, l.bq, pl.geom.Lp());
    DpArgs a{};  // (every pointer null, every number 0 until a step says otherwise)
    BtArgs b{};
    if (reserve_launch_buffers(c, pl, l, sums) || upload_order(c, l) || fill_args(c, pl, pp, p, l, sums, &a, &b) ||
        choose_bound(c, pl, pp, p, l, &a))
        return 1;
    // The trace-back plane is the one buffer whose size follows the batch (tens of GB for 16S): borrowed
    // from the device's pool of two (ctx.h) until this launch's results are on the host.
    tb_plane_lease plane;
    if (plane.acquire(c, std::max<uint64_t>(tb_cell_bytes(forbid) * sums.tb_cells, 16))) return 1;
    b.tb = c->last_tb = a.tb = plane.ptr;
    // (rows the kernel never visits show the value a skipped row shows its successors)
    if (l.want_dbg_value && pp.on)
        SH_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->dbg.p), 0x49742400 /* 1e6f */, sums.tb_cells, c->stream));
    // (debug read-back of the planes: rows the kernel skips leave their trace-back cells unwritten -- "untouched cell"
    // everywhere first, so that unpacking them stays inside the DAG)
    if (l.debug_planes && !forbid)
        SH_CHECK(hipMemsetD16Async(reinterpret_cast<hipDeviceptr_t>(plane.ptr), (unsigned short)kTbNone, sums.tb_cells, c->stream));
    uint64_t dp_no = ~0ull;
    if (launch_dp_and_walk(c, pl, p, l, a, b, &dp_no) || fetch_results(c, l)) return 1;
    return account_launch(c, pl, p, l, sums.cells, dp_no);
}

int align_family_batches(sina_hip_ctx *c, const FamilyCall &f) {
    const std::string w(f.who);
    const sina_hip_align_params *p = f.p;
    const uint64_t *qoff = f.qoff, *fam_off = f.fam_off;
    const uint32_t nq = f.nq;
    if (!c || !f.fam_ids || !fam_off || !f.qmask || !qoff || !p || !f.out)
        SH_FAIL(w + ": null argument");
    const uint32_t *weight_set = f.weight_set;
    uint32_t n_sets = f.n_sets;
    if (check_weight_sets(f.who, p, &weight_set, &n_sets, nq)) return 1;
    align_call call(c);  // (nothing counts until call.begin below: a call that ends early has counted nothing)
    sina_hip_hint_guard hints(c);
    if (!c->st->have_refs) SH_FAIL(w + ": upload references first");
    if (nq == 0) return 0;
    SH_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (c->st->width > 524288u) SH_FAIL_LIMIT(w + ": alignment wider than 524288 columns (use align_graphs)");
    // (scoring_scheme_profile takes no positional weights, src/align.cpp:428-433: refused like a profile batch of align_graphs)
    if (f.profile_batch && weighted_scheme(p)) SH_FAIL(w + ": a profile batch takes no positional weights (scoring_scheme_profile)");
    uint32_t maxL = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const uint64_t L = qoff[q + 1] - qoff[q], F = fam_off[q + 1] - fam_off[q];
        if (L == 0 || L > 65535) SH_FAIL(w + ": query length must be in 1..65535");
        if (F == 0 || F > (uint64_t)kFamilyMax) SH_FAIL(w + ": family size must be in 1..128");
        maxL = std::max<uint32_t>(maxL, (uint32_t)L);
    }
    DpPlan pl;
    if (plan_dp(c, maxL, &pl)) return 1;
    const int Lp = pl.geom.Lp();
    if (upload_weights(c, p, n_sets)) return 1;
    if (c->h_out_pos.reserve(4 * std::max<uint64_t>(qoff[nq] - qoff[0], 1))) return 1;
    if (call.begin(kMayCountPairs | kMayCountIdentity, p, nq) || call.begin_rank(p, f.qmask, qoff, nq)) return 1;
    // (SINA_HIP_TEST=dp_range_q=N: at most N queries per DP launch range, so that a small call takes several;
    // fam_chunk_q=N: at most N queries per build chunk, so that it spans several builds)
    const uint32_t range_q = (uint32_t)strtoul(test_knob("dp_range_q").c_str(), nullptr, 10);
    const uint32_t forced_chunk_q = (uint32_t)strtoul(test_knob("fam_chunk_q").c_str(), nullptr, 10);

    const uint64_t tb_budget_cells = tb_plane_budget(c) / tb_cell_bytes(p->insertion == SINA_INSERTION_FORBID);
    // queries per DAG build and DP launch: up to three rounds of DP wave slots (one DP wave per query) -- a DP
    // launch ends with ~4.4 ms of draining device whatever its size, so a third round makes it 3 % faster per
    // query than two (a fourth adds 2 % and another 22 GB per trace-back plane); the DP
    // launches below are whole rounds where the trace-back budget cuts a chunk
    const uint32_t slots = dp_wave_slots(c, pl.geom.B);
    const uint32_t chunk_q = forced_chunk_q != 0 ? std::min(forced_chunk_q, 3 * slots) : 3 * slots;
    BuiltGraphs bg;
    std::vector<uint32_t> dag_of;      // per query of the chunk: which of the chunk's distinct DAGs is its family's
    std::vector<uint32_t> ufam_ids;    // the distinct families, concatenated
    std::vector<uint64_t> ufam_off;
    std::vector<QDesc> qd;
    for (uint32_t q0 = 0; q0 < nq; q0 += chunk_q) {
        const uint32_t bq = std::min(chunk_q, nq - q0);
        // Queries with the same ORDERED family share one DAG (node order, weights, predecessor lists and the DP's
        // row-slot assignment depend on nothing else): amplicons of one region against one reference clade.  The
        // DAG is built once per distinct family of the chunk; every query keeps its own trace-back cells, spill
        // rows and edge records -- and its own positional weights (weight_set): the DAG holds none.
        const uint32_t n_dags = distinct_families(f.fam_ids, fam_off, q0, bq, &dag_of, &ufam_ids, &ufam_off);
        const bool packed = n_dags < bq;  // (the distinct families, packed for the build)
        // (certified row skip of the DP kernel: the DAG build adds every node's bound on the gain still to come; a
        // profile launch runs without it and without the scout)
        PrunePlan pp;
        if (!f.profile_batch)
            pp = prune_plan(p, (float)(1.0 / (double)(p->fs_weight + 1) + (double)p->fs_weight), p->fs_weight >= 0.f ? 0.f : -1.f, maxL, false);
        if (f.build(c, packed ? ufam_ids.data() : f.fam_ids, packed ? ufam_off.data() : fam_off, packed ? 0 : q0, n_dags, p, pl.W, pp, &bg))
            return 1;
        {
            std::lock_guard<std::mutex> slk(c->st->stats_mu);
            c->st->stats.dags_built += n_dags;
            c->st->stats.dags_used += bq;
        }
        // DP in sub-ranges that fit the trace-back budget
        auto nodes_of = [&](uint32_t r) { return bg.sizes[(size_t)kBuiltWords * dag_of[r] + kBuiltN]; };
        for (uint32_t r0 = 0, r1; r0 < bq; r0 = r1) {
            r1 = dp_cut_range(nodes_of, r0, bq, Lp, tb_budget_cells, slots);
            if (range_q != 0) r1 = std::min(r1, r0 + range_q);
            family_qdescs(bg, dag_of.data(), qoff, q0, r0, r1, Lp, &qd);
            const uint32_t rq = r1 - r0;
            const uint64_t qbase = qoff[q0 + r0], nqm = qoff[q0 + r1] - qbase;
            if (c->qd.reserve(sizeof(QDesc) * rq) || c->qmask.reserve(std::max<uint64_t>(nqm, 1))) return 1;
            if (upload(c, 5, c->qd.p, qd.data(), sizeof(QDesc) * rq, s) || upload(c, 6, c->qmask.p, f.qmask + qbase, nqm, s))
                return 1;
            DpLaunch l;
            l.qd = qd.data();
            l.bq = rq;
            l.nqm = nqm;
            l.width = c->st->width;
            l.out = f.out + q0 + r0;
            l.out_pos = f.out_pos ? f.out_pos + qbase : nullptr;
            l.out_pos_base = qbase - qoff[0];
            l.q_base = q0 + r0;
            l.profile_batch = f.profile_batch;  // (the DP reads the builder's prof16, the walk the entry point's self16)
            l.chain_ncap = f.profile_batch ? 0u : bg.ncap;
            l.wset = weight_set ? weight_set + q0 + r0 : nullptr;
            l.fam_ncap = bg.ncap;
            l.fam_off = fam_off + q0 + r0;
            if (run_dp_device(c, pl, pp, p, l)) return 1;
        }
    }
    return 0;
}

}  // namespace sina_hip
