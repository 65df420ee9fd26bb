// What a DP launch is planned from, as plain host code: no HIP runtime call, no context, no environment -- every
// function here runs (and is tested: tests/dp_plan_check.cpp) without a device.  dp_launch.hip, api.hip and the launchers (mesh_dp.hip, traceback.hip) call them.
#pragma once

#include <cassert>
#include <cmath>
#include <cstring>
#include <string_view>
#include <unordered_map>

#include "common.h"

namespace sina_hip {

// ---- the gates: which DP kernel a launch runs, whether it may skip rows, whether its waves scout
// (tests/gate_check.cpp states each rule a second time, from the outside, and compares)
// The kernel of a launch (mesh_dp.hip, launch_tb; reported as sina_hip_dp_info::kernel -- the numbers are
// SINA_DP_KERNEL_* of sina_hip.h).  The specialised kernel takes the simple scheme with gap_open >= gap_extend in a
// launch below the initial value (every BASELINE configuration), with the certified row skip where the launch has a
// bound and two strips or more -- in a single strip column 0, where an alignment may start at any row for free,
// keeps every row in play.  Everything else is an instance of the generic kernel.
enum DpKernelKind : uint32_t {
    kDpKernelNone = SINA_DP_KERNEL_NONE,
    kDpKernelSimple = SINA_DP_KERNEL_SIMPLE,
    kDpKernelSimpleSkip = SINA_DP_KERNEL_SIMPLE_SKIP,
    kDpKernelGenericBelow = SINA_DP_KERNEL_GENERIC_BELOW,  // mesh_dp_kernel<B, false, false, true>
    kDpKernelGeneric = SINA_DP_KERNEL_GENERIC,             // <B, false, false, false>
    kDpKernelWeighted = SINA_DP_KERNEL_WEIGHTED,           // <B, true, false, false>
    kDpKernelForbid = SINA_DP_KERNEL_FORBID,               // <B, false, true, false>
    kDpKernelWeightedForbid = SINA_DP_KERNEL_WEIGHTED_FORBID,
};
inline DpKernelKind dp_kernel_kind(bool weighted, bool forbid, bool below_init, float gp, float gpe, bool generic_only,
                                   bool profile_batch, bool prune_on, uint32_t n_strips) {
    if (!weighted && !forbid && below_init && gp >= gpe && !generic_only && !profile_batch)
        return (prune_on && n_strips >= 2) ? kDpKernelSimpleSkip : kDpKernelSimple;
    if (!weighted && !forbid) return below_init ? kDpKernelGenericBelow : kDpKernelGeneric;
    if (weighted) return forbid ? kDpKernelWeightedForbid : kDpKernelWeighted;
    return kDpKernelForbid;
}

// The arithmetic of prune_plan (dp_launch.hip, which reads the environment and the geometry): what a launch may prune
// with.  env_off: SINA_HIP_DP_PRUNE=0; single_strip: the launch's geometry has one strip.
inline PrunePlan prune_plan_for(float match, float mismatch, float gp, float gpe, bool weighted, bool forbid,
                                bool profile_batch, float wmax, float wmin, uint32_t maxL, bool env_off, bool single_strip) {
    PrunePlan pp;
    if (!std::isfinite(wmax) || !std::isfinite(wmin)) return pp;  // (a NaN weight: no bound holds)
    if (env_off) return pp;
    if (profile_batch || weighted || forbid) return pp;
    // gaps must cost, node weights must not be negative (a match gains match_score * weight, nothing else gains)
    if (!(gp >= 0.f) || !(gpe >= 0.f) || !(wmin >= 0.f)) return pp;
    const float kappa = std::max(0.f, std::max(match, mismatch));
    if (!std::isfinite(kappa)) return pp;
    pp.kappa64 = 64.0f * 1.0001f * kappa;
    pp.amax = prune_gain_units(wmax, pp.kappa64);
    // (the bounds are exact float32 integers in units of 1/64 only below 2^24)
    if (pp.amax > kPruneMaxStep || (uint64_t)pp.amax * maxL >= (1u << 23)) return pp;
    // No step gains anything (kappa == 0): amax is the one unit of margin.  The builders, which see kappa64 = 1e-30, give
    // every node TWO units (a product above 0 rounds up to 1, plus the margin).  Both stand: the bound is the smaller of
    // two terms, a * r and the column term, each a bound on its own as long as its step is at least the true gain of
    // a match (0 here) plus the unit of margin -- a and the node gains need not be equal (gate_check.cpp asserts this).
    if (pp.kappa64 <= 0.f) pp.kappa64 = 1e-30f;
    // (a launch whose queries fit ONE strip skips nothing -- column 0 keeps every row in play -- so nobody needs the
    // bound: the DAG build leaves its step 9 out, 9 % of its time for V4 amplicons)
    if (single_strip) return pp;
    pp.on = 1;
    return pp;
}

// Whether a launch's waves run the scout pass (mesh_dp.hip, chain_scout_wave) -- apart from the test hook that sets
// every scout value: a chain to scout along (device-built DAGs), the kernel that has the pass (the specialised one, with
// the skip on and two strips or more), and no fixed guess.  T: the geometry's virtual thread count (64 per strip).
inline bool scout_allowed(bool has_chain, bool weighted, bool forbid, bool prune_on, bool rho_fixed, bool below_init, float gp,
                          float gpe, int T, bool scout_knob_off, bool generic_only) {
    return has_chain && !weighted && !forbid && prune_on && !rho_fixed && below_init && gp >= gpe && T > 64 && !scout_knob_off &&
           !generic_only;
}

// ---- geometry and LDS ring of a launch, lanes or waves for its walk
// A geometry is (columns per lane B, strips S): one wave sweeps S strips of 64*B columns; T = 64 * S
// is kept as the geometry's "virtual thread count" (T * B columns).  Fat lanes amortise the per-row
// fixed work of a wave (row record, chain exchange, publish) over more cells, thin lanes need fewer
// registers and allow more waves per SIMD.  Measured on MI355X, 16S queries, DP kernel alone on a
// launch that fills every wave slot (tools/perf_dp_geoms.sh): B = 12 (2 waves/SIMD) 403 Gcell/s,
// B = 8 (3 waves/SIMD) 461, B = 4 (4 waves/SIMD) 226.  The geometry for a launch is the one with
// the smallest padded width / throughput.
constexpr int kLaneCells[] = {4, 8, 12};
constexpr double kLaneRate[] = {226.0, 461.0, 403.0};  // Gcell/s of the B = 4, 8, 12 kernels (above)
constexpr int kMaxStrips = 40;  // 40 x 256 columns (B = 4) cover SINA_HIP_MAX_QUERY_LEN

// The geometry for a batch whose longest query has maxL bases; false: none covers it.  forced_T, forced_B: the
// SINA_HIP_TEST="geom=T,B" hook (0, 0: none) -- taken if it is a geometry the kernels have and covers maxL, else ignored.
inline bool dp_geom_for(uint32_t maxL, int forced_T, int forced_B, DpGeom *g) {
    if (forced_T % 64 == 0 && forced_T >= 64 && forced_T <= 64 * kMaxStrips && (forced_B == 4 || forced_B == 8 || forced_B == 12) &&
        (uint32_t)(forced_T * forced_B) >= maxL) {
        g->T = forced_T;
        g->B = forced_B;
        return true;
    }
    // one strip covers the query: the thinnest lanes that do (a wider lane would only idle -- V4
    // amplicons, 250 bases: B = 4 487 Gcell/s, B = 8 with half the lanes unused 260)
    for (int i = 0; i < 3; i++)
        if (maxL <= 64u * (uint32_t)kLaneCells[i]) {
            g->T = 64;
            g->B = kLaneCells[i];
            return true;
        }
    // several strips: B = 8 or 12 by padded width / throughput
    double best = 0;
    bool found = false;
    for (int i = 1; i < 3; i++) {
        const int b = kLaneCells[i];
        const uint32_t strips = (maxL + 64u * b - 1) / (64u * b);
        if (strips > (uint32_t)kMaxStrips) continue;
        const double cost = (double)(strips * 64u * b) / kLaneRate[i];
        if (!found || cost < best) {
            best = cost;
            g->T = (int)strips * 64;
            g->B = b;
            found = true;
        }
    }
    return found;
}

// one LDS row slot: value | gapm_val of the strip's columns + the value left of the strip
inline size_t dp_slot_bytes(const DpGeom &g) { return (size_t)64 * g.B * 8 + 16; }
constexpr int kDpMaxRing = 8;  // the slot allocators keep 8 slot states; deeper rings gain nothing
// LDS per workgroup (= per wave) that still lets the kernel's register budget decide the occupancy
inline size_t dp_default_lds_budget(const DpGeom &g) { return (size_t)160 * 1024 / (4 * dp_waves_per_simd(g.B)) - 64; }
// The LDS ring of a launch of geometry g: as many row slots as the budget holds (budget_override, bytes per workgroup:
// the context's lds_budget; 0: the default), one at least, no more than a CU's 160 KB and no deeper than kDpMaxRing.
inline void dp_ring_plan(const DpGeom &g, size_t budget_override, DpPlan *pl) {
    const size_t slot = dp_slot_bytes(g);
    size_t budget = budget_override ? budget_override : dp_default_lds_budget(g);
    if (budget < slot) budget = slot;
    if (budget > 160 * 1024) budget = 160 * 1024;
    pl->geom = g;
    pl->W = std::min((int)(budget / slot), kDpMaxRing);
    pl->lds = (size_t)pl->W * slot;
}

// Launches of kBtLanesMin queries and more, none longer than kBtLanesMaxLen, walk one lane per query
// (backtrack_lanes_kernel, traceback.hip).  The lanes' walk takes 1.4 us per step whatever the launch (2.2 ms for 16S; 2 us
// and 3.1 ms before a step fetched its cell, record and predecessors together, round 11), the waves' walk 0.27 us of
// the device's instruction issue per query (2.5 ms at 9216 queries, 1.1 at 3072): at 9216 queries the lanes' are
// latency that the launches queued behind on the other FIFO stream cover where the waves' are instructions taken
// from them.  Re-measured in round 11 with the shorter lane walk (profiles/r11_walk_onetrip_ab.txt), the rule stands:
// the headline with waves forced is below every run with lanes; with half the queries duplicates (4608 per launch)
// lanes and waves are within each other's run-to-run band, where lanes cost 6-8 % before; and a launch of
// 23S-long queries (6000 steps; lanes 12 ms in the pipeline, 16 before) is waited for by a pipeline that holds two
// batches of them -- 95 k sequences/s with lanes against 101 k with waves.  forced: SINA_HIP_TEST=bt_lanes=0/1 forces
// one (-1: none).
constexpr uint32_t kBtLanesMin = 8192, kBtLanesMaxLen = 2048;
inline bool bt_by_lanes(uint32_t nq, uint32_t asm_cap, int forced) {
    if (forced >= 0) return forced != 0;
    return nq >= kBtLanesMin && asm_cap <= kBtLanesMaxLen;
}

// ---- launch ranges
// End of a DP launch range that the trace-back budget cut short (q1 < limit): whole rounds of wave
// slots if it holds at least one.
inline uint32_t dp_round_range(uint32_t q0, uint32_t q1, uint32_t limit, uint32_t slots) {
    const uint32_t n = q1 - q0;
    return (q1 < limit && n > slots) ? q0 + n / slots * slots : q1;
}
// End of the launch range that starts at q0: the largest range below `limit` whose trace-back plane (sum of
// N * Lp cells) fits the budget -- one query at least --, cut to whole rounds.  n_of(q): nodes of query q's DAG.
template <class NodeCount>
inline uint32_t dp_cut_range(NodeCount n_of, uint32_t q0, uint32_t limit, int Lp, uint64_t budget_cells, uint32_t slots) {
    uint32_t q1 = q0;
    uint64_t cells = 0;
    while (q1 < limit) {
        const uint64_t add = (uint64_t)n_of(q1) * (uint64_t)Lp;
        if (q1 > q0 && cells + add > budget_cells) break;
        cells += add;
        q1++;
    }
    return dp_round_range(q0, q1, limit, slots);
}

// ---- what a launch's QDesc array adds up to
struct LaunchSums {
    uint64_t tb_cells = 0, spill_rows = 0, cells = 0;
    // edge records per strip boundary: every query's region starts on a 64-byte line (common.h, EdgeRec)
    uint64_t edge_entries = 0;
    uint32_t max_n = 0, max_l = 0;  // the longest DAG and query
};
inline LaunchSums launch_sums(const QDesc *qd, uint32_t bq, int Lp) {
    LaunchSums s;
    for (uint32_t q = 0; q < bq; q++) {
        assert(qd[q].tb_off == s.tb_cells && qd[q].spill_off == s.spill_rows && qd[q].erec_off == s.edge_entries);
        s.tb_cells += (uint64_t)qd[q].N * (uint64_t)Lp;
        s.spill_rows += qd[q].n_spill;
        s.cells += (uint64_t)qd[q].N * qd[q].L;
        s.edge_entries += dp_edge_entries(qd[q].N);
        s.max_n = std::max(s.max_n, qd[q].N);
        s.max_l = std::max(s.max_l, qd[q].L);
    }
    return s;
}

// ---- families that share a DAG
// What a builder left in the context's rec / node_pos / succ_minpos / pred (/ rgain, prof16) buffers for the n distinct
// families of a chunk: family u's node arrays start at u * ncap, its predecessor entries at pred_off[u].
struct BuiltGraphs {
    uint32_t ncap = 0;
    std::vector<uint64_t> pred_off;  // per family, into c->pred
    std::vector<uint32_t> sizes;     // per family: kBuiltWords words (common.h, kBuiltN ...)
};

// Queries q0 .. q0 + bq - 1 (fam_off is absolute) with the same ORDERED family share one DAG.  dag_of[q]: which of the
// chunk's distinct families query q0 + q has, numbered by first appearance; returns their number.  If that is below bq,
// ufam_ids / ufam_off hold the distinct families, packed in that order (offsets from 0); else they are left alone.
inline uint32_t distinct_families(const uint32_t *fam_ids, const uint64_t *fam_off, uint32_t q0, uint32_t bq,
                                  std::vector<uint32_t> *dag_of, std::vector<uint32_t> *ufam_ids, std::vector<uint64_t> *ufam_off) {
    dag_of->resize(bq);
    for (uint32_t q = 0; q < bq; q++) (*dag_of)[q] = q;
    if (bq < 2) return bq;
    auto len = [&](uint32_t q) { return fam_off[q0 + q + 1] - fam_off[q0 + q]; };
    auto ids = [&](uint32_t q) { return fam_ids + fam_off[q0 + q]; };
    std::unordered_map<std::string_view, uint32_t> seen;  // the id list, as bytes -> its DAG
    seen.reserve(2 * (size_t)bq);
    std::vector<uint32_t> first;  // first[u] = first query (in the chunk) of DAG u
    for (uint32_t q = 0; q < bq; q++) {
        const auto at = seen.try_emplace(std::string_view(reinterpret_cast<const char *>(ids(q)), 4 * len(q)), (uint32_t)first.size());
        if (at.second) first.push_back(q);
        (*dag_of)[q] = at.first->second;
    }
    const uint32_t n_dags = (uint32_t)first.size();
    if (n_dags == bq) return bq;  // (dag_of is the identity: families appear in query order)
    ufam_off->assign((size_t)n_dags + 1, 0);
    for (uint32_t u = 0; u < n_dags; u++) (*ufam_off)[u + 1] = (*ufam_off)[u] + len(first[u]);
    ufam_ids->resize((*ufam_off)[n_dags]);
    for (uint32_t u = 0; u < n_dags; u++) memcpy(ufam_ids->data() + (*ufam_off)[u], ids(first[u]), 4 * len(first[u]));
    return n_dags;
}

// The descriptors of queries q0 + r0 .. q0 + r1 - 1 of a chunk whose DAGs a device builder made (qoff is absolute):
// every query keeps its own trace-back cells, spill rows and edge records, the node arrays are its family's.
inline void family_qdescs(const BuiltGraphs &bg, const uint32_t *dag_of, const uint64_t *qoff, uint32_t q0, uint32_t r0,
                          uint32_t r1, int Lp, std::vector<QDesc> *qd) {
    qd->resize(r1 - r0);
    uint64_t tbc = 0, sprows = 0;
    uint32_t erec_cursor = 0;
    for (uint32_t r = r0; r < r1; r++) {
        const uint32_t u = dag_of[r];  // (this query's DAG among the chunk's distinct ones)
        const uint32_t *sz = bg.sizes.data() + (size_t)kBuiltWords * u;
        QDesc &d = (*qd)[r - r0];
        d.node_off = (uint64_t)u * bg.ncap;
        d.edge_off = bg.pred_off[u];
        d.q_off = qoff[q0 + r] - qoff[q0 + r0];
        d.tb_off = tbc;
        d.spill_off = sprows;
        d.N = sz[kBuiltN];
        d.L = (uint32_t)(qoff[q0 + r + 1] - qoff[q0 + r]);
        d.n_spill = sz[kBuiltSpill];
        d.first_sink = sz[kBuiltFirstSink];
        d.gmin = sz[kBuiltGmin];
        d.erec_off = erec_cursor;
        erec_cursor += dp_edge_entries(d.N);
        tbc += (uint64_t)d.N * (uint64_t)Lp;
        sprows += d.n_spill;
    }
}

// ---- what a launch swept (certified row skip), and what its queries say about the next launch's guess
struct SweepSummary {
    uint64_t rows_nominal = 0, rows_swept = 0, cells_swept = 0, n_pruned = 0, n_second = 0, n_full = 0;
    std::vector<float> ratios;  // optimum / first-cell bound of the queries that have one
};
inline SweepSummary summarise_sweep(const QDesc *qd, const DpResult *res, uint32_t bq, uint32_t kstrip) {
    SweepSummary s;
    for (uint32_t q = 0; q < bq; q++) {
        const uint64_t strips = (qd[q].L - 1) / kstrip + 1;
        s.rows_nominal += strips * qd[q].N;
        const DpResult &r = res[q];
        if (r.attempts == 0) {  // (a kernel that sweeps everything)
            s.rows_swept += strips * qd[q].N;
            s.cells_swept += (uint64_t)qd[q].N * qd[q].L;
            continue;
        }
        s.rows_swept += r.rows_done;
        s.cells_swept += r.cells_done;
        s.n_pruned++;
        s.n_second += r.attempts == 2 ? 1 : 0;
        s.n_full += r.attempts >= 3 ? 1 : 0;
        if (r.status == 0 && r.gain0 > 0.f && r.raw < 0.f) s.ratios.push_back(-r.raw / r.gain0);
    }
    return s;
}
// The launch's smallest optimum / bound, less a margin: a query whose first bound fails pays a second sweep, and
// the launch ends with its slowest wave -- one such query among the last to start costs the whole device a sweep's
// time, so the guess aims at NO failures among queries like the ones seen (a wider band costs a few per cent).
// Two guesses per store.  Alone (a launch without a scout pass: caller-built DAGs) a guess that fails ONE query costs
// the whole launch a sweep's time -- it ends with its slowest wave -- so it aims below the smallest ratio seen
// (round 5; the 2 % point, tried in round 6: 95 second attempts in 184 320 queries, DP launches 30.1 instead of
// 26.4 ms).  As the GUARD of the scout's values it only has to catch a scout that lost its query: the 2 % point,
// six per cent looser still in the kernel -- one poorly aligning query among 9216 does not widen everybody's guard.
// (ratios is reordered.)
inline void update_rho(float *rho, float *rho_guard, std::vector<float> &ratios) {
    if (ratios.empty()) return;
    const float rho_seen = *std::min_element(ratios.begin(), ratios.end()) - 0.015f;
    const size_t at = ratios.size() / 50;
    std::nth_element(ratios.begin(), ratios.begin() + (std::ptrdiff_t)at, ratios.end());
    const float rho_guard_seen = ratios[at] - 0.015f;
    if (!(rho_seen > 0.f)) return;
    // down at once (a second sweep per query is what a bold guess costs), up by halves
    *rho = rho_seen < *rho ? rho_seen : 0.5f * (*rho + rho_seen);
    *rho = std::min(0.99f, std::max(0.05f, *rho));
    *rho_guard = rho_guard_seen < *rho_guard ? rho_guard_seen : 0.5f * (*rho_guard + rho_guard_seen);
    *rho_guard = std::min(0.99f, std::max(0.05f, *rho_guard));
}

// ---- host-built graphs
// Host-side preparation of a range of host-built graphs: descriptors, row records
// (sink flag, spill slot for rows with a successor further than W rows away).
struct HostPrep {
    std::vector<QDesc> qd;
    std::vector<uint4> rec;
    std::vector<uint2> rgain;     // the DP kernel's row-skip bound per node + its last successor (common.h), filled when kappa64 > 0
    bool rgain_ok = true;         // ... and valid: every DAG of the range is laid out by columns
    std::vector<uint32_t> pred;  // id | (LDS slot or spill row) << 16 | spilled << 31 (what mesh_dp_kernel reads)
    std::vector<uint2> pred4;    // per node, beside rec: its first four predecessor ids (common.h, pred4_pack; what the walk reads)
    std::vector<uint32_t> last;  // scratch: last successor per row
};

// spill_q: where a query that needs more than kMaxSpillRows spill rows is reported (sina_hip_align_graphs_any sends
// that query through the wide kernel)
inline int prep_range(const sina_hip_graph_batch *g, const uint64_t *qoff, uint32_t q0, uint32_t q1, int Lp, int W,
                       HostPrep *hp, float kappa64, uint32_t *spill_q) {
    const uint64_t nbase = g->node_off[q0], ebase = g->edge_off[q0];
    const uint64_t nn = g->node_off[q1] - nbase;
    hp->qd.resize(q1 - q0);
    hp->rec.resize(nn);
    hp->pred4.resize(nn);
    hp->rgain.assign(kappa64 > 0.f ? nn : 0, uint2{0u, 0u});
    hp->rgain_ok = true;
    hp->pred.resize(g->edge_off[q1] - ebase + 8);
    uint64_t tb_cells = 0, spill_rows = 0;
    uint32_t erec_cursor = 0;
    for (uint32_t q = q0; q < q1; q++) {
        QDesc &d = hp->qd[q - q0];
        const uint64_t no = g->node_off[q], eo = g->edge_off[q];
        const uint32_t N = (uint32_t)(g->node_off[q + 1] - no);
        d.node_off = no - nbase;
        d.erec_off = erec_cursor;
        erec_cursor += dp_edge_entries(N);
        d.edge_off = eo - ebase;
        d.q_off = qoff[q] - qoff[q0];
        d.tb_off = tb_cells;
        d.spill_off = spill_rows;
        d.N = N;
        d.L = (uint32_t)(qoff[q + 1] - qoff[q]);
        const uint32_t *po = g->pred_off + no + q;  // N+1 entries, relative to eo
        uint4 *rec = hp->rec.data() + d.node_off;
        for (uint32_t m = 0; m < N; m++) {
            // (what the row record and the kernel's topological sweep can represent: fail, do not truncate)
            // (the count is a limit of this path, a descending pred_off is malformed input: same message, different kind)
            if (po[m + 1] < po[m]) SH_FAIL("align_graphs: a node has more than 255 predecessors (or pred_off is not ascending)");
            if (po[m + 1] - po[m] > 255u)
                SH_FAIL_LIMIT("align_graphs: a node has more than 255 predecessors (or pred_off is not ascending)");
            for (uint32_t e = po[m]; e < po[m + 1]; e++)
                if (g->pred[eo + e] >= m) SH_FAIL("align_graphs: predecessor ids must be smaller than the node's id");
            uint32_t wbits;
            memcpy(&wbits, &g->node_weight[no + m], 4);
            rec[m].x = po[m];
            rec[m].y = wbits;
            rec[m].z = ((po[m + 1] - po[m]) & 0xffu) | ((uint32_t)(g->node_mask[no + m] & 0xffu) << 8) | kRecSink;
            rec[m].w = kRowNone;
        }
        // last successor of every row (0 = none), sink and fence flags
        std::vector<uint32_t> &last = hp->last;
        last.assign(N, 0);
        for (uint32_t m = 0; m < N; m++) {
            for (uint32_t e = po[m]; e < po[m + 1]; e++) {
                const uint32_t p = g->pred[eo + e];
                rec[p].z &= ~kRecSink;
                last[p] = m;  // rows ascend
                if (m - p > (uint32_t)kFarLds) rec[p].z |= kRecFence;
            }
        }
        d.first_sink = 0;
        d.gmin = 0;
        for (uint32_t m = 0; m < N; m++)
            if (rec[m].z & kRecSink) {
                d.first_sink = m;
                break;
            }
        // LDS slots by liveness, first free slot wins; a row that finds none is spilled.  Rows are
        // allocated in independent segments (dp_slot_segment, common.h), like the device DAG build does.
        uint32_t nsp = 0;
        uint32_t free_at[64];
        const uint32_t seg_len = dp_slot_segment(N);
        for (uint32_t m = 0; m < N; m++) {
            if (m % seg_len == 0)
                for (int x = 0; x < W; x++) free_at[x] = 0;
            if (rec[m].z & kRecSink) continue;  // w stays kRowNone
            if (last[m] == m + 1) continue;      // only the next row reads it: handed over in registers
            int slot = -1;
            const uint32_t seg_end = std::min<uint32_t>(N, (m / seg_len + 1) * seg_len);
            if (!(rec[m].z & kRecFence) && last[m] < seg_end)  // (else: always a spill row)
                for (int x = 0; x < W; x++)
                    if (free_at[x] <= m) {
                        slot = x;
                        break;
                    }
            if (slot >= 0) {
                free_at[slot] = last[m];
                rec[m].w = (uint32_t)slot;
            } else {
                rec[m].w = kRowSpilled | nsp++;
            }
        }
        for (uint32_t m = 0; m < N; m++) {
            uint32_t first_far = 0;
            uint32_t dist = po[m + 1] > po[m] ? 0u : kRecDistFar;
            uint32_t p4[4] = {0u, 0u, 0u, 0u};
            for (uint32_t e = po[m]; e < po[m + 1]; e++) {
                const uint32_t p = g->pred[eo + e];
                if (e - po[m] < 4u) p4[e - po[m]] = p;
                const uint32_t pw = rec[p].w == kRowNone ? 0u : rec[p].w;  // (kRowNone: in registers for this row)
                const bool sp = (pw & kRowSpilled) != 0;
                if (sp && first_far == 0) first_far = e - po[m] + 1;
                dist = std::max(dist, m - p);
                hp->pred[d.edge_off + e] = p | ((pw & 0x7FFFu) << 16) | (sp ? kPredSpilled : 0u);
            }
            rec[m].z |= (first_far << 24) | (std::min(dist, kRecDistFar) << kRecDistShift);
            hp->pred4[d.node_off + m] = pred4_pack(p4[0], p4[1], p4[2], p4[3]);
        }
        if (nsp > kMaxSpillRows) {
            if (spill_q) *spill_q = q;
            SH_FAIL_LIMIT("align_graphs: too many spill rows for one query");
        }
        // The row-skip bound, as the device DAG build computes it (graph_build.hip step 9): R(m) = the sum, over the
        // columns right of node m's, of the column's best node's gain.  It is a bound only for a DAG laid out like
        // mseq's -- columns ascend with the node ids, every edge leads to a column further right --, which a caller's
        // arrays need not be: checked here, and a launch holding a DAG that is not runs without the skip.
        if (kappa64 > 0.f) {
            uint2 *rg = hp->rgain.data() + d.node_off;
            const uint32_t *pos = g->node_pos + no;
            bool ok = true;
            for (uint32_t m = 0; m < N && ok; m++) {
                if (m > 0 && pos[m] < pos[m - 1]) ok = false;
                for (uint32_t e = po[m]; e < po[m + 1] && ok; e++)
                    if (pos[g->pred[eo + e]] >= pos[m]) ok = false;
            }
            if (!ok) hp->rgain_ok = false;
            uint32_t right = 0, cols_right = 0, gmin = 0xFFFFFFFFu;  // columns right of the one being finished
            for (uint32_t m = N; ok && m > 0;) {
                uint32_t first = m - 1, mx = 0;
                while (first > 0 && pos[first - 1] == pos[m - 1]) first--;
                for (uint32_t j = first; j < m; j++) {
                    mx = std::max(mx, prune_gain_units(g->node_weight[no + j], kappa64));
                    rg[j] = uint2{right, last[j] | (cols_right << 16)};
                }
                right += mx;
                cols_right++;
                gmin = std::min(gmin, mx);
                m = first;
            }
            d.gmin = ok ? gmin : 0u;
        }
        d.n_spill = nsp;
        spill_rows += nsp;
        tb_cells += (uint64_t)N * Lp;
    }
    return 0;
}

// sina_hip_align_graphs_any: what is malformed in any path, and which queries only the wide kernel takes by the cheap
// limits (nodes, bases, predecessors per node; the spill-row limit shows when a fast range is prepared).  Every edge of
// every query is looked at here, and prep_range looks at a fitting query's edges again: one more pass over the CSR per
// batch, the price of routing before anything runs on this opt-in path.
inline int classify_any(const sina_hip_graph_batch *g, const uint64_t *qoff, bool all_wide, std::vector<uint8_t> *wide) {
    wide->assign(g->nq, all_wide ? 1 : 0);
    for (uint32_t q = 0; q < g->nq; q++) {
        const uint64_t L = qoff[q + 1] - qoff[q];
        const uint64_t N = g->node_off[q + 1] - g->node_off[q];
        if (L == 0 || N == 0) SH_FAIL("align_graphs_any: empty query or graph");
        if (L > 0xFFFFFFFFull || N > 0xFFFFFFFFull) SH_FAIL("align_graphs_any: more than 2^32 - 1 nodes or bases");
        // (the wide mesh has (N + L - 1) * min(N, L) cells: kept below 2^63, so that the budget sees the real number)
        if (N + L - 1 > (1ull << 63) / std::min(N, L)) SH_FAIL("align_graphs_any: a mesh of more than 2^63 cells");
        if (L > SINA_HIP_MAX_QUERY_LEN || N > 65535) (*wide)[q] = 1;
        const uint64_t no = g->node_off[q], eo = g->edge_off[q], ne = g->edge_off[q + 1] - eo;
        const uint32_t *po = g->pred_off + no + q;
        for (uint64_t m = 0; m < N; m++) {
            if (po[m + 1] < po[m] || po[m + 1] > ne) SH_FAIL("align_graphs_any: pred_off is not ascending (or leaves the query's edges)");
            if (po[m + 1] - po[m] > 255u) (*wide)[q] = 1;
            for (uint32_t e = po[m]; e < po[m + 1]; e++)
                if (g->pred[eo + e] >= m) SH_FAIL("align_graphs_any: predecessor ids must be smaller than the node's id");
        }
    }
    return 0;
}
}  // namespace sina_hip
