// Checks the planning code of the DP driver (sina_amd/csrc/dp_plan.h) against plain models, without a device.
// Built and run by tests/test_dp_plan_cpu.py (address + undefined-behaviour sanitizers); exits non-zero with a
// message on the first difference.  All inputs are seeded.
#include <cstdarg>
#include <map>
#include <random>
#include <set>

#include "dp_plan.h"

namespace sina_hip {
static std::string g_err;
static int g_err_limit = -1;  // -1 none, 0 plain, 1 limit
void set_error(const std::string &m) { g_err = m, g_err_limit = 0; }
void set_limit_error(const std::string &m) { g_err = m, g_err_limit = 1; }
}  // namespace sina_hip
using namespace sina_hip;

#define NOINLINE __attribute__((noinline))
static const char *g_case = "";
[[noreturn]] static void fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "dp_plan_check: %s: ", g_case);
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(1);
}
#define CHECK(cond, ...) \
    do {                 \
        if (!(cond)) fail(__VA_ARGS__); \
    } while (0)

using Rng = std::mt19937_64;
static uint32_t below(Rng &r, uint32_t n) { return (uint32_t)(r() % n); }  // 0 .. n-1
static uint32_t between(Rng &r, uint32_t lo, uint32_t hi) { return lo + below(r, hi - lo + 1); }

// ------------------------------------------------------------------------------------------------ prep_range
struct Dag {
    std::vector<uint32_t> pos, pred_off{0}, pred;  // pred_off: N + 1 entries
    std::vector<uint8_t> mask;
    std::vector<float> weight;
    uint32_t n() const { return (uint32_t)pos.size(); }
    NOINLINE void node(uint32_t column, std::vector<uint32_t> preds, float w = 1.f, uint8_t m = 1) {
        std::sort(preds.begin(), preds.end());
        pos.push_back(column), mask.push_back(m), weight.push_back(w);
        pred.insert(pred.end(), preds.begin(), preds.end());
        pred_off.push_back((uint32_t)pred.size());
    }
};
struct Batch {
    std::vector<Dag> dags;
    std::vector<uint64_t> node_off{0}, edge_off{0}, qoff{0};
    std::vector<uint32_t> pos, pred_off, pred;
    std::vector<uint8_t> mask;
    std::vector<float> weight;
    sina_hip_graph_batch g{};
    NOINLINE void add(const Dag &d, uint32_t qlen) {
        dags.push_back(d);
        node_off.push_back(node_off.back() + d.n());
        edge_off.push_back(edge_off.back() + d.pred.size());
        qoff.push_back(qoff.back() + qlen);
        pos.insert(pos.end(), d.pos.begin(), d.pos.end());
        mask.insert(mask.end(), d.mask.begin(), d.mask.end());
        weight.insert(weight.end(), d.weight.begin(), d.weight.end());
        pred_off.insert(pred_off.end(), d.pred_off.begin(), d.pred_off.end());
        pred.insert(pred.end(), d.pred.begin(), d.pred.end());
    }
    const sina_hip_graph_batch *batch() {
        g.nq = (uint32_t)dags.size();
        g.node_off = node_off.data(), g.edge_off = edge_off.data();
        g.node_pos = pos.data(), g.node_mask = mask.data(), g.node_weight = weight.data();
        g.pred_off = pred_off.data(), g.pred = pred.data();
        g.width = 100000;
        return &g;
    }
};

// a random layered DAG: columns ascend with the node ids, every edge leads to a column further right; mostly a chain,
// with edges that skip a few rows, some that skip many (spill rows, fences) and columns of several nodes
NOINLINE static Dag random_dag(Rng &r, uint32_t n) {
    Dag d;
    const uint32_t far_every = between(r, 5, 60), same_col = below(r, 4);
    uint32_t col = below(r, 5);
    std::vector<uint32_t> col_first;  // first node of every node's column
    for (uint32_t m = 0; m < n; m++) {
        const bool same = m > 0 && below(r, 10) < same_col;
        if (m > 0 && !same) col += between(r, 1, 3);
        const uint32_t first = same ? col_first[m - 1] : m;  // predecessors lie before the column's first node
        col_first.push_back(first);
        std::set<uint32_t> ps;
        if (first > 0) {
            if (below(r, 10) < 8) ps.insert(first - 1);
            for (uint32_t k = below(r, 3); k > 0; k--) ps.insert(first - 1 - below(r, std::min(first, 6u)));
            if (below(r, far_every) == 0) ps.insert(below(r, first));
        }
        d.node(col, std::vector<uint32_t>(ps.begin(), ps.end()), 0.25f * (float)between(r, 0, 8), (uint8_t)between(r, 1, 15));
    }
    return d;
}

static uint32_t node_with_pred(const Dag &d, uint32_t from) {
    while (d.pred_off[from + 1] == d.pred_off[from]) from++;
    return from;
}

// what a DAG's edges say about its rows, computed directly
struct RowModel {
    std::vector<uint32_t> last;  // last successor (0: none)
    std::vector<bool> has_succ, fence;
    bool by_columns = true;  // columns ascend with the ids, every edge leads further right
    explicit RowModel(const Dag &d) : last(d.n(), 0), has_succ(d.n(), false), fence(d.n(), false) {
        for (uint32_t m = 0; m < d.n(); m++) {
            if (m > 0 && d.pos[m] < d.pos[m - 1]) by_columns = false;
            for (uint32_t e = d.pred_off[m]; e < d.pred_off[m + 1]; e++) {
                const uint32_t p = d.pred[e];
                has_succ[p] = true;
                last[p] = std::max(last[p], m);
                if (m - p > (uint32_t)kFarLds) fence[p] = true;
                if (d.pos[p] >= d.pos[m]) by_columns = false;
            }
        }
    }
};

// row records: flags, and where every row is kept (LDS slot by liveness, spill row, or nowhere); returns the spill rows
NOINLINE static uint32_t check_rows(uint32_t q, const Dag &d, const RowModel &mo, const uint4 *rec, int W) {
    const uint32_t N = d.n(), seg = dp_slot_segment(N);
    uint32_t nsp = 0;
    for (uint32_t m = 0; m < N; m++) {
        const uint32_t np = d.pred_off[m + 1] - d.pred_off[m];
        uint32_t wbits;
        memcpy(&wbits, &d.weight[m], 4);
        CHECK(rec[m].x == d.pred_off[m] && rec[m].y == wbits, "q %u row %u: rec.x / rec.y", q, m);
        CHECK((rec[m].z & 0xffu) == np && ((rec[m].z >> 8) & 0xffu) == d.mask[m], "q %u row %u: predecessor count / mask", q, m);
        CHECK(((rec[m].z & kRecSink) != 0) == !mo.has_succ[m], "q %u row %u: sink flag", q, m);
        CHECK(((rec[m].z & kRecFence) != 0) == mo.fence[m], "q %u row %u: fence flag", q, m);
        const uint32_t w = rec[m].w;
        if (!mo.has_succ[m] || mo.last[m] == m + 1) {
            CHECK(w == kRowNone, "q %u row %u: a sink / a row read only by the next row is kept (%08x)", q, m, w);
            continue;
        }
        CHECK(w != kRowNone, "q %u row %u: a row with a later successor is not kept", q, m);
        const uint32_t seg0 = m / seg * seg, seg_end = std::min(N, seg0 + seg);
        uint32_t live = 0, n_live = 0;  // slots (a bit each) of the segment's earlier rows that still have a successor to come
        for (uint32_t r = seg0; r < m; r++)
            if (rec[r].w < 32u && mo.last[r] > m) {
                CHECK(!(live >> rec[r].w & 1u), "q %u: rows %u and another share slot %u while both are live at row %u", q, r, rec[r].w, m);
                live |= 1u << rec[r].w, n_live++;
            }
        const bool must_spill = mo.fence[m] || mo.last[m] >= seg_end || (int)n_live == W;
        CHECK(((w & kRowSpilled) != 0) == must_spill, "q %u row %u: spilled %d, expected %d (fence %d, last %u, segment end %u, %u of %d slots live)",
              q, m, (w & kRowSpilled) != 0, must_spill, (int)mo.fence[m], mo.last[m], seg_end, n_live, W);
        if (w & kRowSpilled) {
            CHECK((w & ~kRowSpilled) == nsp, "q %u row %u: spill index %u, expected %u", q, m, w & ~kRowSpilled, nsp);
            nsp++;
        } else {
            CHECK(w < (uint32_t)W && !(live >> w & 1u), "q %u row %u: slot %u is out of range or live", q, m, w);
            CHECK((live & ((1u << w) - 1u)) == (1u << w) - 1u, "q %u row %u: slot %u taken though a lower one is free", q, m, w);
        }
    }
    return nsp;
}

// predecessor entries, first_far, distance
NOINLINE static void check_pred_entries(uint32_t q, const Dag &d, const uint4 *rec, const uint32_t *pe) {
    for (uint32_t m = 0; m < d.n(); m++) {
        uint32_t first_far = 0, dist = d.pred_off[m + 1] > d.pred_off[m] ? 0u : kRecDistFar;
        for (uint32_t e = d.pred_off[m]; e < d.pred_off[m + 1]; e++) {
            const uint32_t p = d.pred[e], pw = rec[p].w;
            const bool sp = pw != kRowNone && (pw & kRowSpilled);
            const uint32_t where = pw == kRowNone ? 0u : (pw & 0x7FFFu);
            CHECK(pe[e] == (p | (where << 16) | (sp ? kPredSpilled : 0u)), "q %u row %u: predecessor entry %u is %08x", q, m, e - d.pred_off[m], pe[e]);
            if (sp && !first_far) first_far = e - d.pred_off[m] + 1;
            dist = std::max(dist, m - p);
        }
        CHECK((rec[m].z >> 24) == first_far, "q %u row %u: first_far %u, expected %u", q, m, rec[m].z >> 24, first_far);
        CHECK(((rec[m].z >> kRecDistShift) & 63u) == std::min(dist, kRecDistFar), "q %u row %u: distance field", q, m);
    }
}

// the row-skip bound, by brute force over the columns
NOINLINE static void check_bound(uint32_t q, const Dag &d, const RowModel &mo, const QDesc &qd, const uint2 *rg, float kappa64) {
    std::map<uint32_t, uint32_t> best;  // column -> its best node's gain
    for (uint32_t m = 0; m < d.n(); m++) best[d.pos[m]] = std::max(best[d.pos[m]], prune_gain_units(d.weight[m], kappa64));
    uint32_t gmin = 0xFFFFFFFFu;
    for (const auto &c : best) gmin = std::min(gmin, c.second);
    CHECK(qd.gmin == gmin, "q %u: gmin %u, expected %u", q, qd.gmin, gmin);
    for (uint32_t m = 0; m < d.n(); m++) {
        uint32_t right = 0, cols = 0;
        for (auto c = best.upper_bound(d.pos[m]); c != best.end(); ++c) right += c->second, cols++;
        CHECK(rg[m].x == right && rg[m].y == (mo.last[m] | (cols << 16)), "q %u row %u: rgain {%u, %08x}, expected {%u, %08x}", q, m, rg[m].x, rg[m].y,
              right, mo.last[m] | (cols << 16));
    }
}

// returns HostPrep::rgain_ok
NOINLINE static bool check_prep(Batch &b, uint32_t q0, uint32_t q1, int Lp, int W, float kappa64) {
    HostPrep hp;
    const sina_hip_graph_batch *g = b.batch();
    CHECK(prep_range(g, b.qoff.data(), q0, q1, Lp, W, &hp, kappa64, nullptr) == 0, "prep_range failed: %s", g_err.c_str());
    CHECK(hp.qd.size() == q1 - q0, "qd size");
    uint64_t tb = 0, spill = 0, erec = 0;
    bool all_ok = true;
    for (uint32_t q = q0; q < q1; q++) {
        const Dag &d = b.dags[q];
        const QDesc &qd = hp.qd[q - q0];
        // descriptors: relative offsets and prefix sums
        CHECK(qd.N == d.n() && qd.L == b.qoff[q + 1] - b.qoff[q], "q %u: N / L", q);
        CHECK(qd.node_off == b.node_off[q] - b.node_off[q0] && qd.edge_off == b.edge_off[q] - b.edge_off[q0] &&
                  qd.q_off == b.qoff[q] - b.qoff[q0], "q %u: node / edge / query offset", q);
        CHECK(qd.tb_off == tb && qd.spill_off == spill && qd.erec_off == erec, "q %u: tb_off / spill_off / erec_off are not prefix sums", q);
        const RowModel mo(d);
        const uint32_t nsp = check_rows(q, d, mo, hp.rec.data() + qd.node_off, W);
        check_pred_entries(q, d, hp.rec.data() + qd.node_off, hp.pred.data() + qd.edge_off);
        CHECK(qd.n_spill == nsp, "q %u: n_spill %u, expected %u", q, qd.n_spill, nsp);
        const uint32_t first_sink = (uint32_t)(std::find(mo.has_succ.begin(), mo.has_succ.end(), false) - mo.has_succ.begin());
        CHECK(qd.first_sink == first_sink, "q %u: first_sink %u, expected %u", q, qd.first_sink, first_sink);
        all_ok = all_ok && mo.by_columns;
        if (kappa64 > 0.f && mo.by_columns) check_bound(q, d, mo, qd, hp.rgain.data() + qd.node_off, kappa64);
        else CHECK(qd.gmin == 0, "q %u: gmin %u without a valid bound", q, qd.gmin);
        tb += (uint64_t)d.n() * (uint64_t)Lp, spill += nsp, erec += dp_edge_entries(d.n());
    }
    CHECK(hp.rgain_ok == (kappa64 > 0.f ? all_ok : true), "rgain_ok %d", (int)hp.rgain_ok);
    CHECK(hp.rgain.size() == (kappa64 > 0.f ? b.node_off[q1] - b.node_off[q0] : 0), "rgain size");
    const LaunchSums s = launch_sums(hp.qd.data(), q1 - q0, Lp);  // (asserts the prefix sums once more)
    CHECK(s.tb_cells == tb && s.spill_rows == spill && s.edge_entries == erec, "launch_sums of a prepared range");
    return hp.rgain_ok;
}

NOINLINE static bool check_one(const Dag &d, uint32_t qlen, int W, float kappa64 = 128.f) {
    Batch b;
    b.add(d, qlen);
    return check_prep(b, 0, 1, 512, W, kappa64);
}
NOINLINE static int prep_fails(const Dag &d, std::string *msg) {  // 0 accepted, else 1 + "is a limit"
    Batch b;
    b.add(d, 10);
    HostPrep hp;
    g_err_limit = -1;
    if (prep_range(b.batch(), b.qoff.data(), 0, 1, 512, 4, &hp, 128.f, nullptr) == 0) return 0;
    *msg = g_err;
    return 1 + g_err_limit;
}

NOINLINE static void test_prep_range() {
    Rng r(20250);
    g_case = "prep_range, random";
    for (int it = 0; it < 300; it++) {
        Batch b;
        const uint32_t nq = between(r, 1, 4);
        for (uint32_t q = 0; q < nq; q++) {
            const uint32_t n = below(r, 4) ? between(r, 1, 120) : between(r, 1, 600);
            b.add(random_dag(r, n), between(r, 1, 400));
        }
        const uint32_t q0 = below(r, nq), q1 = between(r, q0 + 1, nq);
        check_prep(b, q0, q1, (int)(256 * between(r, 1, 4)), (int)between(r, 1, kDpMaxRing), below(r, 4) ? 128.f * 1.0001f : 0.f);
    }
}

NOINLINE static void test_prep_directed() {
    Rng r(20255);
    g_case = "prep_range, directed";
    std::string msg;
    for (int W : {1, 4, kDpMaxRing}) {
        Dag one;
        one.node(7, {});
        check_one(one, 1, W);
        Dag chain;
        for (uint32_t m = 0; m < 50; m++) chain.node(2 * m, m ? std::vector<uint32_t>{m - 1} : std::vector<uint32_t>{});
        check_one(chain, 30, W);
        for (uint32_t np : {255u, 256u}) {  // one node with np predecessors
            Dag fan;
            std::vector<uint32_t> all;
            for (uint32_t m = 0; m < np; m++) fan.node(m, {}), all.push_back(m);
            fan.node(np, all);
            if (np == 255) check_one(fan, 40, W);
            else CHECK(prep_fails(fan, &msg) == 2 && msg == "align_graphs: a node has more than 255 predecessors (or pred_off is not ascending)", "256 predecessors: %s", msg.c_str());
        }
        for (uint32_t far : {(uint32_t)kFarLds, (uint32_t)kFarLds + 1}) {  // node 3's last successor is `far` rows on
            Dag d;
            for (uint32_t m = 0; m < 260; m++) {
                std::vector<uint32_t> ps;
                if (m) ps.push_back(m - 1);
                if (m == 3 + far) ps.push_back(3);
                d.node(m, ps);
            }
            check_one(d, 100, W);
        }
        for (uint32_t n : {257u, 16u * 256u + 1u}) {  // one row past a slot-segment boundary, edges across every boundary
            Dag d;
            const uint32_t seg = dp_slot_segment(n);
            for (uint32_t m = 0; m < n; m++) {
                std::vector<uint32_t> ps;
                if (m) ps.push_back(m - 1);
                if (m >= 3 && (m % seg < 2 || m % 7 == 0)) ps.push_back(m - 3);
                d.node(m, ps);
            }
            check_one(d, 64, W);
        }
        Dag unsorted = random_dag(r, 80);  // columns that do not ascend: no bound
        std::swap(unsorted.pos[40], unsorted.pos[10]);
        CHECK(!check_one(unsorted, 64, W), "columns that do not ascend were taken for a valid layout");
        Dag same_col = random_dag(r, 60);  // an edge inside a column: no bound either
        const uint32_t sc = node_with_pred(same_col, 30);
        same_col.pos[same_col.pred[same_col.pred_off[sc]]] = same_col.pos[sc];
        CHECK(!check_one(same_col, 64, W, 64.f), "an edge inside a column was taken for a valid layout");
    }
    Dag self;
    self.node(0, {}), self.node(1, {0});
    self.pred[0] = 1;  // a node as its own predecessor
    CHECK(prep_fails(self, &msg) == 1 && msg == "align_graphs: predecessor ids must be smaller than the node's id", "self edge: %s", msg.c_str());
    Dag desc;
    desc.node(0, {}), desc.node(1, {0}), desc.node(2, {});
    desc.pred_off = {0, 0, 1, 0};
    CHECK(prep_fails(desc, &msg) == 1 && msg == "align_graphs: a node has more than 255 predecessors (or pred_off is not ascending)", "descending pred_off: %s", msg.c_str());
}

// ------------------------------------------------------------------------------------------------ dp_cut_range
NOINLINE static void test_cut_range() {
    g_case = "dp_cut_range";
    Rng r(20251);
    for (int it = 0; it < 2000; it++) {
        const uint32_t nq = between(r, 1, 40), q_first = below(r, 3), slots = between(r, 1, 10);
        const int Lp = (int)(256 * between(r, 1, 4));
        std::vector<uint32_t> n(q_first + nq);
        uint64_t total = 0;
        for (auto &x : n) x = between(r, 1, 600), total += (uint64_t)x * Lp;
        const uint64_t budget = below(r, 8) == 0 ? r() % 1000 : r() % (total + total / 4 + 1);
        const uint32_t limit = q_first + nq;
        uint32_t q0 = q_first;
        while (q0 < limit) {
            const uint32_t q1 = dp_cut_range([&](uint32_t q) { return n[q]; }, q0, limit, Lp, budget, slots);
            const uint32_t q1_array = dp_cut_range([p = n.data()](uint32_t q) { return p[q]; }, q0, limit, Lp, budget, slots);
            CHECK(q1 == q1_array, "callable and array disagree");
            CHECK(q1 > q0 && q1 <= limit, "range [%u, %u) of [%u, %u) is empty or too long", q0, q1, q_first, limit);
            uint32_t u = q0 + 1;  // the largest range that fits, one query at least
            uint64_t cells = (uint64_t)n[q0] * Lp;
            while (u < limit && cells + (uint64_t)n[u] * Lp <= budget) cells += (uint64_t)n[u++] * Lp;
            CHECK(u == q0 + 1 || cells <= budget, "model");
            CHECK(q1 == dp_round_range(q0, u, limit, slots), "range [%u, %u): unrounded end %u, %u slots", q0, q1, u, slots);
            uint64_t got = 0;
            for (uint32_t q = q0; q < q1; q++) got += (uint64_t)n[q] * Lp;
            CHECK(q1 == q0 + 1 || got <= budget, "range [%u, %u) holds %llu cells, budget %llu", q0, q1, (unsigned long long)got, (unsigned long long)budget);
            q0 = q1;  // (successive ranges: no overlap, no hole)
        }
        CHECK(q0 == limit, "ranges end at %u, not %u", q0, limit);
    }
    // whole rounds only where the budget cut the range short, and only if it holds more than one
    CHECK(dp_round_range(0, 25, 30, 10) == 20 && dp_round_range(0, 25, 25, 10) == 25 && dp_round_range(5, 12, 30, 10) == 12 &&
              dp_round_range(5, 15, 30, 10) == 15 && dp_round_range(5, 16, 30, 10) == 15, "dp_round_range");
}

// ------------------------------------------------------------------------------------------------ distinct_families
NOINLINE static void check_families(const std::vector<std::vector<uint32_t>> &fams, uint32_t q0) {
    std::vector<uint32_t> ids;
    std::vector<uint64_t> off{0};
    for (const auto &f : fams) ids.insert(ids.end(), f.begin(), f.end()), off.push_back(ids.size());
    const uint32_t bq = (uint32_t)fams.size() - q0;
    std::map<std::vector<uint32_t>, uint32_t> first_of;  // ordered id list -> number of its DAG
    std::vector<uint32_t> want_dag(bq), firsts;
    for (uint32_t q = 0; q < bq; q++) {
        auto at = first_of.emplace(fams[q0 + q], (uint32_t)firsts.size());
        if (at.second) firsts.push_back(q);
        want_dag[q] = at.first->second;
    }
    const std::vector<uint32_t> sentinel_ids{0xdeadbeefu};
    const std::vector<uint64_t> sentinel_off{77};
    std::vector<uint32_t> dag_of{9, 9, 9}, uids = sentinel_ids;
    std::vector<uint64_t> uoff = sentinel_off;
    const uint32_t n = distinct_families(ids.data(), off.data(), q0, bq, &dag_of, &uids, &uoff);
    CHECK(n == firsts.size(), "%u distinct families, expected %zu", n, firsts.size());
    CHECK(dag_of.size() == bq, "dag_of size");
    if (n == bq) {
        for (uint32_t q = 0; q < bq; q++) CHECK(dag_of[q] == q, "all distinct: dag_of is not the identity");
        CHECK(uids == sentinel_ids && uoff == sentinel_off, "all distinct: the packed arrays were touched");
        return;
    }
    CHECK(dag_of == want_dag, "dag_of differs from the map's numbering by first appearance");
    CHECK(uoff.size() == n + 1 && uoff[0] == 0 && uids.size() == uoff[n], "packed offsets");
    for (uint32_t u = 0; u < n; u++) {
        const auto &f = fams[q0 + firsts[u]];
        CHECK(uoff[u + 1] - uoff[u] == f.size() && std::equal(f.begin(), f.end(), uids.begin() + (std::ptrdiff_t)uoff[u]), "packed family %u", u);
    }
}
NOINLINE static void test_families() {
    g_case = "distinct_families";
    check_families({{1, 2, 3}, {4}, {3, 2, 1}, {1, 2}}, 0);                          // all distinct; a permutation; a prefix
    check_families({{5, 6}, {5, 6}, {5, 6}, {5, 6}}, 0);                              // all equal
    check_families({{5, 6}, {5, 6}, {5, 6}, {5, 6}}, 3);                              // bq = 1
    check_families({{9}}, 0);
    check_families({{1, 2, 3}, {3, 2, 1}, {2, 1, 3}, {1, 2, 3}, {3, 2, 1}}, 0);       // permutations are distinct
    check_families({{7, 7}, {7}, {7, 7, 7}, {7, 7}, {7}}, 0);                         // differ only in length
    check_families({{0, 0}, {0}, {0}, {0, 0}, {0, 0, 0}}, 1);
    Rng r(20252);
    for (int it = 0; it < 600; it++) {
        std::vector<std::vector<uint32_t>> fams(between(r, 1, 60));
        const uint32_t alphabet = between(r, 1, 4), max_len = between(r, 1, 5);
        for (auto &f : fams) {
            f.resize(between(r, 1, max_len));
            for (auto &x : f) x = below(r, alphabet) * 1000003u;
        }
        check_families(fams, below(r, (uint32_t)fams.size()));
    }
}

// ------------------------------------------------------------------------------------------------ family_qdescs, launch_sums
NOINLINE static void test_family_qdescs() {
    g_case = "family_qdescs / launch_sums";
    Rng r(20253);
    for (int it = 0; it < 500; it++) {
        const uint32_t n_dags = between(r, 1, 12), bq = between(r, 1, 30), q0 = below(r, 5);
        const int Lp = (int)(256 * between(r, 1, 4));
        BuiltGraphs bg;
        bg.ncap = between(r, 600, 700);
        bg.sizes.resize((size_t)kBuiltWords * n_dags);
        for (auto &x : bg.sizes) x = between(r, 1, 600);
        for (uint32_t u = 0; u < n_dags; u++) bg.pred_off.push_back(1000ull * u + below(r, 9));
        std::vector<uint32_t> dag_of(bq);
        for (auto &u : dag_of) u = below(r, n_dags);
        std::vector<uint64_t> qoff(q0 + bq + 1, 5);
        for (size_t q = 1; q < qoff.size(); q++) qoff[q] = qoff[q - 1] + between(r, 1, 400);
        const uint32_t r0 = below(r, bq), r1 = between(r, r0 + 1, bq);
        std::vector<QDesc> qd(3);
        family_qdescs(bg, dag_of.data(), qoff.data(), q0, r0, r1, Lp, &qd);
        CHECK(qd.size() == r1 - r0, "size");
        uint64_t tb = 0, spill = 0, cells = 0, erec = 0;
        uint32_t max_n = 0, max_l = 0;
        for (uint32_t q = r0; q < r1; q++) {
            const QDesc &d = qd[q - r0];
            const uint32_t *sz = &bg.sizes[(size_t)kBuiltWords * dag_of[q]];
            CHECK(d.N == sz[0] && d.n_spill == sz[2] && d.first_sink == sz[4] && d.gmin == sz[5], "query %u: size words", q);
            CHECK(d.node_off == (uint64_t)dag_of[q] * bg.ncap && d.edge_off == bg.pred_off[dag_of[q]], "query %u: its DAG's arrays", q);
            CHECK(d.L == qoff[q0 + q + 1] - qoff[q0 + q] && d.q_off == qoff[q0 + q] - qoff[q0 + r0], "query %u: L / q_off", q);
            CHECK(d.tb_off == tb && d.spill_off == spill && d.erec_off == erec, "query %u: offsets are not prefix sums", q);
            tb += (uint64_t)d.N * Lp, spill += d.n_spill, cells += (uint64_t)d.N * d.L, erec += (d.N + 3) / 4 * 4;
            max_n = std::max(max_n, d.N), max_l = std::max(max_l, d.L);
        }
        const LaunchSums s = launch_sums(qd.data(), r1 - r0, Lp);
        CHECK(s.tb_cells == tb && s.spill_rows == spill && s.cells == cells && s.edge_entries == erec && s.max_n == max_n && s.max_l == max_l,
              "launch_sums differs from a direct sum");
    }
    CHECK(kBuiltN == 0 && kBuiltEdges == 1 && kBuiltSpill == 2 && kBuiltStatus == 3 && kBuiltFirstSink == 4 && kBuiltGmin == 5 &&
              kBuiltChainLen == 6 && kBuiltWords == 8 && kBuiltNodeCap == 2 && kBuiltSpillCap == 4, "the builders' size words moved");
}

// ------------------------------------------------------------------------------------------------ summarise_sweep, update_rho
static QDesc qdesc(uint32_t n, uint32_t l) {
    QDesc d{};
    d.N = n, d.L = l;
    return d;
}
static DpResult result(uint32_t attempts, uint32_t rows, uint32_t cells, int32_t status, float raw, float gain0) {
    DpResult r{};
    r.attempts = attempts, r.rows_done = rows, r.cells_done = cells, r.status = status, r.raw = raw, r.gain0 = gain0;
    return r;
}
NOINLINE static void test_sweep_and_rho() {
    g_case = "summarise_sweep";
    // strips of 256 columns: 2, 1, 2, 1, 1, 1 strips -> 20 + 20 + 10 + 7 + 3 + 4 nominal rows
    const QDesc qd[6] = {qdesc(10, 300), qdesc(20, 100), qdesc(5, 257), qdesc(7, 256), qdesc(3, 1), qdesc(4, 9)};
    const DpResult res[6] = {
        result(0, 999, 999, 0, -1.f, 1.f),      // swept in full by a kernel that does not skip: 20 rows, 3000 cells, no ratio
        result(1, 15, 1200, 0, -150.f, 200.f),  // ratio 0.75
        result(2, 9, 1000, 0, -50.f, 100.f),    // second attempt, ratio 0.5
        result(3, 14, 1792, 0, -50.f, 0.f),     // full sweep; no first-cell bound: no ratio
        result(1, 2, 3, 1, -50.f, 100.f),       // failed: no ratio
        result(1, 4, 30, 0, 0.f, 100.f),        // optimum not below 0: no ratio
    };
    SweepSummary s = summarise_sweep(qd, res, 6, 256);
    CHECK(s.rows_nominal == 64 && s.rows_swept == 20 + 15 + 9 + 14 + 2 + 4 && s.cells_swept == 3000 + 1200 + 1000 + 1792 + 3 + 30, "rows / cells");
    CHECK(s.n_pruned == 5 && s.n_second == 1 && s.n_full == 1, "attempt counts");
    CHECK(s.ratios == (std::vector<float>{0.75f, 0.5f}), "ratios");

    g_case = "update_rho";
    float rho = 0.8f, guard = 0.7f;
    std::vector<float> none;
    update_rho(&rho, &guard, none);
    CHECK(rho == 0.8f && guard == 0.7f, "no usable ratio moved the guesses");
    std::vector<float> tiny{0.01f};  // smallest ratio less the margin is not above 0: nothing to learn
    update_rho(&rho, &guard, tiny);
    CHECK(rho == 0.8f && guard == 0.7f, "a ratio below the margin moved the guesses");
    update_rho(&rho, &guard, s.ratios);  // below both guesses: down at once
    CHECK(rho == 0.5f - 0.015f && guard == 0.5f - 0.015f, "down at once: %g %g", rho, guard);
    rho = 0.4f, guard = 0.3f;
    std::vector<float> above{0.9f};  // above both: up by halves
    update_rho(&rho, &guard, above);
    CHECK(rho == 0.5f * (0.4f + (0.9f - 0.015f)) && guard == 0.5f * (0.3f + (0.9f - 0.015f)), "up by halves: %g %g", rho, guard);
    std::vector<float> hundred;  // the guard follows the size / 50 point: the third smallest of a hundred
    for (int i = 0; i < 100; i++) hundred.push_back(0.5f + 0.004f * (float)((i * 37) % 100));
    const float smallest = 0.5f, third = 0.5f + 0.004f * 2.f;
    rho = 0.8f, guard = 0.49f;
    update_rho(&rho, &guard, hundred);
    CHECK(rho == smallest - 0.015f && guard == 0.5f * (0.49f + (third - 0.015f)), "size / 50 point: %g %g", rho, guard);
    rho = guard = 0.8f;
    std::vector<float> low{0.03f};
    update_rho(&rho, &guard, low);
    CHECK(rho == 0.05f && guard == 0.05f, "lower clamp: %g %g", rho, guard);
    rho = guard = 0.99f;
    std::vector<float> high{1.5f};
    update_rho(&rho, &guard, high);
    CHECK(rho == 0.99f && guard == 0.99f, "upper clamp: %g %g", rho, guard);
}

// ------------------------------------------------------------------------------------------------ classify_any
NOINLINE static void test_classify() {
    g_case = "classify_any";
    Batch b;
    Rng r(20254);
    b.add(random_dag(r, 40), 30);
    Dag fan;  // 256 predecessors: only the wide kernel takes it
    std::vector<uint32_t> all;
    for (uint32_t m = 0; m < 256; m++) fan.node(m, {}), all.push_back(m);
    fan.node(256, all);
    b.add(fan, 20);
    b.add(random_dag(r, 10), SINA_HIP_MAX_QUERY_LEN + 1);  // too long for the fast kernel
    std::vector<uint8_t> wide;
    CHECK(classify_any(b.batch(), b.qoff.data(), false, &wide) == 0 && wide == (std::vector<uint8_t>{0, 1, 1}), "routing");
    CHECK(classify_any(b.batch(), b.qoff.data(), true, &wide) == 0 && wide == (std::vector<uint8_t>{1, 1, 1}), "all wide");
    const uint32_t m = node_with_pred(b.dags[0], 20);
    b.pred[b.edge_off[0] + b.dags[0].pred_off[m]] = m;  // a node as its own predecessor
    CHECK(classify_any(b.batch(), b.qoff.data(), false, &wide) == 1 && g_err_limit == 0, "a malformed DAG is a plain error");
}

// ------------------------------------------------------------------------------------------------ dp_geom_for
// pick_geom as it stood in mesh_dp.hip before the geometry moved into dp_plan.h (less its test hook), kept to sweep against
static bool geom_before(uint32_t maxL, DpGeom *g) {
    static const int cells[] = {4, 8, 12};
    static const double rate[] = {226.0, 461.0, 403.0};
    for (int i = 0; i < 3; i++)
        if (maxL <= 64u * (uint32_t)cells[i]) {
            g->T = 64;
            g->B = cells[i];
            return true;
        }
    double best = 0;
    bool found = false;
    for (int i = 1; i < 3; i++) {
        const int b = cells[i];
        const uint32_t strips = (maxL + 64u * b - 1) / (64u * b);
        if (strips > 40u) continue;
        const double cost = (double)(strips * 64u * b) / rate[i];
        if (!found || cost < best) {
            best = cost;
            g->T = (int)strips * 64;
            g->B = b;
            found = true;
        }
    }
    return found;
}
NOINLINE static void test_geometry() {
    g_case = "dp_geom_for";
    struct Case {
        uint32_t maxL;
        int T, B;  // T = 0: no geometry
    };
    const Case cases[] = {{1, 64, 4},       {256, 64, 4},     {257, 64, 8},       {512, 64, 8},       {513, 64, 12},
                          {768, 64, 12},    {769, 128, 8},    {1024, 128, 8},     {1025, 192, 8},     {10240, 1280, 8},
                          {20480, 2560, 8}, {20481, 1728, 12}, {30720, 2560, 12}, {30721, 0, 0}};
    for (const Case &c : cases) {
        DpGeom g{-1, -1};
        const bool ok = dp_geom_for(c.maxL, 0, 0, &g);
        CHECK(ok == (c.T != 0), "maxL %u: %s", c.maxL, ok ? "a geometry where none covers it" : "no geometry");
        if (ok) CHECK(g.T == c.T && g.B == c.B, "maxL %u: (%d, %d), expected (%d, %d)", c.maxL, g.T, g.B, c.T, c.B);
    }
    // every length: what pick_geom answered; and with the rates as measured, B = 12 wins no multi-strip launch that
    // B = 8 has the strips for (up to 40 x 512 = 20480 columns) -- whoever re-measures kLaneRate sees that move here
    for (uint32_t maxL = 1; maxL <= 31000; maxL++) {
        DpGeom g{-1, -1}, w{-1, -1};
        const bool ok = dp_geom_for(maxL, 0, 0, &g), want = geom_before(maxL, &w);
        CHECK(ok == want && (!ok || (g.T == w.T && g.B == w.B)), "maxL %u: (%d, %d), pick_geom gave (%d, %d)", maxL, g.T, g.B, w.T, w.B);
        CHECK(ok == (maxL <= 30720), "maxL %u: covered %d", maxL, (int)ok);
        if (ok) CHECK((uint32_t)g.Lp() >= maxL && g.T % 64 == 0 && g.T <= 64 * kMaxStrips, "maxL %u: (%d, %d) does not cover it", maxL, g.T, g.B);
        if (maxL > 768 && maxL <= 20480) CHECK(g.B == 8, "maxL %u: B = %d where B = 8 has the strips", maxL, g.B);
        if (maxL > 20480 && ok) CHECK(g.B == 12, "maxL %u: B = %d beyond B = 8's 40 strips", maxL, g.B);
    }
    // a forced geometry: taken if the kernels have it and it covers maxL ...
    auto forced = [](uint32_t maxL, int T, int B) {
        DpGeom g{-1, -1};
        CHECK(dp_geom_for(maxL, T, B, &g), "maxL %u forced (%d, %d): no geometry", maxL, T, B);
        return g;
    };
    auto is = [](const DpGeom &g, int T, int B) { return g.T == T && g.B == B; };
    CHECK(is(forced(900, 128, 8), 128, 8), "forced (128, 8)");
    CHECK(is(forced(900, 256, 4), 256, 4) && is(forced(900, 192, 12), 192, 12) && is(forced(1, 64 * 40, 12), 2560, 12), "forced, accepted");
    // ... else ignored: the unforced answer for 900 bases is (128, 8)
    CHECK(is(forced(900, 0, 0), 128, 8), "unforced");
    CHECK(is(forced(900, 64, 12), 128, 8), "forced (64, 12) covers 768 of 900 bases");
    CHECK(is(forced(900, 96, 12), 128, 8), "forced T = 96");
    CHECK(is(forced(900, 64 * 41, 4), 128, 8), "forced T = 64 * 41");
    CHECK(is(forced(900, 256, 6), 128, 8), "forced B = 6");
    CHECK(is(forced(900, 0, 8), 128, 8) && is(forced(900, -128, 8), 128, 8), "forced T <= 0");
    DpGeom none{-1, -1};
    CHECK(!dp_geom_for(30721, 64 * 40, 12, &none), "a forced geometry that does not cover the query made one");
}

// ------------------------------------------------------------------------------------------------ dp_ring_plan
NOINLINE static void test_ring_plan() {
    g_case = "dp_ring_plan";
    const size_t want_lds[] = {6192, 12336, 18480};
    for (int i = 0; i < 3; i++) {
        const DpGeom g{128, 4 * (i + 1)};
        const size_t slot = dp_slot_bytes(g);
        CHECK(slot == (size_t)64 * g.B * 8 + 16, "slot bytes");
        auto plan = [&](size_t budget) {
            DpPlan pl{};
            dp_ring_plan(g, budget, &pl);
            CHECK(pl.geom.T == g.T && pl.geom.B == g.B && pl.lds == (size_t)pl.W * slot, "B %d budget %zu: geometry / lds", g.B, budget);
            return pl.W;
        };
        DpPlan def{};
        dp_ring_plan(g, 0, &def);
        CHECK(def.W == 3 && def.lds == want_lds[i], "B %d: default ring %d, %zu bytes", g.B, def.W, def.lds);
        CHECK(plan(dp_default_lds_budget(g)) == 3, "B %d: the default budget, given", g.B);
        CHECK(plan(1) == 1 && plan(slot - 1) == 1, "B %d: a budget below one slot", g.B);
        // (160 KB hold 26 slots and more: the clamp comes first, the ring's depth second)
        CHECK(160 * 1024 / slot > (size_t)kDpMaxRing && plan(1u << 20) == kDpMaxRing && kDpMaxRing == 8, "B %d: 1 MB", g.B);
        for (int k = 2; k <= kDpMaxRing; k++)
            CHECK(plan(k * slot) == k && plan(k * slot - 1) == k - 1, "B %d: budgets around %d slots", g.B, k);
        CHECK(plan((kDpMaxRing + 1) * slot) == kDpMaxRing, "B %d: nine slots' budget", g.B);
    }
}

// ------------------------------------------------------------------------------------------------ bt_by_lanes
NOINLINE static void test_lanes_rule() {
    g_case = "bt_by_lanes";
    CHECK(!bt_by_lanes(8191, 2048, -1) && bt_by_lanes(8192, 2048, -1) && !bt_by_lanes(8192, 2049, -1), "thresholds");
    CHECK(bt_by_lanes(1u << 20, 64, -1) && !bt_by_lanes(1, 64, -1) && !bt_by_lanes(1u << 20, 4096, -1), "far from the thresholds");
    for (uint32_t nq : {1u, 8191u, 8192u})
        for (uint32_t cap : {2048u, 2049u})
            CHECK(!bt_by_lanes(nq, cap, 0) && bt_by_lanes(nq, cap, 1), "forced, %u queries of %u bases", nq, cap);
}

// ------------------------------------------------------------------------------------------------ --words
// `dp_plan_check --words FILE RING`: prep_range's words of one DAG read from FILE, for tests/test_graph_cpu.py to compare
// with tests/graph_ref.py dp_words.  FILE is text: N E, then N columns, N masks, N weights (float bits), N + 1 pred_off,
// E predecessors.  The DAG passes the checks above first; then a line "sizes N spill-rows first-sink", a line "z w" per
// row and a line per predecessor entry.
NOINLINE static int print_words(const char *path, int W) {
    g_case = "--words";
    FILE *f = fopen(path, "r");
    CHECK(f != nullptr, "cannot read %s", path);
    unsigned n = 0, e = 0;
    CHECK(fscanf(f, "%u %u", &n, &e) == 2 && W >= 1 && W <= kDpMaxRing, "header / ring");
    Dag d;
    d.pos.resize(n), d.mask.resize(n), d.weight.resize(n), d.pred_off.resize(n + 1), d.pred.resize(e);
    auto read = [&](uint32_t *out) {
        unsigned v;
        CHECK(fscanf(f, "%u", &v) == 1, "short file");
        *out = v;
    };
    for (auto &x : d.pos) read(&x);
    for (auto &x : d.mask) {
        uint32_t v;
        read(&v);
        x = (uint8_t)v;
    }
    for (auto &x : d.weight) {
        uint32_t v;
        read(&v);
        memcpy(&x, &v, 4);
    }
    for (auto &x : d.pred_off) read(&x);
    for (auto &x : d.pred) read(&x);
    fclose(f);
    CHECK(d.pred_off[0] == 0 && d.pred_off[n] == e, "pred_off");
    Batch b;
    b.add(d, 10);
    check_prep(b, 0, 1, 512, W, 128.f);
    HostPrep hp;
    CHECK(prep_range(b.batch(), b.qoff.data(), 0, 1, 512, W, &hp, 0.f, nullptr) == 0, "prep_range failed: %s", g_err.c_str());
    printf("sizes %u %u %u\n", hp.qd[0].N, hp.qd[0].n_spill, hp.qd[0].first_sink);
    for (uint32_t m = 0; m < n; m++) printf("%u %u\n", hp.rec[m].z, hp.rec[m].w);
    for (uint32_t x = 0; x < e; x++) printf("%u\n", hp.pred[x]);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "--words")) return print_words(argv[2], atoi(argv[3]));
    test_prep_range();
    test_prep_directed();
    test_cut_range();
    test_families();
    test_family_qdescs();
    test_sweep_and_rho();
    test_classify();
    test_geometry();
    test_ring_plan();
    test_lanes_rule();
    printf("dp_plan_check: ok\n");
    return 0;
}
