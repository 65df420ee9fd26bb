// C-ABI entry points of include/sina_hip.h: context, reference store, alignment.
// (The k-mer search's entry points live in kmer_launch.hip, the index's in kmer_index.hip, the device DAG build in
// graph_build.hip, the DP driver in dp_launch.hip.)
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "ctx.h"

namespace sina_hip {

static thread_local std::string g_last_error;
static thread_local bool g_last_error_is_limit = false;
void set_error(const std::string &msg) {
    g_last_error = msg;
    g_last_error_is_limit = false;
}
void set_limit_error(const std::string &msg) {
    g_last_error = msg;
    g_last_error_is_limit = true;
}

// The two streams of a context: uploads, k-mer searches' copies ... on `stream`; DP hand-over, result copies (and, for a
// launch that is not chained, the backtrack walk) on `stream_dp`.  Both at the DEFAULT priority since round 4.
// Rounds 1-3 created `stream` at the highest and `stream_dp` at the lowest priority (round 1: kernels of different
// batches overlapped freely and a DAG build starved beside a DP kernel).  Since the device-filling kernels go through
// the store's FIFO that no longer decides anything -- except that a lowest-priority walk is not dispatched while a
// default-priority kernel still has workgroups to hand out: with one more stream in the process the walk started
// 5 ms late in half of the launches, ran beside the next DP launch and took 16 ms instead of 7
// (profiles/r04_bt_delay.txt).
int make_streams(sina_hip_ctx *c) {
    SH_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    SH_CHECK(hipStreamCreateWithFlags(&c->stream_dp, hipStreamNonBlocking));
    return 0;
}

// The dynamic-LDS ceiling of a kernel is raised ONCE per kernel and device to all of a CU's 160 KB (a
// per-launch size would race between contexts launching from different host threads; the attribute belongs
// to the current device's function object, so a process with contexts on several devices sets it on each).
int allow_full_lds(const void *kernel) {
    static std::mutex mu;
    static std::vector<std::pair<int, const void *>> done;
    int dev = 0;
    SH_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    for (const auto &k : done)
        if (k.first == dev && k.second == kernel) return 0;
    hipFuncAttributes fa;
    SH_CHECK(hipFuncGetAttributes(&fa, kernel));  // (the ceiling is what the kernel's static LDS leaves of the 160 KB)
    const int room = 160 * 1024 - (int)fa.sharedSizeBytes;
    SH_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, room));
    done.emplace_back(dev, kernel);
    return 0;
}

// What sina_hip_debug_mesh asks of its one query: the planes, unpacked cell by cell (value: optional), and whether the
// row skip stays on.
struct MeshDebug {
    float *value;
    uint32_t *vm, *vs;
    bool prune;
};

// single-query debug: unpack the planes of the launch just run (hp: its one query)
static int unpack_debug_planes(sina_hip_ctx *c, const HostPrep &hp, int Lp, bool forbid, const MeshDebug &dbg) {
    const QDesc &d = hp.qd[0];
    std::vector<uint32_t> tbh((size_t)d.N * Lp);
    if (forbid) {
        SH_CHECK(hipMemcpy(tbh.data(), c->last_tb, 4 * tbh.size(), hipMemcpyDeviceToHost));
    } else {  // 16-bit cells (common.h)
        std::vector<uint16_t> t16(tbh.size());
        SH_CHECK(hipMemcpy(t16.data(), c->last_tb, 2 * t16.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < tbh.size(); i++) tbh[i] = t16[i];
    }
    std::vector<float> vh;
    if (dbg.value) {
        vh.resize(tbh.size());
        SH_CHECK(hipMemcpy(vh.data(), c->dbg.p, 4 * vh.size(), hipMemcpyDeviceToHost));
    }
    // value_midx of a gap-extending deletion is the predecessor's gapm_idx (common.h, Ext / OpLast)
    const uint4 *rec = hp.rec.data() + d.node_off;
    const uint32_t *pr = hp.pred.data() + d.edge_off;
    const uint32_t ext_bit = forbid ? kTbExt : kTb16Ext;
    auto gapm_idx = [&](uint32_t x, uint32_t col) -> uint32_t {
        for (;;) {
            const uint32_t np = rec[x].z & 0xffu;
            if (np == 0) return 0;
            const uint32_t lastp = pr[rec[x].x + np - 1] & 0xffffu;
            const uint32_t cx = tbh[(size_t)x * Lp + col];
            if (forbid ? (cx & kTbOpLast) != 0 : !(cx & kTb16XLast)) return lastp;
            x = lastp;
        }
    };
    for (uint32_t m = 0; m < d.N; m++)
        for (uint32_t x = 0; x < d.L; x++) {
            const uint32_t cell = tbh[(size_t)m * Lp + x];
            uint32_t vm, vs;
            if (forbid) {
                vm = cell >> 16;
                vs = cell & kTbSMask;
            } else {  // type code + predecessor ordinal instead of the indices
                const uint32_t t = cell & kTbTypeMask;
                vm = t == kTbIns ? m : (t == kTbNone ? 0u : (pr[rec[m].x + (cell >> kTb16OrdShift)] & 0xffffu));
                if (t == kTbNone) vs = 0;
                else if (t == kTbMatch) vs = x - 1;
                else if (t == kTbDel) vs = x;
                else {  // insertion: where the run of insertion cells to the left ends
                    uint32_t k = x - 1;
                    while (k > 0 && (tbh[(size_t)m * Lp + k] & kTbTypeMask) == kTbIns) --k;
                    vs = k;
                }
            }
            if (cell & ext_bit) vm = gapm_idx(vm, x);
            dbg.vm[(size_t)m * d.L + x] = vm;
            dbg.vs[(size_t)m * d.L + x] = vs;
            if (dbg.value) dbg.value[(size_t)m * d.L + x] = vh[(size_t)m * Lp + x];
        }
    return 0;
}

// [qa, qb): the queries of the batch to align (qa = 0, qb = 0: all of them); every offset of the batch is absolute, the
// staged columns are laid out for the whole batch.  done_to / spill_q (sina_hip_align_graphs_any): on failure, the
// queries before *done_to have their results, and *spill_q names the query that needs too many spill rows (if that
// is why; it then goes through the wide kernel).  dbg: sina_hip_debug_mesh.
static int align_graphs_impl(sina_hip_ctx *c, const sina_hip_graph_batch *g, const uint8_t *qmask,
                             const uint64_t *qoff, const sina_hip_align_params *p, sina_hip_align_out *out,
                             uint32_t *out_pos, const MeshDebug *dbg = nullptr,
                             uint32_t qa = 0, uint32_t qb = 0, uint32_t *done_to = nullptr, uint32_t *spill_q = nullptr,
                             const uint32_t *weight_set = nullptr, uint32_t n_sets = 1) {
    if (!c || !g || !qmask || !qoff || !p || !out) SH_FAIL("align_graphs: null argument");
    const uint32_t nq = g->nq;
    const bool per_query_sets = weight_set != nullptr;
    if (check_weight_sets("align_graphs_wsets", p, &weight_set, &n_sets, nq)) return 1;
    if (per_query_sets && g->node_score16 != nullptr)
        SH_FAIL("align_graphs_wsets: a profile batch takes no positional weights (scoring_scheme_profile)");
    if (nq == 0) return 0;
    if (qb == 0) qb = nq;
    if (done_to) *done_to = qa;
    SH_CHECK(hipSetDevice(c->device));
    if (c->h_out_pos.reserve(4 * std::max<uint64_t>(qoff[nq] - qoff[0], 1))) return 1;
    const bool forbid = p->insertion == SINA_INSERTION_FORBID;
    if (forbid && !g->succ_minpos) SH_FAIL("align_graphs: insertion=forbid needs succ_minpos");
    uint32_t maxL = 0;
    for (uint32_t q = qa; q < qb; q++) {
        const uint64_t L = qoff[q + 1] - qoff[q];
        const uint64_t N = g->node_off[q + 1] - g->node_off[q];
        if (L == 0 || N == 0) SH_FAIL("align_graphs: empty query or graph");
        if (L > SINA_HIP_MAX_QUERY_LEN || N > 65535) SH_FAIL_LIMIT("align_graphs: query longer than SINA_HIP_MAX_QUERY_LEN bases or DAG of more than 65535 nodes");
        maxL = std::max<uint32_t>(maxL, (uint32_t)L);
    }
    DpPlan pl;
    if (plan_dp(c, maxL, &pl)) return 1;
    const int Lp = pl.geom.Lp();
    if (upload_weights(c, p, n_sets)) return 1;
    float wmax = 0.f, wmin = 0.f;
    if (!g->node_score16 && g->node_weight) {
        const uint64_t n_all = g->node_off[qb] - g->node_off[qa];
        for (uint64_t i = 0; i < n_all; i++) {
            const float w = g->node_weight[g->node_off[qa] + i];
            if (!(w == w)) wmax = wmin = NAN;  // (a NaN compares false both ways and would slip through: it switches the row skip off)
            if (!(wmax == wmax)) break;
            wmax = (i == 0 || w > wmax) ? w : wmax;
            wmin = (i == 0 || w < wmin) ? w : wmin;
        }
    }
    const bool profile_batch = g->node_score16 != nullptr;
    PrunePlan pp = prune_plan(p, wmax, wmin, maxL, profile_batch);
    if (dbg && !dbg->prune) pp.on = 0;

    const uint64_t tb_budget_cells = tb_plane_budget(c) / tb_cell_bytes(forbid);
    const uint32_t slots = dp_wave_slots(c, pl.geom.B);
    // (SINA_HIP_TEST=dp_range_q=N: at most N queries per DP launch range, so that a small call takes several)
    const uint32_t range_q = (uint32_t)strtoul(test_knob("dp_range_q").c_str(), nullptr, 10);
    auto nodes_of = [&](uint32_t q) { return g->node_off[q + 1] - g->node_off[q]; };
    HostPrep hp;
    for (uint32_t q0 = qa, q1; q0 < qb; q0 = q1) {
        // largest sub-batch whose trace-back plane fits the budget
        q1 = dbg ? q0 + 1 : dp_cut_range(nodes_of, q0, qb, Lp, tb_budget_cells, slots);
        if (range_q != 0) q1 = std::min(q1, q0 + range_q);
        if (prep_range(g, qoff, q0, q1, Lp, pl.W, &hp, pp.on ? pp.kappa64 : 0.f, spill_q)) return 1;
        const uint32_t bq = q1 - q0;
        const uint64_t nbase = g->node_off[q0], nn = g->node_off[q1] - nbase;
        const uint64_t ebase = g->edge_off[q0], ne = g->edge_off[q1] - ebase;
        const uint64_t qbase = qoff[q0], nqm = qoff[q1] - qbase;
        if (c->qd.reserve(sizeof(QDesc) * bq) || c->rec.reserve(sizeof(uint4) * nn) || c->node_pos.reserve(4 * nn) ||
            c->pred.reserve(4 * std::max<uint64_t>(ne, 1)) || c->pred4.reserve(sizeof(uint2) * nn) || c->succ_minpos.reserve(4 * nn) ||
            c->qmask.reserve(nqm) || (pp.on && c->rgain.reserve(8 * nn)))
            return 1;
        hipStream_t s = c->stream;
        SH_CHECK(hipMemcpyAsync(c->qd.p, hp.qd.data(), sizeof(QDesc) * bq, hipMemcpyHostToDevice, s));
        SH_CHECK(hipMemcpyAsync(c->rec.p, hp.rec.data(), sizeof(uint4) * nn, hipMemcpyHostToDevice, s));
        SH_CHECK(hipMemcpyAsync(c->node_pos.p, g->node_pos + nbase, 4 * nn, hipMemcpyHostToDevice, s));
        if (ne) SH_CHECK(hipMemcpyAsync(c->pred.p, hp.pred.data(), 4 * ne, hipMemcpyHostToDevice, s));
        SH_CHECK(hipMemcpyAsync(c->pred4.p, hp.pred4.data(), sizeof(uint2) * nn, hipMemcpyHostToDevice, s));
        if (g->succ_minpos)
            SH_CHECK(hipMemcpyAsync(c->succ_minpos.p, g->succ_minpos + nbase, 4 * nn, hipMemcpyHostToDevice, s));
        SH_CHECK(hipMemcpyAsync(c->qmask.p, qmask + qbase, nqm, hipMemcpyHostToDevice, s));
        PrunePlan pp_launch = pp;
        if (!hp.rgain_ok) pp_launch.on = 0;
        if (pp.on) SH_CHECK(hipMemcpyAsync(c->rgain.p, hp.rgain.data(), 8 * nn, hipMemcpyHostToDevice, s));
        if (profile_batch) {  // --fs-no-graph: the profile's match-term tables (sina_hip.h)
            if (!g->self_score16) SH_FAIL("align_graphs: node_score16 without self_score16");
            if (weighted_scheme(p)) SH_FAIL("align_graphs: a profile batch takes no positional weights (scoring_scheme_profile)");
            if (c->prof16.reserve(64 * std::max<uint64_t>(nn, 1)) || c->self16.reserve(64)) return 1;
            SH_CHECK(hipMemcpyAsync(c->prof16.p, g->node_score16 + 16 * nbase, 64 * nn, hipMemcpyHostToDevice, s));
            SH_CHECK(hipMemcpyAsync(c->self16.p, g->self_score16, 64, hipMemcpyHostToDevice, s));
        }
        DpLaunch l;
        l.qd = hp.qd.data();
        l.bq = bq;
        l.nqm = nqm;
        l.width = g->width;
        l.out = out + q0;
        l.out_pos = out_pos ? out_pos + qbase : nullptr;
        l.out_pos_base = qbase - qoff[0];
        l.q_base = q0;
        l.profile_batch = profile_batch;
        l.debug_planes = dbg != nullptr;
        l.want_dbg_value = dbg && dbg->value;
        l.wset = weight_set ? weight_set + q0 : nullptr;
        if (run_dp_device(c, pl, pp_launch, p, l)) return 1;
        if (dbg && unpack_debug_planes(c, hp, Lp, forbid, *dbg)) return 1;
        if (done_to) *done_to = q0 + bq;
    }
    return 0;
}

static int align_graphs_any_impl(sina_hip_ctx *c, const sina_hip_graph_batch *g, const uint8_t *qmask, const uint64_t *qoff,
                                 const sina_hip_align_params *p, sina_hip_align_out *out, uint32_t *out_pos) {
    if (!c || !g || !qmask || !qoff || !p || !out) SH_FAIL("align_graphs_any: null argument");
    const uint32_t nq = g->nq;
    if (nq == 0) return 0;
    SH_CHECK(hipSetDevice(c->device));
    if (p->insertion == SINA_INSERTION_FORBID && !g->succ_minpos) SH_FAIL("align_graphs_any: insertion=forbid needs succ_minpos");
    if (g->node_score16 != nullptr) {
        if (!g->self_score16) SH_FAIL("align_graphs_any: node_score16 without self_score16");
        if (weighted_scheme(p)) SH_FAIL("align_graphs_any: a profile batch takes no positional weights (scoring_scheme_profile)");
    } else if (!g->node_mask || !g->node_weight) {
        SH_FAIL("align_graphs_any: null argument");
    }
    std::vector<uint8_t> wide;
    if (classify_any(g, qoff, test_knob("wide") == "1", &wide)) return 1;
    if (c->h_out_pos.reserve(4 * std::max<uint64_t>(qoff[nq] - qoff[0], 1))) return 1;
    std::vector<uint32_t> qs;
    uint32_t q = 0;
    while (q < nq) {
        uint32_t e = q;
        while (e < nq && wide[e] == wide[q]) e++;
        if (wide[q]) {  // a run of queries for the wide kernel
            qs.resize(e - q);
            for (uint32_t i = q; i < e; i++) qs[i - q] = i;
            if (run_wide(c, g, qmask, qoff, p, qs.data(), e - q, out, out_pos)) return 1;
            q = e;
            continue;
        }
        // a maximal run of fitting queries through the fast path, unchanged -- up to a query that needs too many
        // spill rows: the run is split there, that one query goes wide
        uint32_t done_to = q, spill_q = 0xFFFFFFFFu;
        if (align_graphs_impl(c, g, qmask, qoff, p, out, out_pos, nullptr, q, e, &done_to, &spill_q)) {
            if (spill_q == 0xFFFFFFFFu || spill_q < done_to || spill_q >= e) return 1;
            wide[spill_q] = 1;
            q = done_to;  // (the queries before it have their results; [done_to, spill_q) run again as a range of their own)
            continue;
        }
        q = e;
    }
    return 0;
}

}  // namespace sina_hip

using namespace sina_hip;

extern "C" {

int sina_hip_abi_version(void) { return SINA_HIP_ABI_VERSION; }
const char *sina_hip_last_error(void) { return g_last_error.c_str(); }
int sina_hip_last_error_is_limit(void) { return g_last_error_is_limit ? 1 : 0; }

// a partly built context is taken apart again when init / fork fails half-way
static void discard_ctx(sina_hip_ctx *c) {
    if (!c) return;
    for (auto &e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->stream_dp) (void)hipStreamDestroy(c->stream_dp);
    c->free_all();
    delete c;
}
static int finish_ctx(sina_hip_ctx *c) {  // streams + events of a new context
    for (auto &e : c->ev) e = nullptr;
    if (make_streams(c)) return 1;
    for (auto &e : c->ev) SH_CHECK(hipEventCreate(&e));
    return 0;
}

// Runs when the library is loaded, i.e. normally before the HIP runtime has started: the pipeline's
// streams need more hardware queues than the runtime's default of four (see sina_amd/__init__.py).
// ROC_SIGNAL_POOL_SIZE: the runtime recycles completion signals out of a pool (default 64); four batches in
// flight, each with a dozen copies, kernels and events on several streams, run it dry, and from then on the
// runtime's helper thread creates and waits for interrupt signals one ioctl at a time -- 0.8 of a core in
// kernel mode at 125 k sequences/s (bench.py under SINA_HOST_PROFILE=1: "timed region: thread ..." lines;
// tools/ubench/bench_env_matrix.sh).  With 256 the thread is idle for 16S (3.2 -> 2.5 busy cores, same rate);
// the V4 shape (365 k sequences/s) needs 1024 for that (7.9 -> 6.8).
// An explicit setting in the environment wins, and a host that wants its process environment left alone
// altogether sets SINA_HIP_NO_RUNTIME_DEFAULTS (to anything but "0") before it loads the library: nothing is
// touched then -- the pipeline still works, with the costs described above.
__attribute__((constructor)) static void sina_hip_runtime_defaults() {
    const char *off = getenv("SINA_HIP_NO_RUNTIME_DEFAULTS");
    if (off && *off && !(off[0] == '0' && off[1] == 0)) return;
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    setenv("ROC_SIGNAL_POOL_SIZE", "1024", 0);
}

int sina_hip_init(int device, sina_hip_ctx **ctx) {
    if (!ctx) SH_FAIL("init: null ctx pointer");
    int ndev = 0;
    SH_CHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) SH_FAIL("init: no such HIP device");
    SH_CHECK(hipSetDevice(device));
    sina_hip_ctx *c = new sina_hip_ctx();
    c->device = device;
    c->st = new sina_hip_store();
    c->owns_store = true;
    memset(&c->st->stats, 0, sizeof(c->st->stats));
    // (the FIFO of device-filling kernels: two streams taking turns + the "queue has run dry" words, ctx.h)
    auto make_heavy = [](sina_hip_store *st) {
        if (hipStreamCreateWithFlags(&st->heavy, hipStreamNonBlocking) != hipSuccess) return 1;
        if (hipStreamCreateWithFlags(&st->heavy2, hipStreamNonBlocking) != hipSuccess) return 1;
        for (auto &e : st->heavy_done)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return 1;
        for (auto &e : st->dp_end)
            if (hipEventCreate(&e) != hipSuccess) return 1;
        // (chained launches need hipStreamWaitValue32: a device without it keeps dry_mem == nullptr and every launch
        // waits for the end of the one before, as until round 3)
        int can_wait_value = 0;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&can_wait_value, hipDeviceAttributeCanUseStreamWaitValue, dev) != hipSuccess) {
            (void)hipGetLastError();
            can_wait_value = 0;
        }
        if (!can_wait_value) return 0;
        // (the flag word in signal memory -- what hipStreamWaitValue32 is documented for --, the counters in a plain block;
        // a runtime that will not give signal memory leaves the store unchained)
        if (hipExtMallocWithFlags(reinterpret_cast<void **>(&st->dry_flag), 8, hipMallocSignalMemory) != hipSuccess) {
            (void)hipGetLastError();
            st->dry_flag = nullptr;
            return 0;
        }
        const size_t bytes = 4 * (size_t)sina_hip_store::kDryCounters;
        if (hipMalloc(reinterpret_cast<void **>(&st->dry_mem), bytes) != hipSuccess) return 1;
        if (hipMemset(st->dry_flag, 0, 8) != hipSuccess) return 1;
        return hipMemset(st->dry_mem, 0, bytes) != hipSuccess ? 1 : 0;
    };
    if (finish_ctx(c) || make_heavy(c->st)) {
        const std::string why = sina_hip_last_error();
        discard_ctx(c);
        set_error(why.empty() ? "init: could not create the context's streams" : why);
        return 1;
    }
    c->bind_hints();
    c->lds_budget = (size_t)std::max(0, atoi(test_knob("lds_kb").c_str())) * 1024;  // (test hook: LDS per DP workgroup)
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->n_cu < 1) {
        (void)hipGetLastError();
        c->n_cu = 256;
    }
    *ctx = c;
    return 0;
}

int sina_hip_fork(sina_hip_ctx *parent, sina_hip_ctx **ctx) {
    if (!parent || !ctx) SH_FAIL("fork: null argument");
    SH_CHECK(hipSetDevice(parent->device));
    sina_hip_ctx *c = new sina_hip_ctx();
    c->device = parent->device;
    c->st = parent->st;  // same reference store, index and counters; never freed by the fork
    c->owns_store = false;
    c->lds_budget = parent->lds_budget;
    c->n_cu = parent->n_cu;
    // (the in-place counts' switches stay off: they are per context, sina_hip_align_count_pairs / _count_identity)
    c->bind_hints();
    if (finish_ctx(c)) {
        const std::string why = sina_hip_last_error();
        discard_ctx(c);
        set_error(why);
        return 1;
    }
    *ctx = c;
    return 0;
}

int sina_hip_prewarm(sina_hip_ctx *c, int kind) {
    if (!c || kind < 0 || kind > 2) SH_FAIL("prewarm: null ctx or unknown kind");
    std::lock_guard<std::mutex> lk(c->mu);
    SH_CHECK(hipSetDevice(c->device));
    return c->prewarm(kind);
}

void sina_hip_destroy(sina_hip_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->stream_dp) (void)hipStreamSynchronize(c->stream_dp);
    c->free_all();
    for (auto &e : c->ev) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->stream);
    if (c->stream_dp) (void)hipStreamDestroy(c->stream_dp);
    delete c;
}

int sina_hip_sync(sina_hip_ctx *c) {
    if (!c) SH_FAIL("sync: null ctx");
    SH_CHECK(hipSetDevice(c->device));
    SH_CHECK(hipStreamSynchronize(c->stream));
    SH_CHECK(hipStreamSynchronize(c->stream_dp));
    if (c->st->heavy) SH_CHECK(hipStreamSynchronize(c->st->heavy));
    if (c->st->heavy2) SH_CHECK(hipStreamSynchronize(c->st->heavy2));
    return 0;
}

const uint32_t *sina_hip_staged_out_pos(sina_hip_ctx *c) {
    return c ? static_cast<const uint32_t *>(c->h_out_pos.p) : nullptr;
}

void sina_hip_align_params_default(sina_hip_align_params *p) {
    memset(p, 0, sizeof(*p));
    p->match_score = 2;
    p->mismatch_score = -1;
    p->gap_penalty = 5;
    p->gap_ext_penalty = 2;
    p->fs_weight = 1;
    p->overhang = SINA_OVERHANG_ATTACH;
    p->lowercase = SINA_LOWERCASE_NONE;
    p->insertion = SINA_INSERTION_SHIFT;
}

int sina_hip_upload_refs(sina_hip_ctx *c, const uint32_t *ab, const uint64_t *off, uint32_t n_refs,
                         uint32_t width) {
    if (!c || !ab || !off) SH_FAIL("upload_refs: null argument");
    if (!c->owns_store) SH_FAIL("upload_refs: a forked context cannot change the reference store");
    std::lock_guard<std::mutex> lk(c->mu);
    SH_CHECK(hipSetDevice(c->device));
    const uint64_t total = off[n_refs];
    if (c->st->ref_ab.reserve(4 * std::max<uint64_t>(total, 1)) || c->st->ref_off.reserve(8 * ((uint64_t)n_refs + 1)))
        return 1;
    SH_CHECK(hipMemcpyAsync(c->st->ref_ab.p, ab, 4 * total, hipMemcpyHostToDevice, c->stream));
    SH_CHECK(hipMemcpyAsync(c->st->ref_off.p, off, 8 * ((uint64_t)n_refs + 1), hipMemcpyHostToDevice, c->stream));
    SH_CHECK(hipStreamSynchronize(c->stream));
    {
        std::lock_guard<std::mutex> alk(c->st->aux_mu);
        c->st->ref_off_host.assign(off, off + n_refs + 1);
        c->st->ref_off_host_ready.store(true, std::memory_order_release);
    }
    c->st->n_refs = n_refs;
    c->st->width = width;
    c->st->total_bases = total;
    c->st->have_refs = true;
    c->st->have_name_order = false;  // (sina_hip_upload_name_order: the order belonged to the references before)
    c->st->fam_meta_ready.store(false, std::memory_order_release);  // (family.hip: rebuilt by the next cascade)
    // and the index: its lists name the references before (an id at or above n_refs would take the count kernels
    // outside their counters) -- build or upload one again
    c->st->have_index = false;
    c->st->dense_ready = false;
    c->st->n_postings = 0;
    c->st->n_dense = 0;
    return 0;
}

int sina_hip_store_view_get(sina_hip_ctx *c, sina_hip_store_view *v) {
    if (!c || !v) SH_FAIL("store_view_get: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->st->have_refs) SH_FAIL("store_view_get: no references uploaded");
    memset(v, 0, sizeof(*v));
    v->ref_ab = c->st->ref_ab.p;
    v->ref_ab_bytes = 4 * c->st->total_bases;
    v->ref_off = c->st->ref_off.p;
    v->ref_off_bytes = 8 * ((uint64_t)c->st->n_refs + 1);
    v->n_refs = c->st->n_refs;
    v->width = c->st->width;
    v->total_bases = c->st->total_bases;
    if (c->st->have_index) {
        v->idx_offsets = c->st->idx_off.p;
        v->idx_offsets_bytes = 4 * ((1ull << (2 * c->st->k)) + 1);
        v->idx_ids = c->st->idx_ids.p;
        v->idx_ids_bytes = 4 * c->st->n_postings;
        v->k = c->st->k;
        v->nofast = c->st->nofast;
        v->n_postings = c->st->n_postings;
    }
    return 0;
}

int sina_hip_store_alloc_like(sina_hip_ctx *c, sina_hip_store_view *v) {
    if (!c || !v) SH_FAIL("store_alloc_like: null argument");
    if (v->k < 1 || v->k > 12) SH_FAIL("store_alloc_like: k must be in 1..12");
    if (!c->owns_store) SH_FAIL("store_alloc_like: a forked context cannot change the reference store");
    std::lock_guard<std::mutex> lk(c->mu);
    SH_CHECK(hipSetDevice(c->device));
    const uint64_t nk = 1ull << (2 * v->k);
    if (c->st->ref_ab.reserve(4 * std::max<uint64_t>(v->total_bases, 1)) ||
        c->st->ref_off.reserve(8 * ((uint64_t)v->n_refs + 1)) || c->st->idx_off.reserve(4 * (nk + 1)) ||
        c->st->idx_ids.reserve(4 * std::max<uint64_t>(v->n_postings, 1)))
        return 1;
    c->st->n_refs = v->n_refs;
    c->st->width = v->width;
    c->st->total_bases = v->total_bases;
    c->st->k = v->k;
    c->st->nofast = v->nofast;
    c->st->n_postings = v->n_postings;
    c->st->have_refs = c->st->have_index = true;
    c->st->have_name_order = false;
    c->st->fam_meta_ready.store(false, std::memory_order_release);
    c->st->dense_ready = false;  // (the index arrives by broadcast after this call: built by the first search)
    {   // re-read from the device, once, after the broadcast filled it (ensure_ref_off_host)
        std::lock_guard<std::mutex> alk(c->st->aux_mu);
        c->st->ref_off_host_ready.store(false, std::memory_order_release);
        c->st->ref_off_host.clear();
    }
    v->ref_ab = c->st->ref_ab.p;
    v->ref_ab_bytes = 4 * v->total_bases;
    v->ref_off = c->st->ref_off.p;
    v->ref_off_bytes = 8 * ((uint64_t)v->n_refs + 1);
    v->idx_offsets = c->st->idx_off.p;
    v->idx_offsets_bytes = 4 * (nk + 1);
    v->idx_ids = c->st->idx_ids.p;
    v->idx_ids_bytes = 4 * v->n_postings;
    return 0;
}

int sina_hip_align_graphs(sina_hip_ctx *c, const sina_hip_graph_batch *g, const uint8_t *qmask,
                          const uint64_t *qoff, const sina_hip_align_params *p, sina_hip_align_out *out,
                          uint32_t *out_pos) {
    if (!c) SH_FAIL("align_graphs: null ctx");
    align_call call(c);
    sina_hip_hint_guard hints(c);
    if (call.begin(kMayCountPairs, p, g ? g->nq : 0)) return 1;  // (no family comes to the device: no identity)
    if (call.begin_rank(p, qmask, qoff, g ? g->nq : 0)) return 1;
    return align_graphs_impl(c, g, qmask, qoff, p, out, out_pos);
}

int sina_hip_align_graphs_wsets(sina_hip_ctx *c, const sina_hip_graph_batch *g, const uint8_t *qmask,
                                const uint64_t *qoff, const sina_hip_align_params *p, const uint32_t *weight_set,
                                uint32_t n_sets, sina_hip_align_out *out, uint32_t *out_pos) {
    if (!c) SH_FAIL("align_graphs_wsets: null ctx");
    if (p && !weighted_scheme(p)) SH_FAIL("align_graphs_wsets: weight sets need positional weights (p->weights, p->n_weights)");
    align_call call(c);
    sina_hip_hint_guard hints(c);
    if (call.begin(kMayCountPairs, p, g ? g->nq : 0)) return 1;  // (no family comes to the device: no identity)
    if (call.begin_rank(p, qmask, qoff, g ? g->nq : 0)) return 1;
    return align_graphs_impl(c, g, qmask, qoff, p, out, out_pos, nullptr, 0, 0, nullptr, nullptr, weight_set, n_sets);
}

int sina_hip_align_graphs_any(sina_hip_ctx *c, const sina_hip_graph_batch *g, const uint8_t *qmask,
                              const uint64_t *qoff, const sina_hip_align_params *p, sina_hip_align_out *out,
                              uint32_t *out_pos) {
    if (!c) SH_FAIL("align_graphs_any: null ctx");
    align_call call(c);
    sina_hip_hint_guard hints(c);
    if (call.begin(kMayCountPairs, p, g ? g->nq : 0)) return 1;  // (no family comes to the device: no identity)
    if (call.begin_rank(p, qmask, qoff, g ? g->nq : 0)) return 1;
    return align_graphs_any_impl(c, g, qmask, qoff, p, out, out_pos);
}

int sina_hip_wide_queries(sina_hip_ctx *c, uint64_t *n) {
    if (!c || !n) SH_FAIL("wide_queries: null argument");
    return read_path_queries(c, kPathWide, n);
}

int sina_hip_debug_mesh_wide(sina_hip_ctx *c, const sina_hip_graph_batch *g, const uint8_t *qmask, uint32_t qlen,
                             const sina_hip_align_params *p, uint32_t *tb_vm, uint32_t *tb_vs, float *value) {
    if (!c || !g || g->nq != 1 || !qmask || !p || !tb_vm || !tb_vs) SH_FAIL("debug_mesh_wide: needs exactly one query");
    align_call call(c);  // (a debug call counts no pairs and no identity: nothing begins)
    SH_CHECK(hipSetDevice(c->device));
    if (p->insertion == SINA_INSERTION_FORBID && !g->succ_minpos) SH_FAIL("debug_mesh_wide: insertion=forbid needs succ_minpos");
    if (g->node_score16 != nullptr && (!g->self_score16 || weighted_scheme(p)))
        SH_FAIL("debug_mesh_wide: a profile batch needs self_score16 and takes no positional weights");
    const uint64_t qoff[2] = {0, qlen};
    std::vector<uint8_t> wide;
    if (classify_any(g, qoff, true, &wide)) return 1;
    if (c->h_out_pos.reserve(4 * std::max<uint64_t>(qlen, 1))) return 1;
    sina_hip_align_out o;
    const uint32_t q0 = 0;
    return run_wide(c, g, qmask, qoff, p, &q0, 1, &o, nullptr, tb_vm, tb_vs, value);
}

int sina_hip_debug_mesh(sina_hip_ctx *c, const sina_hip_graph_batch *g, const uint8_t *qmask, uint32_t qlen,
                        const sina_hip_align_params *p, uint32_t *tb_vm, uint32_t *tb_vs, float *value, int prune) {
    if (!c || !g || g->nq != 1 || !tb_vm || !tb_vs) SH_FAIL("debug_mesh: needs exactly one query");
    align_call call(c);  // (a debug call counts no pairs and no identity: nothing begins)
    const uint64_t qoff[2] = {0, qlen};
    sina_hip_align_out o;
    std::vector<uint32_t> pos(qlen);
    const MeshDebug dbg{value, tb_vm, tb_vs, prune != 0};
    return align_graphs_impl(c, g, qmask, qoff, p, &o, pos.data(), &dbg);
}

const uint32_t *sina_hip_staged_shift_log(sina_hip_ctx *c) {
    if (!c) {
        set_error("staged_shift_log: null ctx");
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    return c->shift.staged();
}

int sina_hip_assemble_stats(sina_hip_ctx *c, uint64_t *queries, uint64_t *assembled, uint64_t *shifted_queries, uint64_t *shifted_runs) {
    if (!c || !queries || !assembled || !shifted_queries || !shifted_runs) SH_FAIL("assemble_stats: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *queries = c->asm_use.queries;
    *assembled = c->asm_use.assembled;
    *shifted_queries = c->asm_use.shifted_queries;
    *shifted_runs = c->asm_use.shifted_runs;
    return 0;
}

// The assembly alone: the caller's columns and walk results go up as a launch's would lie on the device behind the
// walk, assemble_kernel runs over them, both come down again.  Everything the kernel indexes with is checked here.
int sina_hip_debug_assemble(sina_hip_ctx *c, const sina_hip_align_params *p, uint32_t width, const uint8_t *qmask, const uint64_t *qoff,
                            uint32_t nq, sina_hip_align_out *out, uint32_t *out_pos) {
    if (!c || !p || !qmask || !qoff || !out || !out_pos) SH_FAIL("debug_assemble: null argument");
    if (p->assemble != 1 && p->assemble != SINA_ASSEMBLE_SHIFT) SH_FAIL("debug_assemble: p->assemble must be 1 or 2");
    if (width == 0 || width > 0x1000000u) SH_FAIL("debug_assemble: width must be in 1..2^24");
    align_call call(c);
    sina_hip_hint_guard hints(c);
    if (nq == 0) return 0;
    const bool keep_over = p->overhang != SINA_OVERHANG_REMOVE;
    std::vector<QDesc> qd(nq);
    uint32_t max_l = 0;
    for (uint32_t q = 0; q < nq; q++) {
        if (qoff[q + 1] <= qoff[q] || qoff[q + 1] - qoff[q] > 65535) SH_FAIL("debug_assemble: query length must be in 1..65535");
        const uint64_t L = qoff[q + 1] - qoff[q];
        const sina_hip_align_out &o = out[q];
        if (o.status == 0) {
            if (o.cutoff_tail < 0 || o.cutoff_head < 0 || o.aligned_bases < 0) SH_FAIL("debug_assemble: negative count");
            const uint64_t first_q = (uint64_t)o.end_s + (keep_over ? (uint64_t)o.cutoff_tail : 0u);  // query index of append 0
            if (o.n_out > L || first_q >= L || (o.n_out != 0 && first_q + 1 < o.n_out))
                SH_FAIL("debug_assemble: query " + std::to_string(q) + ": n_out, end_s and cutoff_tail do not fit its length");
        }
        memset(&qd[q], 0, sizeof(QDesc));
        qd[q].q_off = qoff[q] - qoff[0];
        qd[q].L = (uint32_t)L;
        max_l = std::max<uint32_t>(max_l, (uint32_t)L);
    }
    const uint64_t nqm = qoff[nq] - qoff[0];
    SH_CHECK(hipSetDevice(c->device));
    if (call.begin(0, p, nq)) return 1;  // (no counts; the shift log of assemble = 2)
    if (c->qd.reserve(sizeof(QDesc) * nq) || c->qmask.reserve(nqm) || c->out.reserve(sizeof(sina_hip_align_out) * nq) ||
        c->out_pos.reserve(4 * nqm) || c->h_out.reserve(sizeof(sina_hip_align_out) * nq) || c->h_out_pos.reserve(4 * nqm) ||
        c->shift.reserve(nq))
        return 1;
    hipStream_t s = c->stream;
    for (uint32_t q = 0; q < nq; q++) out[q].assembled = out[q].nast_total = out[q].nast_longest = out[q].nast_last_run = 0;
    if (upload(c, 5, c->qd.p, qd.data(), sizeof(QDesc) * nq, s) || upload(c, 6, c->qmask.p, qmask + qoff[0], nqm, s) ||
        upload(c, 7, c->out.p, out, sizeof(sina_hip_align_out) * nq, s) || upload(c, 8, c->out_pos.p, out_pos + qoff[0], 4 * nqm, s))
        return 1;
    BtArgs b{};
    b.qd = c->qd.as<QDesc>();
    b.out = c->out.as<sina_hip_align_out>();
    b.out_pos = c->out_pos.as<uint32_t>();
    b.nq = nq;
    b.width = width;
    b.overhang = p->overhang;
    b.qmask = c->qmask.as<uint8_t>();
    b.lowercase = p->lowercase;
    b.asm_cap = max_l;
    b.shift_log = p->assemble == SINA_ASSEMBLE_SHIFT ? c->shift.rows.as<uint32_t>() : nullptr;
    SH_CHECK(hipEventRecord(c->ev[0], s));  // (no launch of the DP path is under way: the context's mutex is held)
    if (launch_assemble(b, s)) return 1;
    SH_CHECK(hipEventRecord(c->ev[1], s));
    SH_CHECK(hipMemcpyAsync(c->h_out.p, c->out.p, sizeof(sina_hip_align_out) * nq, hipMemcpyDeviceToHost, s));
    SH_CHECK(hipMemcpyAsync(c->h_out_pos.p, c->out_pos.p, 4 * nqm, hipMemcpyDeviceToHost, s));
    if (c->shift.copy(0, nq, s)) return 1;
    SH_CHECK(wait_stream(c, s));
    memcpy(out, c->h_out.p, sizeof(sina_hip_align_out) * nq);
    memcpy(out_pos + qoff[0], c->h_out_pos.p, 4 * nqm);
    float ms = 0;
    SH_CHECK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->debug_assemble_ms = ms;
    return 0;
}

int sina_hip_debug_assemble_ms(sina_hip_ctx *c, double *kernel_ms) {
    if (!c || !kernel_ms) SH_FAIL("debug_assemble_ms: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *kernel_ms = c->debug_assemble_ms;
    return 0;
}

int sina_hip_debug_dp_info(sina_hip_ctx *c, uint32_t q, sina_hip_dp_info *out) {
    if (!c || !out) SH_FAIL("debug_dp_info: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (q >= c->last_bq || !c->res.p) SH_FAIL("debug_dp_info: no such query in the last launch");
    SH_CHECK(hipSetDevice(c->device));
    DpResult r;
    SH_CHECK(hipMemcpy(&r, c->res.as<DpResult>() + q, sizeof r, hipMemcpyDeviceToHost));
    out->end_m = r.end_m;
    out->end_s = r.end_s;
    out->raw = r.raw;
    out->status = r.status;
    out->rows_swept = r.rows_done;
    out->cells_swept = r.cells_done;
    out->attempts = r.attempts;
    out->gain0 = r.gain0;
    out->ubound = r.ubound;
    out->prune_step = c->last_prune_step;
    out->kernel = c->last_kernel;
    QDesc d;
    SH_CHECK(hipMemcpy(&d, c->qd.as<QDesc>() + q, sizeof d, hipMemcpyDeviceToHost));
    out->prune_gmin = d.gmin;
    out->scout = NAN;
    if (c->last_scout && c->scout_u.p) SH_CHECK(hipMemcpy(&out->scout, c->scout_u.as<float>() + q, sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int sina_hip_debug_rgain(sina_hip_ctx *c, uint32_t n, uint32_t *out, uint32_t *cols_right) {
    if (!c || !out) SH_FAIL("debug_rgain: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->rgain.p || c->rgain.cap < 8 * (size_t)n) SH_FAIL("debug_rgain: no bound of that many nodes on the device");
    SH_CHECK(hipSetDevice(c->device));
    std::vector<uint2> tmp(n);
    SH_CHECK(hipMemcpy(tmp.data(), c->rgain.p, 8 * (size_t)n, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        out[i] = tmp[i].x;
        if (cols_right) cols_right[i] = tmp[i].y >> 16;
    }
    return 0;
}

int sina_hip_debug_chain_rows(sina_hip_ctx *c, uint16_t *out, uint32_t cap, uint32_t *len) {
    if (!c || !out || !len) SH_FAIL("debug_chain_rows: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->scout.p || !c->g_sizes.p) SH_FAIL("debug_chain_rows: no device-built DAG in this context");
    SH_CHECK(hipSetDevice(c->device));
    uint32_t sizes[kBuiltWords];
    SH_CHECK(hipMemcpy(sizes, c->g_sizes.p, sizeof sizes, hipMemcpyDeviceToHost));
    *len = sizes[kBuiltChainLen];
    const size_t n = std::min<size_t>(std::min<uint32_t>(*len, cap), c->scout.cap / 2);
    if (n) SH_CHECK(hipMemcpy(out, c->scout.p, 2 * n, hipMemcpyDeviceToHost));
    return 0;
}

int sina_hip_get_stats(sina_hip_ctx *c, sina_hip_stats *s) {
    if (!c || !s) SH_FAIL("get_stats: null argument");
    std::lock_guard<std::mutex> slk(c->st->stats_mu);
    *s = c->st->stats;
    s->n_dense_lists = c->st->dense_ready.load() ? c->st->n_dense : 0;
    return 0;
}

}  // extern "C"
