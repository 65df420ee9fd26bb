// The wide DP path behind sina_hip_align_graphs_any: the reference's mesh (src/mesh.h:55-144) as it is, every
// cell's seven (--insertion=forbid: eight) fields in HBM, full 32-bit row ids, column ids and predecessor counts,
// the caller's CSR read as given.  It takes what the fast kernel (mesh_dp.hip) refuses -- more than 65535 nodes,
// more than 255 predecessors, more than kMaxSpillRows far rows, more than SINA_HIP_MAX_QUERY_LEN bases -- and it
// is plain on purpose: one workgroup per query sweeps the anti-diagonals d = m + s in order (every read of cell
// (m, s) has a smaller d: SURVEY.md section 8), its threads take the cells of one diagonal, __syncthreads().
// Nothing is exchanged between workgroups.
#include <cstring>

#include "common.h"
#include "ctx.h"

namespace sina_hip {
namespace {

// One query of a launch.  The pointers lead into the launch's input block (sina_hip_ctx::wide_in).
struct WideQ {
    const uint32_t *pos, *pred_off, *pred, *succ_minpos, *snk;  // node columns; the caller's CSR; sinks, ascending
    const float *weight, *prof16;                               // node weights; --fs-no-graph: [16 * node + mask], else nullptr
    const uint8_t *mask, *qmask;
    uint64_t plane_off;  // first cell of this query in every plane
    uint64_t out_off;    // first entry of this query in the launch's out_pos
    uint32_t N, L, K, by_s, n_snk, pad_;
};

struct WideRes {
    uint32_t end_m, end_s;
    float raw;
    int32_t status;
};

// The planes of a launch of T cells, one after the other: value, gapm_val, gaps_val (f32), value_midx, value_sidx,
// gapm_idx, gaps_idx (u32) and, for --insertion=forbid, gaps_max (u32).
constexpr int kWidePlanes = 7, kWidePlanesForbid = 8;
enum { kPlValue = 0, kPlGapm, kPlGaps, kPlVm, kPlVs, kPlGmi, kPlGsi, kPlGmax };

struct WideArgs {
    const WideQ *q;
    uint32_t *planes;
    uint64_t T;
    const float *weights;
    uint32_t n_weights;
    float ms, mms, gp, gpe;  // scheme ctor args: -match, -mismatch, gap, gapext
    WideRes *res;
    // the walk
    sina_hip_align_out *out;
    uint32_t *out_pos;
    const float *self16;
    uint32_t nq, width;
    int overhang;
};

// Where cell (m, s) lies in a plane.  Diagonal-major: the cells of one anti-diagonal are neighbours, and so are
// the cells a diagonal reads on the two diagonals before it; a diagonal holds at most K = min(N, L) cells and is
// indexed by whichever of s and m is the shorter dimension's, so the plane has (N + L - 1) * K cells, fewer than
// twice the mesh.  (The reference's row-major [m][s] makes a diagonal's accesses stride L - 1: measured 4.5 times
// slower)
__device__ __forceinline__ uint64_t wide_idx(const WideQ &d, uint32_t m, uint32_t s) {
    return ((uint64_t)m + s) * d.K + (d.by_s ? s : m);
}

// the smallest (value, key) of the workgroup, the smaller key among equal values; every thread gets it
__device__ __forceinline__ void block_first_min(float &v, unsigned long long &k, float *sh_v, unsigned long long *sh_k) {
    const uint32_t tid = threadIdx.x, T = blockDim.x;
    sh_v[tid] = v;
    sh_k[tid] = k;
    __syncthreads();
    uint32_t stride = 1;
    while (stride < T) stride <<= 1;
    for (stride >>= 1; stride > 0; stride >>= 1) {
        if (tid < stride && tid + stride < T) {
            const float ov = sh_v[tid + stride];
            const unsigned long long ok = sh_k[tid + stride];
            if (ov < sh_v[tid] || (ov == sh_v[tid] && ok < sh_k[tid])) {
                sh_v[tid] = ov;
                sh_k[tid] = ok;
            }
        }
        __syncthreads();
    }
    v = sh_v[0];
    k = sh_k[0];
    __syncthreads();
}

// The recurrence as SURVEY.md section 8 states it ("DP recurrence spec"): init, deletion per predecessor in
// ascending order (the last predecessor's gapm wins), insertion, match, store.
template <bool WEIGHTED, bool FORBID>
__global__ void __launch_bounds__(1024) mesh_wide_kernel(WideArgs a) {
    __shared__ float sh_v[1024];
    __shared__ unsigned long long sh_k[1024];
    const WideQ d = a.q[blockIdx.x];
    const uint32_t N = d.N, L = d.L, T = blockDim.x, tid = threadIdx.x;
    float *value = reinterpret_cast<float *>(a.planes + kPlValue * a.T + d.plane_off);
    float *gapm_val = reinterpret_cast<float *>(a.planes + kPlGapm * a.T + d.plane_off);
    float *gaps_val = reinterpret_cast<float *>(a.planes + kPlGaps * a.T + d.plane_off);
    uint32_t *value_midx = a.planes + kPlVm * a.T + d.plane_off;
    uint32_t *value_sidx = a.planes + kPlVs * a.T + d.plane_off;
    uint32_t *gapm_idx = a.planes + kPlGmi * a.T + d.plane_off;
    uint32_t *gaps_idx = a.planes + kPlGsi * a.T + d.plane_off;
    uint32_t *gaps_max = FORBID ? a.planes + kPlGmax * a.T + d.plane_off : nullptr;
    const uint32_t nw1 = WEIGHTED ? a.n_weights - 1 : 0;

    const uint64_t n_diag = (uint64_t)N + L - 1;
    for (uint64_t dg = 0; dg < n_diag; ++dg) {
        const uint32_t s_lo = dg >= N ? (uint32_t)(dg - (N - 1)) : 0u;
        const uint32_t s_hi = dg < L ? (uint32_t)dg : L - 1;
        const uint32_t count = s_hi - s_lo + 1;
        const uint32_t trips = (count + T - 1) / T;  // (the same for every thread: nobody skips the barrier)
        for (uint32_t it = 0; it < trips; ++it) {
            const uint32_t i = it * T + tid;
            if (i >= count) continue;
            const uint32_t s = s_lo + i, m = (uint32_t)(dg - s);
            const uint32_t pb = d.pred_off[m], pe = d.pred_off[m + 1];
            // per-row constants (scoring_schemes.h:102-241; the weighted scheme's index past the last column is
            // guarded as mesh_dp_kernel guards it)
            float cM = 0.f, cX = 0.f, gd_open = a.gp, gd_ext = a.gpe, gi_open = a.gp;
            uint32_t mpos = 0;
            if (WEIGHTED || FORBID) mpos = d.pos[m];
            if (d.prof16 == nullptr) {
                const float wgt = d.weight[m];
                if constexpr (WEIGHTED) {
                    const float wp = a.weights[mpos < nw1 ? mpos : nw1];
                    cM = a.ms * wp * wgt;
                    cX = a.mms * wp * wgt;
                } else {
                    cM = a.ms * wgt;
                    cX = a.mms * wgt;
                }
            }
            if constexpr (WEIGHTED) {
                const float wp = a.weights[mpos < nw1 ? mpos : nw1];
                const float wp1 = a.weights[mpos + 1 < nw1 ? mpos + 1 : nw1];
                gd_open = a.gp * wp;
                gd_ext = a.gpe * wp;
                gi_open = a.gp * wp1;
            }
            // init
            const float iv = (pb == pe || s == 0) ? 1.0f : 1000000.0f;
            float v = iv, gm = iv, gs = iv;
            uint32_t vm = 0, vs = 0, gmi = 0, gsi = 0, gmax = 0;
            // deletion
            for (uint32_t e = pb; e < pe; ++e) {
                const uint32_t p = d.pred[e];
                const uint64_t ip = wide_idx(d, p, s);
                const float ov = value[ip] + gd_open;
                const float og = gapm_val[ip] + gd_ext;
                float cand;
                uint32_t cm;
                if (ov < og) {
                    gm = ov;
                    gmi = p;
                    cand = ov;
                    cm = p;
                } else {
                    gm = og;
                    gmi = gapm_idx[ip];
                    cand = og;
                    cm = gmi;
                }
                if (cand < v) {
                    v = cand;
                    vm = cm;
                    vs = s;
                }
            }
            if (s > 0) {
                // insertion
                const uint64_t il = wide_idx(d, m, s - 1);
                const float lv = value[il], lgs = gaps_val[il];
                const uint32_t lgsi = gaps_idx[il];
                const bool extend = lgs == lv;
                bool ins = true;
                uint32_t gmax_n = 0;
                if constexpr (FORBID) {
                    // int max_insert = min_mpos - pos - 1, passed as unsigned idx_type (mesh.h:480-489)
                    const uint32_t smax = (uint32_t)(int)(d.succ_minpos[m] - mpos - 1);
                    const uint32_t lgmax = gaps_max[il];
                    ins = smax >= 1 && (!extend || lgmax > 0);
                    gmax_n = extend ? lgmax - 1 : smax - 1;
                }
                if (ins) {
                    if (!extend) {
                        gs = lv + gi_open;
                        gsi = s - 1;
                    } else {
                        float gi_ext = a.gpe;
                        if constexpr (WEIGHTED) {
                            const uint32_t wi = mpos + 1 + ((s - 1) - lgsi);
                            gi_ext = a.gpe * a.weights[wi < nw1 ? wi : nw1];
                        }
                        gs = lgs + gi_ext;
                        gsi = lgsi;
                    }
                    gmax = gmax_n;
                    if (gs <= v) {
                        v = gs;
                        vs = gsi;
                        vm = m;
                    }
                }
                // match
                const uint32_t qm = d.qmask[s] & 0xfu;
                float csel;
                if (d.prof16 != nullptr) csel = d.prof16[16 * (size_t)m + qm];
                else csel = (d.mask[m] & qm) ? cM : cX;  // comp(): optimistic IUPAC match (aligned_base.h:153)
                for (uint32_t e = pb; e < pe; ++e) {
                    const uint32_t p = d.pred[e];
                    const float mv = value[wide_idx(d, p, s - 1)] + csel;
                    if (mv < v) {
                        v = mv;
                        vm = p;
                        vs = s - 1;
                    }
                }
            }
            // store
            const uint64_t ic = wide_idx(d, m, s);
            value[ic] = v;
            gapm_val[ic] = gm;
            gaps_val[ic] = gs;
            value_midx[ic] = vm;
            value_sidx[ic] = vs;
            gapm_idx[ic] = gmi;
            gaps_idx[ic] = gsi;
            if constexpr (FORBID) gaps_max[ic] = gmax;
        }
        __syncthreads();  // (the diagonal's stores before the next one's loads: all of it inside this workgroup)
    }

    // End cell (mesh.h:567-592): the first minimum in this order -- the first sink's last-column cell, every
    // row's last-column cell, then the sinks in order across all columns; only a strictly smaller value displaces.
    const float inf = __builtin_inff();
    float bv = inf;
    unsigned long long bk = ~0ull;
    for (uint64_t i = tid; i < (uint64_t)N + 1; i += T) {
        const uint32_t m = i == 0 ? d.snk[0] : (uint32_t)(i - 1);
        const float x = value[wide_idx(d, m, L - 1)];
        if (x < bv || (x == bv && i < bk)) {
            bv = x;
            bk = i;
        }
    }
    block_first_min(bv, bk, sh_v, sh_k);
    const uint32_t m1 = bk == 0 ? d.snk[0] : (uint32_t)(bk - 1);
    float cv = tid == 0 ? bv : inf;
    unsigned long long ck = tid == 0 ? 0ull : ~0ull;
    const uint64_t n_sc = (uint64_t)d.n_snk * L;
    for (uint64_t i = tid; i < n_sc; i += T) {
        const uint32_t m = d.snk[i / L], s = (uint32_t)(i % L);
        const float x = value[wide_idx(d, m, s)];
        if (x < cv || (x == cv && i + 1 < ck)) {
            cv = x;
            ck = i + 1;
        }
    }
    block_first_min(cv, ck, sh_v, sh_k);
    if (tid == 0) {
        WideRes r;
        r.end_m = ck == 0 ? m1 : d.snk[(ck - 1) / L];
        r.end_s = ck == 0 ? L - 1 : (uint32_t)((ck - 1) % L);
        r.raw = cv;
        r.status = 0;
        a.res[blockIdx.x] = r;
    }
}

// The cell walk of backtrack() (mesh.h:594-721) over the explicit (value_midx, value_sidx) planes, one lane per
// query: what walk_query (traceback.hip) emits with assemble = 0 -- tail overhang, the one-step deletion skip,
// sum_weight in the reference's order, head overhang, self16 for profiles.  The wide path never assembles.
__global__ void __launch_bounds__(64) mesh_wide_walk_kernel(WideArgs a) {
    const uint32_t q = blockIdx.x * 64u + threadIdx.x;
    if (q >= a.nq) return;
    const WideQ d = a.q[q];
    const WideRes r = a.res[q];
    const uint32_t *value_midx = a.planes + kPlVm * a.T + d.plane_off;
    const uint32_t *value_sidx = a.planes + kPlVs * a.T + d.plane_off;
    sina_hip_align_out o;
    o.status = r.status;
    o.end_m = r.end_m;
    o.end_s = r.end_s;
    o.raw = r.raw;
    o.sum_weight = 0.f;
    o.aligned_bases = 0;
    o.cutoff_head = o.cutoff_tail = 0;
    o.n_out = 0;
    o.assembled = o.nast_total = o.nast_longest = o.nast_last_run = 0;
    uint32_t *out = a.out_pos + d.out_off;
    const uint32_t width = a.width, L = d.L;
    uint32_t m = r.end_m, s = r.end_s, n = 0;
    auto emit = [&](uint32_t p) {
        if (n < L) out[n] = p;  // (tail + aligned + head never exceed the query: a guard, not a rule)
        n++;
    };
    // right hand overhang (:594-615)
    const int tail = (int)(L - 1 - s);
    o.cutoff_tail = tail;
    if (tail && a.overhang != SINA_OVERHANG_REMOVE) {
        int pos = (a.overhang == SINA_OVERHANG_ATTACH) ? (int)(width - 1 - d.pos[m] - (uint32_t)tail) : 0;
        for (int i = 0; i < tail; i++) {
            const int p = pos++;
            emit((uint32_t)(p > 0 ? p : 0));
        }
    }
    auto mscore_at = [&](uint32_t row, uint32_t si) -> float {  // tr.s.match(sum, ab2, ab1) with comp() == true
        if (a.self16 != nullptr) return a.self16[d.qmask[si] & 0xfu];
        const float wgt = d.weight[row];
        if (a.weights != nullptr) {
            const uint32_t nw1 = a.n_weights - 1, col = d.pos[row];
            return a.ms * a.weights[col < nw1 ? col : nw1] * wgt;
        }
        return a.ms * wgt;
    };
    unsigned int pos = width - 1 - d.pos[m];
    float sum_weight = 0.f;
    int aligned = 0;
    emit(pos);
    aligned++;
    sum_weight = sum_weight + mscore_at(m, s);
    // :642-685 (a source node has no predecessors)
    while (s != 0 && d.pred_off[m + 1] != d.pred_off[m]) {
        const uint64_t ic = wide_idx(d, m, s);
        const uint32_t snew = value_sidx[ic];
        m = value_midx[ic];
        if (snew != 0) {  // the one-step deletion skip (:653-655)
            const uint64_t i2 = wide_idx(d, m, snew);
            if (value_sidx[i2] == snew) m = value_midx[i2];
        }
        pos = width - 1 - d.pos[m];
        while (s != snew) {
            --s;
            emit(pos);
            aligned++;
            sum_weight = sum_weight + mscore_at(m, s);
        }
    }
    // left hand overhang (:690-721)
    if (s != 0) {
        o.cutoff_head = (int)s;
        if (a.overhang == SINA_OVERHANG_ATTACH) {
            while (s-- != 0) {
                ++pos;
                emit((width - 1 < pos) ? width - 1 : pos);
            }
        } else if (a.overhang == SINA_OVERHANG_EDGE) {
            int k = (int)s;
            while (k--) emit(width - (uint32_t)k - 1);
        }
    }
    o.sum_weight = sum_weight;
    o.aligned_bases = aligned;
    o.n_out = n;
    a.out[q] = o;
}

// a launch's inputs, packed into one block: every array starts on a 16-byte boundary
struct Packer {
    std::vector<unsigned char> bytes;
    template <typename T> size_t put(const T *src, size_t n) {
        const size_t at = (bytes.size() + 15) & ~(size_t)15;
        bytes.resize(at + n * sizeof(T));
        if (n) memcpy(bytes.data() + at, src, n * sizeof(T));
        return at;
    }
};

}  // namespace

uint64_t wide_budget_cells() {
    if (const std::string v = test_knob("wide_cells"); !v.empty()) return std::max<uint64_t>(1, strtoull(v.c_str(), nullptr, 10));
    return SINA_HIP_WIDE_CELLS;
}

int run_wide(sina_hip_ctx *c, const sina_hip_graph_batch *g, const uint8_t *qmask, const uint64_t *qoff,
             const sina_hip_align_params *p, const uint32_t *qs, uint32_t n, sina_hip_align_out *out, uint32_t *out_pos,
             uint32_t *dbg_vm, uint32_t *dbg_vs, float *dbg_value) {
    if (n == 0) return 0;
    hipStream_t s = c->stream;
    const bool weighted = weighted_scheme(p);
    const bool forbid = p->insertion == SINA_INSERTION_FORBID;
    const bool profile = g->node_score16 != nullptr;
    const int n_planes = forbid ? kWidePlanesForbid : kWidePlanes;
    const uint64_t budget = wide_budget_cells();
    c->last_bq = 0;  // (sina_hip_debug_dp_info: the context's res buffer holds no fast-kernel results from here on)
    if (upload_weights(c, p)) return 1;
    if (profile) {
        if (c->self16.reserve(64)) return 1;
        if (upload(c, 8, c->self16.p, g->self_score16, 64, s)) return 1;
    }
    auto cells_of = [&](uint32_t q) -> uint64_t {
        const uint64_t N = g->node_off[q + 1] - g->node_off[q], L = qoff[q + 1] - qoff[q];
        return (N + L - 1) * std::min(N, L);  // (below 2^63: classify_any, dp_plan.h)
    };
    std::vector<uint32_t> snk;
    std::vector<uint8_t> has_succ;
    uint32_t i0 = 0;
    while (i0 < n) {
        // the queries of one launch: as many as fit the budget
        uint32_t i1 = i0;
        uint64_t T = 0;
        while (i1 < n) {
            const uint64_t cq = cells_of(qs[i1]);
            if (cq > budget) {
                char msg[256];
                snprintf(msg, sizeof msg,
                         "align_graphs_any: the mesh of query %u needs %llu bytes, the wide path's budget is %llu bytes",
                         qs[i1], (unsigned long long)(cq * 4 * n_planes), (unsigned long long)(budget * 4 * n_planes));
                SH_FAIL(msg);
            }
            if (T + cq > budget) break;
            T += cq;
            i1++;
        }
        const uint32_t bq = i1 - i0;
        Packer pk;
        std::vector<WideQ> qd(bq);
        std::vector<size_t> at(9 * (size_t)bq);
        uint64_t plane_off = 0, out_off = 0, cells = 0;
        uint32_t max_k = 1;
        for (uint32_t i = 0; i < bq; i++) {
            const uint32_t q = qs[i0 + i];
            const uint64_t no = g->node_off[q], eo = g->edge_off[q];
            const uint32_t N = (uint32_t)(g->node_off[q + 1] - no), L = (uint32_t)(qoff[q + 1] - qoff[q]);
            const uint32_t *po = g->pred_off + no + q;
            const uint32_t E = po[N] - po[0];
            has_succ.assign(N, 0);
            for (uint32_t e = 0; e < E; e++) has_succ[g->pred[eo + po[0] + e]] = 1;
            snk.clear();
            for (uint32_t m = 0; m < N; m++)
                if (!has_succ[m]) snk.push_back(m);
            size_t *w = at.data() + 9 * (size_t)i;
            w[0] = pk.put(g->node_pos + no, N);
            w[1] = pk.put(po, (size_t)N + 1);
            w[2] = pk.put(g->pred + eo, (size_t)po[N]);  // (pred_off is relative to edge_off[q]: entries before po[0] included)
            w[3] = forbid ? pk.put(g->succ_minpos + no, N) : 0;
            w[4] = pk.put(snk.data(), snk.size());
            w[5] = profile ? 0 : pk.put(g->node_weight + no, N);
            w[6] = profile ? pk.put(g->node_score16 + 16 * no, 16 * (size_t)N) : 0;
            w[7] = profile ? 0 : pk.put(g->node_mask + no, N);
            w[8] = pk.put(qmask + qoff[q], L);
            WideQ &d = qd[i];
            d.N = N;
            d.L = L;
            d.by_s = L <= N ? 1u : 0u;
            d.K = d.by_s ? L : N;
            d.n_snk = (uint32_t)snk.size();
            d.pad_ = 0;
            d.plane_off = plane_off;
            d.out_off = out_off;
            plane_off += cells_of(q);
            out_off += L;
            cells += (uint64_t)N * L;
            max_k = std::max(max_k, d.K);
        }
        const size_t qd_at = pk.put(qd.data(), 0);  // (the descriptors go behind the arrays: their pointers need the block's address)
        const size_t in_bytes = qd_at + sizeof(WideQ) * bq;
        if (c->wide_in.reserve(in_bytes) || c->wide_planes.reserve_exact(4 * (size_t)n_planes * T) ||
            c->res.reserve(sizeof(WideRes) * bq) || c->out.reserve(sizeof(sina_hip_align_out) * bq) ||
            c->out_pos.reserve(4 * std::max<uint64_t>(out_off, 1)))
            return 1;
        const unsigned char *base = static_cast<const unsigned char *>(c->wide_in.p);
        for (uint32_t i = 0; i < bq; i++) {
            const size_t *w = at.data() + 9 * (size_t)i;
            WideQ &d = qd[i];
            d.pos = reinterpret_cast<const uint32_t *>(base + w[0]);
            d.pred_off = reinterpret_cast<const uint32_t *>(base + w[1]);
            d.pred = reinterpret_cast<const uint32_t *>(base + w[2]);
            d.succ_minpos = forbid ? reinterpret_cast<const uint32_t *>(base + w[3]) : nullptr;
            d.snk = reinterpret_cast<const uint32_t *>(base + w[4]);
            d.weight = profile ? nullptr : reinterpret_cast<const float *>(base + w[5]);
            d.prof16 = profile ? reinterpret_cast<const float *>(base + w[6]) : nullptr;
            d.mask = profile ? nullptr : base + w[7];
            d.qmask = base + w[8];
        }
        pk.bytes.resize(in_bytes);
        memcpy(pk.bytes.data() + qd_at, qd.data(), sizeof(WideQ) * bq);
        // (through the context's pinned staging: the block above is this loop's own and may go before the copy has run)
        if (upload(c, 7, c->wide_in.p, pk.bytes.data(), in_bytes, s)) return 1;

        WideArgs a;
        a.q = reinterpret_cast<const WideQ *>(base + qd_at);
        a.planes = c->wide_planes.as<uint32_t>();
        a.T = T;
        a.weights = weighted ? c->weights.as<float>() : nullptr;
        a.n_weights = weighted ? p->n_weights : 0;
        a.ms = -p->match_score;  // scoring_scheme_*(-match, -mismatch, gap, gapext), align.cpp:406-414
        a.mms = -p->mismatch_score;
        a.gp = p->gap_penalty;
        a.gpe = p->gap_ext_penalty;
        a.res = c->res.as<WideRes>();
        a.out = c->out.as<sina_hip_align_out>();
        a.out_pos = c->out_pos.as<uint32_t>();
        a.self16 = profile ? c->self16.as<float>() : nullptr;
        a.nq = bq;
        a.width = g->width;
        a.overhang = p->overhang;
        // a thread per cell of the launch's longest diagonal, whole waves, at most 1024
        const uint32_t threads = std::min<uint32_t>(1024u, (max_k + 63u) / 64u * 64u);
        SH_CHECK(hipEventRecord(c->ev[0], s));
        if (weighted && forbid) hipLaunchKernelGGL((mesh_wide_kernel<true, true>), dim3(bq), dim3(threads), 0, s, a);
        else if (weighted) hipLaunchKernelGGL((mesh_wide_kernel<true, false>), dim3(bq), dim3(threads), 0, s, a);
        else if (forbid) hipLaunchKernelGGL((mesh_wide_kernel<false, true>), dim3(bq), dim3(threads), 0, s, a);
        else hipLaunchKernelGGL((mesh_wide_kernel<false, false>), dim3(bq), dim3(threads), 0, s, a);
        SH_CHECK(hipGetLastError());
        SH_CHECK(hipEventRecord(c->ev[1], s));
        hipLaunchKernelGGL(mesh_wide_walk_kernel, dim3((bq + 63u) / 64u), dim3(64), 0, s, a);
        SH_CHECK(hipGetLastError());
        SH_CHECK(hipEventRecord(c->ev[2], s));
        if (download(c, 5, c->out.p, sizeof(sina_hip_align_out) * bq, s) || download(c, 6, c->out_pos.p, 4 * out_off, s)) return 1;
        SH_CHECK(wait_stream(c, s));
        const sina_hip_align_out *h_out = c->h_stage[5].as<sina_hip_align_out>();
        const uint32_t *h_pos = c->h_stage[6].as<uint32_t>();
        uint32_t *staged = c->h_out_pos.as<uint32_t>();
        for (uint32_t i = 0; i < bq; i++) {
            const uint32_t q = qs[i0 + i];
            out[q] = h_out[i];
            // (the staged columns are laid out like the caller's out_pos with qoff[0] taken as 0)
            memcpy(staged + (qoff[q] - qoff[0]), h_pos + qd[i].out_off, 4 * (size_t)qd[i].L);
            if (out_pos) memcpy(out_pos + qoff[q], h_pos + qd[i].out_off, 4 * (size_t)qd[i].L);
        }
        if (dbg_vm) {  // sina_hip_debug_mesh_wide: one query; the planes as the reference lays them out, [N * L]
            const WideQ &d = qd[0];
            const uint64_t nc = cells_of(qs[i0]);
            std::vector<uint32_t> pl(nc);
            for (int k = 0; k < 3; k++) {
                const int which = k == 0 ? kPlVm : (k == 1 ? kPlVs : kPlValue);
                uint32_t *dst = k == 0 ? dbg_vm : (k == 1 ? dbg_vs : reinterpret_cast<uint32_t *>(dbg_value));
                if (!dst) continue;
                SH_CHECK(hipMemcpy(pl.data(), c->wide_planes.as<uint32_t>() + (uint64_t)which * T + d.plane_off, 4 * nc, hipMemcpyDeviceToHost));
                for (uint32_t m = 0; m < d.N; m++)
                    for (uint32_t x = 0; x < d.L; x++)
                        dst[(size_t)m * d.L + x] = pl[((uint64_t)m + x) * d.K + (d.by_s ? x : m)];
            }
        }
        float dp_ms = 0, bt_ms = 0;
        SH_CHECK(hipEventElapsedTime(&dp_ms, c->ev[0], c->ev[1]));
        SH_CHECK(hipEventElapsedTime(&bt_ms, c->ev[1], c->ev[2]));
        c->path_queries[kPathWide] += bq;
        {
            std::lock_guard<std::mutex> slk(c->st->stats_mu);
            c->st->stats.dp_ms += dp_ms;
            c->st->stats.dp_busy_ms += dp_ms;
            c->st->stats.backtrack_ms += bt_ms;
            c->st->stats.dp_cells += cells;
            c->st->stats.dp_cells_swept += cells;
            c->st->stats.dp_launches++;
        }
        i0 = i1;
    }
    return 0;
}

}  // namespace sina_hip
