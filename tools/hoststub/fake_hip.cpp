// HOST-PROFILING STUB -- not part of the product, never shipped in sina_amd/, never loaded by tests or bench.py.
//
// A stand-in for libsina_hip.so that answers the C-ABI calls of the host stages (host/store.cpp, famfinder.cpp, aligner.cpp, search_filter.cpp) with
// plausible, deterministic, WRONG results in no time, so that the CPU cost of the host side of the boundary
// (trays, famfinder's cascade, the aligner's glue, the sink) can be measured per query in a container
// without a GPU (tools/hoststub/host_perf.py).  It computes nothing: k-mer "results" are hash-picked
// reference ids with descending scores, "alignments" put query base i in column 3 i.  Anything that checks
// results against the oracle must use the real library.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "sina_hip.h"

struct sina_hip_ctx {
    sina_hip_ctx *root;
    uint32_t n_refs = 0, width = 0;
    std::vector<uint32_t> staged;
};
static thread_local std::string g_err;

extern "C" {
int sina_hip_abi_version(void) { return SINA_HIP_ABI_VERSION; }
const char *sina_hip_last_error(void) { return g_err.c_str(); }
int sina_hip_last_error_is_limit(void) { return 0; }
int sina_hip_init(int, sina_hip_ctx **ctx) {
    *ctx = new sina_hip_ctx();
    (*ctx)->root = *ctx;
    return 0;
}
int sina_hip_fork(sina_hip_ctx *parent, sina_hip_ctx **ctx) {
    *ctx = new sina_hip_ctx();
    (*ctx)->root = parent->root;
    return 0;
}
int sina_hip_prewarm(sina_hip_ctx *, int) { return 0; }
void sina_hip_destroy(sina_hip_ctx *c) { delete c; }
int sina_hip_sync(sina_hip_ctx *) { return 0; }
int sina_hip_upload_refs(sina_hip_ctx *c, const uint32_t *, const uint64_t *, uint32_t n_refs, uint32_t width) {
    c->root->n_refs = n_refs;
    c->root->width = width;
    return 0;
}
int sina_hip_build_index(sina_hip_ctx *, unsigned, int) { return 0; }
int sina_hip_download_index(sina_hip_ctx *, uint32_t *, uint32_t *) { g_err = "stub"; return 1; }
int sina_hip_upload_index(sina_hip_ctx *, unsigned, int, const uint32_t *, const uint32_t *, uint64_t) { return 0; }
int sina_hip_store_view_get(sina_hip_ctx *, sina_hip_store_view *) { g_err = "stub"; return 1; }
int sina_hip_store_alloc_like(sina_hip_ctx *, sina_hip_store_view *) { g_err = "stub"; return 1; }
int sina_hip_kmer_topk(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t max,
                       uint32_t *out_ids, float *out_scores, uint32_t *out_n) {
    const uint32_t n = c->root->n_refs;
    if (max > n) max = n;
    for (uint32_t q = 0; q < nq; q++) {
        uint64_t h = 0x9E3779B97F4A7C15ull * (qoff[q + 1] - qoff[q] + 1);
        for (uint64_t x = qoff[q]; x < qoff[q] + 16 && x < qoff[q + 1]; x++) h = (h ^ qmask[x]) * 0x100000001b3ull;
        const uint32_t base = (uint32_t)(h % n);
        for (uint32_t x = 0; x < max; x++) {
            out_ids[(size_t)q * max + x] = (base + x * 97u) % n;  // (distinct while 97 x < n)
            // (below the query's own k-mer count -- about a quarter of its bases in "fast" mode -- as the scores of a real
            // search nearly always are: a member that carries EVERY k-mer of the query sends the aligner into its
            // exact-relative test, a string search per member)
            const int top = (int)((qoff[q + 1] - qoff[q]) / 6);
            out_scores[(size_t)q * max + x] = (float)std::max(1, top - (int)(x % 200));
        }
        out_n[q] = max;
    }
    return 0;
}
int sina_hip_kmer_scores(sina_hip_ctx *, const uint8_t *, uint32_t, int16_t *) { g_err = "stub"; return 1; }
int sina_hip_kmer_topk_any(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t max,
                           uint32_t *out_ids, float *out_scores, uint32_t *out_n) {
    return sina_hip_kmer_topk(c, qmask, qoff, nq, max, out_ids, out_scores, out_n);
}
int sina_hip_kmer_scores_any(sina_hip_ctx *, const uint8_t *, uint32_t, int16_t *) { g_err = "stub"; return 1; }
int sina_hip_long_queries(sina_hip_ctx *, uint64_t *n) { *n = 0; return 0; }
int sina_hip_big_select_queries(sina_hip_ctx *, uint64_t *n) { *n = 0; return 0; }
int sina_hip_wide_queries(sina_hip_ctx *, uint64_t *n) { *n = 0; return 0; }
int sina_hip_compare(sina_hip_ctx *, const uint32_t *, const uint64_t *, uint32_t, const uint32_t *, const uint64_t *,
                     int, int, sina_hip_match_counts *) { g_err = "stub"; return 1; }
int sina_hip_match_count(sina_hip_ctx *, const uint32_t *, const uint64_t *, uint32_t, const uint32_t *, const uint64_t *,
                          uint16_t *) { g_err = "stub"; return 1; }
// (every candidate "matches" in three quarters of the query's bases: below any usual --fs-msc-max)
int sina_hip_kmer_topk_match(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t max,
                             uint32_t *out_ids, float *out_scores, uint32_t *out_n, uint16_t *out_match) {
    const uint64_t b = q_off[0];
    std::vector<uint8_t> mask(q_off[nq] - b + 1);
    std::vector<uint64_t> rel(nq + 1);
    for (uint64_t i = b; i < q_off[nq]; i++) mask[i - b] = (uint8_t)(q_ab[i] >> 24);
    for (uint32_t q = 0; q <= nq; q++) rel[q] = q_off[q] - b;
    if (sina_hip_kmer_topk(c, mask.data(), rel.data(), nq, max, out_ids, out_scores, out_n)) return 1;
    if (max > c->root->n_refs) max = c->root->n_refs;
    for (uint32_t q = 0; q < nq; q++)
        for (uint32_t x = 0; x < max; x++) out_match[(size_t)q * max + x] = (uint16_t)((rel[q + 1] - rel[q]) * 3 / 4);
    return 0;
}
int sina_hip_match_stats(sina_hip_ctx *, double *ms, uint64_t *pairs, uint64_t *bases, uint64_t *launches) {
    *ms = 0;
    *pairs = *bases = *launches = 0;
    return 0;
}
int sina_hip_family_row_words(const sina_hip_family_rule *r, uint32_t *words) {
    *words = 2 + 2 * ((r->fs_min > r->fs_max ? r->fs_min : r->fs_max) + r->fs_req_full + 2 * r->fs_cover_gene);
    return 0;
}
int sina_hip_family_cascade(sina_hip_ctx *, const uint32_t *, const float *, const uint16_t *, const uint64_t *, const uint32_t *, uint32_t,
                            const sina_hip_family_rule *, const uint32_t *, const uint64_t *, uint32_t *) { g_err = "stub"; return 1; }
// (the "family" is the first fs_max of the hash-picked candidates, and that is always enough)
int sina_hip_kmer_topk_family(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t max,
                              const sina_hip_family_rule *r, const uint32_t *, const uint64_t *, uint32_t *out_rows) {
    if (max > c->root->n_refs) max = c->root->n_refs;
    std::vector<uint32_t> ids((size_t)nq * max + 1), n(nq + 1);
    std::vector<float> sc(ids.size());
    std::vector<uint16_t> mt(ids.size());
    if (sina_hip_kmer_topk_match(c, q_ab, q_off, nq, max, ids.data(), sc.data(), n.data(), mt.data())) return 1;
    uint32_t words = 0;
    sina_hip_family_row_words(r, &words);
    const uint32_t K = (words - 2) / 2;
    memset(out_rows, 0, 4 * (size_t)nq * words);
    for (uint32_t q = 0; q < nq; q++) {
        uint32_t *row = out_rows + (size_t)q * words;
        row[0] = std::min(std::min(n[q], r->fs_max), K);
        row[1] = 1u | (n[q] == 0 ? 2u : 0u);
        for (uint32_t x = 0; x < row[0]; x++) {
            row[2 + x] = ids[(size_t)q * max + x];
            memcpy(&row[2 + K + x], &sc[(size_t)q * max + x], 4);
        }
    }
    return 0;
}
int sina_hip_family_stats(sina_hip_ctx *, double *ms, uint64_t *queries, uint64_t *listed, uint64_t *scanned, uint64_t *launches) {
    *ms = 0;
    *queries = *listed = *scanned = *launches = 0;
    return 0;
}
int sina_hip_upload_name_order(sina_hip_ctx *, const uint32_t *, uint32_t) { return 0; }
int sina_hip_compare_rank(sina_hip_ctx *, const uint32_t *, const uint64_t *, uint32_t, const uint32_t *, const uint64_t *, int, int,
                          int, uint32_t, uint32_t *, float *, uint32_t *, uint32_t *) { g_err = "stub"; return 1; }
int sina_hip_kmer_topk_rank(sina_hip_ctx *, const uint32_t *, const uint64_t *, uint32_t, uint32_t, int, int, int, uint32_t,
                            uint32_t *, float *, uint32_t *, uint32_t *) { g_err = "stub"; return 1; }
int sina_hip_rank_stats(sina_hip_ctx *, double *ms, uint64_t *pairs, uint64_t *bases, uint64_t *launches) {
    *ms = 0;
    *pairs = *bases = *launches = 0;
    return 0;
}
// (a helix map is taken and forgotten; the stub counts no pairs)
int sina_hip_upload_pairs(sina_hip_ctx *, const uint32_t *, uint32_t) { return 0; }
int sina_hip_pair_counts(sina_hip_ctx *, const uint32_t *, const uint64_t *, uint32_t, uint32_t *) { g_err = "stub"; return 1; }
int sina_hip_pair_stats(sina_hip_ctx *, double *ms, uint64_t *seqs, uint64_t *entries, uint64_t *launches) {
    *ms = 0;
    *seqs = *entries = *launches = 0;
    return 0;
}
// (the switch is taken and nothing is counted: an align call of the stub leaves no rows)
int sina_hip_align_count_pairs(sina_hip_ctx *, int) { return 0; }
const uint32_t *sina_hip_staged_pair_counts(sina_hip_ctx *) { return nullptr; }
int sina_hip_pair_inplace_stats(sina_hip_ctx *, double *ms, uint64_t *seqs, uint64_t *launches) {
    *ms = 0;
    *seqs = *launches = 0;
    return 0;
}
// (likewise: the switch is taken, an align call of the stub scores no family)
int sina_hip_align_count_identity(sina_hip_ctx *, int) { return 0; }
const uint32_t *sina_hip_staged_identity(sina_hip_ctx *) { return nullptr; }
int sina_hip_show_dist(sina_hip_ctx *, const uint32_t *, const uint64_t *, const uint32_t *, const uint64_t *, uint32_t, const uint32_t *,
                       const uint64_t *, uint32_t *) { g_err = "stub"; return 1; }
int sina_hip_show_dist_stats(sina_hip_ctx *, double *ms, uint64_t *seqs, uint64_t *pairs, uint64_t *launches) {
    *ms = 0;
    *seqs = *pairs = *launches = 0;
    return 0;
}
// (the aligner's device-copy then keeps its host walk)
int sina_hip_find_bases(sina_hip_ctx *, const uint8_t *, const uint64_t *, uint32_t, const uint32_t *, const uint64_t *, uint32_t *) {
    g_err = "stub";
    return 1;
}
int sina_hip_find_bases_stats(sina_hip_ctx *, double *ms, uint64_t *pairs, uint64_t *bases, uint64_t *launches) {
    *ms = 0;
    *pairs = *bases = *launches = 0;
    return 0;
}
// (famfinder's device-turn then keeps its host route)
int sina_hip_kmer_topk_turn(sina_hip_ctx *, const uint8_t *, const uint64_t *, uint32_t, uint32_t, int, uint8_t *, float *, uint32_t *,
                            float *, uint32_t *) {
    g_err = "stub";
    return 1;
}
int sina_hip_turn_stats(sina_hip_ctx *, double *ms, uint64_t *queries, uint64_t *turned, uint64_t *launches) {
    *ms = 0;
    *queries = *turned = *launches = 0;
    return 0;
}
int sina_hip_identity_inplace_stats(sina_hip_ctx *, double *ms, uint64_t *seqs, uint64_t *pairs, uint64_t *launches) {
    *ms = 0;
    *seqs = *pairs = *launches = 0;
    return 0;
}
// (likewise: the switch is taken, an align call of the stub ranks nothing)
int sina_hip_align_rank(sina_hip_ctx *, int, unsigned, int, uint32_t, int, int, int, uint32_t) { return 0; }
const uint32_t *sina_hip_staged_rank(sina_hip_ctx *) { return nullptr; }
int sina_hip_rank_inplace_stats(sina_hip_ctx *, double *ms, uint64_t *seqs, uint64_t *pairs, uint64_t *launches) {
    *ms = 0;
    *seqs = *pairs = *launches = 0;
    return 0;
}
// (the stub assembles nothing: no shift log, nothing counted)
const uint32_t *sina_hip_staged_shift_log(sina_hip_ctx *) { return nullptr; }
int sina_hip_assemble_stats(sina_hip_ctx *, uint64_t *queries, uint64_t *assembled, uint64_t *shifted_queries, uint64_t *shifted_runs) {
    *queries = *assembled = *shifted_queries = *shifted_runs = 0;
    return 0;
}
int sina_hip_debug_assemble(sina_hip_ctx *, const sina_hip_align_params *, uint32_t, const uint8_t *, const uint64_t *, uint32_t,
                            sina_hip_align_out *, uint32_t *) { g_err = "stub"; return 1; }
int sina_hip_debug_assemble_ms(sina_hip_ctx *, double *ms) {
    *ms = 0;
    return 0;
}
void sina_hip_align_params_default(sina_hip_align_params *p) {
    memset(p, 0, sizeof(*p));
    p->match_score = 2;
    p->mismatch_score = -1;
    p->gap_penalty = 5;
    p->gap_ext_penalty = 2;
    p->fs_weight = 1;
}
const uint32_t *sina_hip_staged_out_pos(sina_hip_ctx *c) { return c->staged.data(); }
int sina_hip_align_families(sina_hip_ctx *c, const uint32_t *, const uint64_t *, uint32_t nq, const uint8_t *qmask,
                            const uint64_t *qoff, const sina_hip_align_params *, sina_hip_align_out *out, uint32_t *) {
    const uint64_t total = qoff[nq] - qoff[0];
    if (c->staged.size() < total) c->staged.resize(total + total / 4);
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t L = (uint32_t)(qoff[q + 1] - qoff[q]);
        uint32_t *pos = c->staged.data() + (qoff[q] - qoff[0]);
        const uint8_t *m = qmask + qoff[q];
        for (uint32_t i = 0; i < L; i++) pos[i] = (3u * i) | ((uint32_t)(m[i] & 0xf) << 24);
        sina_hip_align_out &o = out[q];
        memset(&o, 0, sizeof o);
        o.end_s = L - 1;
        o.raw = -1800.f;
        o.sum_weight = -2000.f;
        o.aligned_bases = (int32_t)L;
        o.n_out = L;
        o.assembled = 1;
    }
    return 0;
}
int sina_hip_align_families_wsets(sina_hip_ctx *c, const uint32_t *fam_ids, const uint64_t *fam_off, uint32_t nq, const uint8_t *qmask,
                                  const uint64_t *qoff, const sina_hip_align_params *p, const uint32_t *, uint32_t,
                                  sina_hip_align_out *out, uint32_t *out_pos) {
    return sina_hip_align_families(c, fam_ids, fam_off, nq, qmask, qoff, p, out, out_pos);
}
int sina_hip_align_graphs_wsets(sina_hip_ctx *, const sina_hip_graph_batch *, const uint8_t *, const uint64_t *,
                                const sina_hip_align_params *, const uint32_t *, uint32_t, sina_hip_align_out *, uint32_t *) {
    g_err = "stub";
    return 1;
}
int sina_hip_align_graphs(sina_hip_ctx *, const sina_hip_graph_batch *, const uint8_t *, const uint64_t *,
                          const sina_hip_align_params *, sina_hip_align_out *, uint32_t *) { g_err = "stub"; return 1; }
int sina_hip_align_graphs_any(sina_hip_ctx *, const sina_hip_graph_batch *, const uint8_t *, const uint64_t *,
                              const sina_hip_align_params *, sina_hip_align_out *, uint32_t *) { g_err = "stub"; return 1; }
int sina_hip_align_profiles(sina_hip_ctx *, const uint32_t *, const uint64_t *, uint32_t, const uint8_t *, const uint64_t *,
                            const sina_hip_align_params *, sina_hip_align_out *, uint32_t *) { g_err = "stub"; return 1; }
int sina_hip_get_stats(sina_hip_ctx *, sina_hip_stats *s) { memset(s, 0, sizeof *s); return 0; }
}
