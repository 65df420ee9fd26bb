// The helix base-pair score on the GPU: pair_count_kernel + sina_hip_upload_pairs,
// sina_hip_pair_counts, sina_hip_pair_stats over finished alignments a caller hands in; pair_count_assembled_kernel +
// sina_hip_align_count_pairs, sina_hip_staged_pair_counts, sina_hip_pair_inplace_stats over the alignments an align
// call has just assembled on the device (launched by dp_launch.hip, launch_inplace_counts; its switch, rows and event
// are the context's inplace[kInplacePairs], ctx.h).  The look-up and the classification are one piece of device code
// for both (pair_dev.h).  The kernels' counters are the context's use[kUsePairs] and use[kUsePairsInplace].
//
// What it computes: for every finished aligned sequence the counters behind align_bp_score_slv
// (cseq_base::calcPairScore, src/cseq.cpp:651-733): for every column i that the helix map pairs with a column p, the
// characters the sequence shows at i and at p -- a base, '-' where it has none, '.' for a word without mask bits --,
// the number of such visits that count (neither side '.', not both '-') and, of those, how many are the unordered
// pairs AG, AU, CG, GG, GU of upper-case unambiguous bases.  The weighted sum and the division stay with the host
// (host/cseq.cpp, pair_score_from_counts): six integers per sequence are all that crosses back.
//
// How it maps to the hardware: one wave per sequence, its lanes striding over the compacted map (pair_plan.h); a lane
// finds each of its two columns by a branch-free binary search over the sequence's packed words in global memory (6 KB
// for 16S: they stay in L1 / L2; every lane of the wave takes the same number of steps), classifies the pair and keeps
// six counters in registers; the wave adds them up across lanes and lane 0 stores the six words.  No LDS, no atomics.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "ctx.h"
#include "pair_dev.h"
#include "pair_plan.h"

namespace sina_hip {
namespace {

constexpr int kPT = 64 * (int)kPairWaves;  // threads per workgroup

struct PairArgs {
    const uint32_t *q_ab;   // the range's packed words
    const uint64_t *q_off;  // [n + 1], relative to q_ab
    const uint2 *ent;       // [n_ent] (column, partner)
    uint32_t *out;          // [n][6]: num, AG, AU, CG, GG, GU
    uint32_t n, n_ent;
};

__global__ void __launch_bounds__(kPT) pair_count_kernel(PairArgs a) {
    const uint32_t seq = blockIdx.x * kPairWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (seq >= a.n) return;  // (whole waves)
    const uint64_t b = a.q_off[seq];
    const uint32_t len = (uint32_t)(a.q_off[seq + 1] - b);
    const uint32_t *W = a.q_ab + b;
    pair_count_wave(W, len, a.ent, a.n_ent, lane, a.out + (size_t)seq * 6);
}

// The same count where the words already lie: behind assemble_kernel (traceback.hip) on its stream, over the words it
// left in BtArgs::out_pos -- no packing, no staging, no upload.  One wave per query of the DP launch range; a query
// the device did not finish (assembled == 0) or that failed (status != 0) gets six zeros, so every row is defined.
// There is no check of the columns here, as pair_first_descending is one for words a caller hands in: assembled == 1
// says that every insertion has been placed -- in its gap, or with assemble = 2 in the range its widening reached -- and
// every column is below the width (assemble_kernel, both instantiations: a widening that would place a base at the
// width leaves the query to the host), so the n_out words are the query's bases in strictly ascending columns -- what
// mask_at's search needs.
struct PairAsmArgs {
    const QDesc *qd;
    const sina_hip_align_out *out;
    const uint32_t *out_pos;
    const uint2 *ent;  // [n_ent] (column, partner)
    uint32_t *counts;  // [n][6]
    uint32_t n, n_ent;
};

__global__ void __launch_bounds__(kPT) pair_count_assembled_kernel(PairAsmArgs a) {
    const uint32_t q = blockIdx.x * kPairWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= a.n) return;  // (whole waves)
    const sina_hip_align_out *o = a.out + q;
    uint32_t *row = a.counts + (size_t)q * 6;
    if (o->status != 0 || o->assembled == 0) {  // (the same for every lane of the wave)
        if (lane < 6) row[lane] = 0;
        return;
    }
    pair_count_wave(a.out_pos + a.qd[q].q_off, o->n_out, a.ent, a.n_ent, lane, row);
}

}  // namespace

int launch_pair_count_assembled(const BtArgs &b, const void *ent, uint32_t n_ent, uint32_t *counts, hipStream_t s) {
    PairAsmArgs a;
    a.qd = b.qd;
    a.out = b.out;
    a.out_pos = b.out_pos;
    a.ent = static_cast<const uint2 *>(ent);
    a.counts = counts;
    a.n = b.nq;
    a.n_ent = n_ent;
    hipLaunchKernelGGL(pair_count_assembled_kernel, dim3(pair_grid(b.nq)), dim3(kPT), 0, s, a);
    SH_CHECK(hipGetLastError());
    return 0;
}

}  // namespace sina_hip

using namespace sina_hip;

extern "C" int sina_hip_upload_pairs(sina_hip_ctx *c, const uint32_t *pairs, uint32_t n) {
    if (!c || (!pairs && n != 0)) SH_FAIL("upload_pairs: null argument");
    if (!c->owns_store) SH_FAIL("upload_pairs: a forked context cannot change the reference store");
    std::lock_guard<std::mutex> lk(c->mu);
    const std::vector<uint32_t> ent = pair_compact(pairs, n);
    c->st->n_pair_ent = 0;
    if (ent.empty()) return 0;  // (an empty or all-zero map: no map)
    SH_CHECK(hipSetDevice(c->device));
    if (c->st->pair_ent.reserve(4 * ent.size())) return 1;
    SH_CHECK(hipMemcpy(c->st->pair_ent.p, ent.data(), 4 * ent.size(), hipMemcpyHostToDevice));
    c->st->n_pair_ent = (uint32_t)(ent.size() / 2);
    return 0;
}

extern "C" int sina_hip_pair_counts(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t *counts) {
    if (!c) SH_FAIL("pair_counts: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    sina_hip_hint_guard hints(c);
    const uint32_t n_ent = c->st->n_pair_ent;
    if (n_ent == 0) SH_FAIL("pair_counts: upload a helix map first");
    if (nq == 0) return 0;
    if (!q_ab || !q_off || !counts) SH_FAIL("pair_counts: null argument");
    for (uint32_t q = 0; q < nq; q++) {
        if (q_off[q + 1] < q_off[q]) SH_FAIL("pair_counts: sequence offsets descend");
        if (q_off[q + 1] - q_off[q] > 0x7FFFFFFFull) SH_FAIL("pair_counts: sequence longer than 2^31 - 1 words");
    }
    if (pair_first_descending(q_ab, q_off, nq) != nq) SH_FAIL("pair_counts: a sequence's columns descend");
    SH_CHECK(hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    // (SINA_HIP_TEST=pair_words=N: launch ranges of N words, so that a small call takes several)
    const std::string words_knob = test_knob("pair_words");
    const uint64_t max_words = words_knob.empty() ? kPairRangeWords : std::max<uint64_t>(1, strtoull(words_knob.c_str(), nullptr, 10));
    std::vector<uint64_t> rel;
    for (const PairRange &r : pair_ranges(q_off, nq, max_words)) {
        const uint32_t n = r.q1 - r.q0;
        const uint64_t words = q_off[r.q1] - q_off[r.q0];
        rel.resize((size_t)n + 1);
        for (uint32_t q = 0; q <= n; q++) rel[q] = q_off[r.q0 + q] - q_off[r.q0];
        if (c->s_qab.reserve(4 * std::max<uint64_t>(words, 1)) || c->s_qoff.reserve(8 * ((uint64_t)n + 1)) ||
            c->s_out.reserve(24 * (uint64_t)n))
            return 1;
        if (upload(c, 1, c->s_qab.p, q_ab + q_off[r.q0], 4 * words, s) || upload(c, 2, c->s_qoff.p, rel.data(), 8 * ((uint64_t)n + 1), s))
            return 1;
        PairArgs a;
        a.q_ab = c->s_qab.as<uint32_t>();
        a.q_off = c->s_qoff.as<uint64_t>();
        a.ent = c->st->pair_ent.as<uint2>();
        a.out = c->s_out.as<uint32_t>();
        a.n = n;
        a.n_ent = n_ent;
        // (a thin kernel beside whatever is resident: on the context's own stream, like the trace-back walk -- ctx.h)
        SH_CHECK(hipEventRecord(c->ev[6], s));
        hipLaunchKernelGGL(pair_count_kernel, dim3(pair_grid(n)), dim3(kPT), 0, s, a);
        SH_CHECK(hipGetLastError());
        SH_CHECK(hipEventRecord(c->ev[7], s));
        if (download(c, 5, c->s_out.p, 24 * (size_t)n, s)) return 1;
        SH_CHECK(wait_stream(c, s));
        float ms = 0;
        SH_CHECK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
        memcpy(counts + (size_t)r.q0 * 6, c->h_stage[5].p, 24 * (size_t)n);
        c->use[kUsePairs].add(ms, n, (uint64_t)n * n_ent, 1);
    }
    return 0;
}

extern "C" int sina_hip_pair_stats(sina_hip_ctx *c, double *kernel_ms, uint64_t *sequences, uint64_t *entries_visited, uint64_t *launches) {
    if (!c || !kernel_ms || !sequences || !entries_visited || !launches) SH_FAIL("pair_stats: null argument");
    return read_use(c, kUsePairs, kernel_ms, sequences, entries_visited, launches);
}

extern "C" int sina_hip_align_count_pairs(sina_hip_ctx *c, int on) {
    if (!c) SH_FAIL("align_count_pairs: null ctx");
    std::lock_guard<std::mutex> lk(c->mu);
    c->inplace[kInplacePairs].on = on != 0;
    return 0;
}

extern "C" const uint32_t *sina_hip_staged_pair_counts(sina_hip_ctx *c) {
    if (!c) {
        set_error("staged_pair_counts: null ctx");
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    return c->inplace[kInplacePairs].staged();
}

extern "C" int sina_hip_pair_inplace_stats(sina_hip_ctx *c, double *kernel_ms, uint64_t *sequences, uint64_t *launches) {
    if (!c || !kernel_ms || !sequences || !launches) SH_FAIL("pair_inplace_stats: null argument");
    return read_use(c, kUsePairsInplace, kernel_ms, sequences, nullptr, launches);
}
