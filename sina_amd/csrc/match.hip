// Famfinder's identity filter on the GPU: match_count_kernel + sina_hip_match_count.
//
// What it computes: for every (query, candidate reference) pair the `match` counter of the lock-step walk behind
// --fs-msc-max (host/famfinder.cpp, identity_cover_query): the number of columns where both sequences have a base and
// (maskA & maskB & 0xF) != 0 -- base_comp_optimistic, no lower-case filter.  The walk's score is
// match / (match + mismatch + only_a + only_a_overhang), and that denominator is the query's base count whenever both
// sides have a base, so this one integer per pair is all the host needs.
//
// How it maps to the hardware: a workgroup keeps the query as a column -> 4-bit mask table in LDS (8 columns per
// 32-bit word, zero = no base), each of its waves streams one candidate at a time from HBM (coalesced 4-byte reads,
// every base read once; four loads in flight per lane) and pays one LDS read and one AND per base.  The count is kept
// as popcount(ballot) in a scalar.  The grid is (query, chunk of that query's candidates): match_plan.h.
// HBM-bound: algorithmic bytes = 4 B x sum of candidate lengths.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "ctx.h"
#include "match_plan.h"

namespace sina_hip {
namespace {

constexpr int kMT = 256;  // threads per workgroup

struct MatchArgs {
    const uint32_t *ref_ab;
    const uint64_t *ref_off;
    const uint32_t *q_ab;
    const uint64_t *q_off;
    const uint32_t *ids;  // [nq][stride]
    const uint32_t *n;    // [nq] candidates of the query; 0xFFFFFFFF (the candidate-list path's overflow mark) = 0
    uint16_t *out;        // [nq][stride]
    uint32_t width, n_refs, stride, chunk, chunks;
};

// LOADS: 4-byte loads a lane keeps in flight in the candidate loop's body (4; 1 is the variant tools/perf_msc.py times beside it)
template <int LOADS>
__global__ void __launch_bounds__(kMT) match_count_kernel(MatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tab[];  // [ceil(width / 8)] nibble per column
    const uint32_t q = blockIdx.x / a.chunks, ch = blockIdx.x % a.chunks, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t n = a.n[q];
    if (n == 0xFFFFFFFFu) n = 0;
    if (n > a.stride) n = a.stride;
    const uint32_t i0 = ch * a.chunk;
    if (i0 >= n) return;  // (the whole workgroup: nothing of this query falls into the chunk)
    const uint32_t i1 = min(n, i0 + a.chunk);

    const uint32_t nwords = (a.width + 7) / 8;
    for (uint32_t i = tid; i < nwords; i += kMT) tab[i] = 0;
    __syncthreads();
    const uint32_t *A = a.q_ab + a.q_off[q];
    const uint32_t la = (uint32_t)(a.q_off[q + 1] - a.q_off[q]);
    for (uint32_t i = tid; i < la; i += kMT) {
        const uint32_t ab = A[i], pos = ab & 0xFFFFFFu;
        if (pos >= a.width) continue;  // cannot meet a reference base
        atomicOr(&tab[pos >> 3], ((ab >> 24) & 0xFu) << ((pos & 7u) * 4u));
    }
    __syncthreads();

    auto hit = [&](uint32_t ab) -> bool {
        const uint32_t pos = ab & 0xFFFFFFu;
        if (pos >= a.width) return false;
        return ((tab[pos >> 3] >> ((pos & 7u) * 4u)) & (ab >> 24) & 0xFu) != 0;
    };
    const uint32_t *ids = a.ids + (size_t)q * a.stride;
    uint16_t *out = a.out + (size_t)q * a.stride;
    for (uint32_t c = i0 + wave; c < i1; c += kMT / 64) {
        const uint32_t id = ids[c];
        uint32_t cnt = 0;
        if (id < a.n_refs) {
            const uint32_t *B = a.ref_ab + a.ref_off[id];
            const uint32_t lb = (uint32_t)(a.ref_off[id + 1] - a.ref_off[id]);
            uint32_t base = 0;
            for (; LOADS == 4 && base + 256 <= lb; base += 256) {  // four loads in flight per lane
                const uint32_t b0 = B[base + lane], b1 = B[base + 64 + lane], b2 = B[base + 128 + lane], b3 = B[base + 192 + lane];
                cnt += __popcll(__ballot(hit(b0))) + __popcll(__ballot(hit(b1))) + __popcll(__ballot(hit(b2))) +
                       __popcll(__ballot(hit(b3)));
            }
            for (; base < lb; base += 64) {
                const uint32_t i = base + lane;
                const bool h = i < lb && hit(B[i]);
                cnt += __popcll(__ballot(h));
            }
        }
        if (lane == 0) out[c] = (uint16_t)cnt;
    }
}

}  // namespace

// nq queries (packed aligned bases d_qab at d_qoff[q], device memory) against the candidates d_ids[q * stride + i],
// i < d_n[q]: counts into d_out[q * stride + i].  Queued behind what the context's stream holds; returns when the
// kernel has ended.  h_ids / h_n: the same lists on the host, for the volume counters only (h_ids null: the ids stayed
// on the device, the candidates' bases are not counted).
int match_launch(sina_hip_ctx *c, const uint32_t *d_qab, const uint64_t *d_qoff, uint32_t nq, const uint32_t *d_ids,
                 const uint32_t *d_n, uint32_t stride, uint16_t *d_out, const uint32_t *h_ids, const uint32_t *h_n) {
    if (nq == 0 || stride == 0) return 0;
    const uint64_t lds = match_table_bytes(c->st->width);
    if (lds > kMatchMaxLds) SH_FAIL_LIMIT("match_counts: alignment too wide for the device match count");
    // (SINA_HIP_TEST=match_floor=N;match_loads=1: the alternatives DESIGN.md 3.4a quotes, tools/perf_msc.py variants)
    const std::string floor_knob = test_knob("match_floor");
    const uint32_t floor = floor_knob.empty() ? kMatchChunkFloor : std::max(1u, (uint32_t)strtoul(floor_knob.c_str(), nullptr, 10));
    const bool one_load = test_knob("match_loads") == "1";
    const MatchPlan pl = match_plan(nq, stride, (uint32_t)c->n_cu, floor);
    if (pl.chunk == 0) SH_FAIL("match_counts: too many queries for one launch");
    MatchArgs a;
    a.ref_ab = c->st->ref_ab.as<uint32_t>();
    a.ref_off = c->st->ref_off.as<uint64_t>();
    a.q_ab = d_qab;
    a.q_off = d_qoff;
    a.ids = d_ids;
    a.n = d_n;
    a.out = d_out;
    a.width = c->st->width;
    a.n_refs = c->st->n_refs;
    a.stride = stride;
    a.chunk = pl.chunk;
    a.chunks = pl.chunks;
    if (allow_full_lds(reinterpret_cast<const void *>(match_count_kernel<4>)) ||
        allow_full_lds(reinterpret_cast<const void *>(match_count_kernel<1>)))
        return 1;
    {
        heavy_launch hl(c, c->stream, kHeavyKmer);  // (a device-filling kernel: ctx.h)
        const hipStream_t hs = hl.stream();
        SH_CHECK(hipEventRecord(c->ev[6], hs));
        const dim3 grid((unsigned)((uint64_t)nq * pl.chunks));
        if (one_load) hipLaunchKernelGGL(match_count_kernel<1>, grid, dim3(kMT), (size_t)lds, hs, a);
        else hipLaunchKernelGGL(match_count_kernel<4>, grid, dim3(kMT), (size_t)lds, hs, a);
        SH_CHECK(hipGetLastError());
        SH_CHECK(hipEventRecord(c->ev[7], hs));
        if (hl.done()) return 1;
    }
    float ms = 0;
    SH_CHECK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
    uint64_t pairs = 0, bases = 0;
    const bool have_off = h_ids && ensure_ref_off_host(c) == 0;
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t n = h_n[q] == 0xFFFFFFFFu ? 0u : std::min(h_n[q], stride);
        pairs += n;
        if (have_off && h_ids)
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t id = h_ids[(size_t)q * stride + i];
                if (id < c->st->n_refs) bases += c->st->ref_off_host[id + 1] - c->st->ref_off_host[id];
            }
    }
    c->use[kUseMatch].add(ms, pairs, bases, 1);
    return 0;
}

// a call's queries: at most 65535 bases each, columns ascending strictly (offsets absolute into q_ab)
int match_check_queries(const char *who, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq) {
    for (uint32_t q = 0; q < nq; q++) {
        const uint64_t b = q_off[q], e = q_off[q + 1];
        if (e < b) SH_FAIL(std::string(who) + ": query offsets descend");
        if (e - b > 65535) SH_FAIL(std::string(who) + ": query longer than 65535 bases");
        for (uint64_t i = b + 1; i < e; i++)
            if ((q_ab[i] & 0xFFFFFFu) <= (q_ab[i - 1] & 0xFFFFFFu))
                SH_FAIL(std::string(who) + ": query columns do not ascend strictly");
    }
    return 0;
}

}  // namespace sina_hip

using namespace sina_hip;

extern "C" int sina_hip_match_count(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq,
                                     const uint32_t *cand_ids, const uint64_t *cand_off, uint16_t *out_match) {
    if (!c || !q_ab || !q_off || !cand_ids || !cand_off || !out_match) SH_FAIL("match_counts: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    sina_hip_hint_guard hints(c);
    if (!c->st->have_refs) SH_FAIL("match_counts: upload references first");
    if (nq == 0) return 0;
    if (cand_off[nq] < cand_off[0]) SH_FAIL("match_counts: candidate offsets descend");
    const uint64_t ncand = cand_off[nq] - cand_off[0];
    uint64_t max_n = 0;
    for (uint32_t q = 0; q < nq; q++) {
        if (cand_off[q + 1] < cand_off[q]) SH_FAIL("match_counts: candidate offsets descend");
        max_n = std::max<uint64_t>(max_n, cand_off[q + 1] - cand_off[q]);
    }
    if (max_n >= 0xFFFFFFFFull) SH_FAIL("match_counts: candidate list too long");
    for (uint64_t i = 0; i < ncand; i++)
        if (cand_ids[cand_off[0] + i] >= c->st->n_refs) SH_FAIL("match_counts: reference id out of range");
    if (match_check_queries("match_counts", q_ab, q_off, nq)) return 1;
    if (match_table_bytes(c->st->width) > kMatchMaxLds) SH_FAIL_LIMIT("match_counts: alignment too wide for the device match count");
    if (ncand == 0) return 0;
    SH_CHECK(hipSetDevice(c->device));
    // the lists as rows of one length (what the kernel addresses): ids padded with 0, n[q] the list's length
    const uint32_t stride = (uint32_t)max_n;
    const uint64_t nqa = q_off[nq] - q_off[0];
    std::vector<uint32_t> ids((size_t)nq * stride, 0u), n(nq);
    std::vector<uint64_t> qrel(nq + 1);
    for (uint32_t q = 0; q <= nq; q++) qrel[q] = q_off[q] - q_off[0];
    for (uint32_t q = 0; q < nq; q++) {
        n[q] = (uint32_t)(cand_off[q + 1] - cand_off[q]);
        memcpy(ids.data() + (size_t)q * stride, cand_ids + cand_off[q], 4 * (size_t)n[q]);
    }
    hipStream_t s = c->stream;
    if (c->s_qab.reserve(4 * std::max<uint64_t>(nqa, 1)) || c->s_qoff.reserve(8 * ((uint64_t)nq + 1)) ||
        c->s_cand.reserve(4 * ids.size()) || c->m_n.reserve(4 * (uint64_t)nq) || c->m_out.reserve(2 * ids.size()))
        return 1;
    if (upload(c, 1, c->s_qab.p, q_ab + q_off[0], 4 * nqa, s) || upload(c, 2, c->s_qoff.p, qrel.data(), 8 * ((uint64_t)nq + 1), s) ||
        upload(c, 3, c->s_cand.p, ids.data(), 4 * ids.size(), s) || upload(c, 4, c->m_n.p, n.data(), 4 * (uint64_t)nq, s))
        return 1;
    if (match_launch(c, c->s_qab.as<uint32_t>(), c->s_qoff.as<uint64_t>(), nq, c->s_cand.as<uint32_t>(), c->m_n.as<uint32_t>(), stride,
                     c->m_out.as<uint16_t>(), ids.data(), n.data()))
        return 1;
    if (download(c, 5, c->m_out.p, 2 * ids.size(), s)) return 1;
    SH_CHECK(wait_stream(c, s));
    const uint16_t *rows = static_cast<const uint16_t *>(c->h_stage[5].p);
    for (uint32_t q = 0; q < nq; q++) memcpy(out_match + cand_off[q], rows + (size_t)q * stride, 2 * (size_t)n[q]);
    return 0;
}

extern "C" int sina_hip_match_stats(sina_hip_ctx *c, double *kernel_ms, uint64_t *pairs, uint64_t *cand_bases, uint64_t *launches) {
    if (!c || !kernel_ms || !pairs || !cand_bases || !launches) SH_FAIL("match_stats: null argument");
    return read_use(c, kUseMatch, kernel_ms, pairs, cand_bases, launches);
}
