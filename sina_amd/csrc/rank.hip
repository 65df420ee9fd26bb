// Search-stage ranking on the GPU: rank_kernel, rank_merge_kernel + sina_hip_compare_rank,
// sina_hip_upload_name_order, sina_hip_rank_stats; sina_hip_kmer_topk_rank (kmer_launch.hip) launches the same kernels on the
// select's id rows.  And the same ranking riding on an align call: rank_assembled_kernel,
// rank_merge_assembled_kernel + sina_hip_align_rank, sina_hip_staged_rank, sina_hip_rank_inplace_stats, launched by
// dp_launch.hip (launch_inplace_counts) over the words the device assembly left.
//
// What it computes: what search_filter does with a query's candidates after comparing them (host/search_filter.cpp): the
// score (float)match / denom of every candidate, denom an integer chosen by the cover rule (cseq_comparator::score),
// and the max_result best by std::greater<result_item> -- score descending, equal scores by name descending.  With
// unique names and no NaN that is a strict total order, so the best N are one sequence whatever sorts them.  A score
// is never negative, so it orders like its bit pattern; a key is (score bits << 32 | rank of the name), compared as one
// 64-bit number.  A candidate with denom == 0 (the host's NaN) is left out and raises the query's flag: the caller
// ranks that query itself.
//
// How it maps to the hardware: the grid is (query, chunk of that query's candidates), rank_plan.h.  A workgroup builds
// the query's LDS tables as compare_kernel does (compare_dev.h); each wave streams one candidate at a time from HBM and
// reduces the six counters into every lane, so the whole wave knows the key and keeps its N best one per lane, in
// order: ballot for the position, shift, insert.  The four waves' lists are merged in LDS by counting, per key, the
// keys that beat it.  With one chunk per query the workgroup writes the final rows; else N keys go to a scratch row and
// rank_merge_kernel, one wave per query, folds the chunks.  HBM-bound like compare_kernel: 4 B x sum of candidate
// lengths in, at most N rows per query out.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "ctx.h"
#include "compare_dev.h"
#include "rank_plan.h"

namespace sina_hip {
namespace {

struct RankArgs {
    const uint32_t *ref_ab;
    const uint64_t *ref_off;
    const uint32_t *q_ab;
    const uint64_t *q_off;
    // a query's candidates: ids + cand_off (lists: ids[cand_off[q] .. cand_off[q + 1])), ids + row_n (rows:
    // ids[q * stride + i], i < row_n[q]; 0xFFFFFFFF, the select's overflow mark, = 0), or neither: every reference
    const uint32_t *ids;
    const uint64_t *cand_off;
    const uint32_t *row_n;
    const uint32_t *name_rank;  // [n_refs] position of the reference's name in ascending order
    const uint32_t *name_inv;   // [n_refs] its inverse
    uint64_t *keys;             // [nq][chunks][N] (chunks > 1)
    uint32_t *out_ids;          // [nq][N]
    uint32_t *out_scores;       // [nq][N] float bits
    uint32_t *out_n, *out_flag; // [nq]
    unsigned long long *cnt;    // [2] pairs scored, bases of their candidates
    uint32_t width, n_refs, stride, chunk, chunks, N;
    int iupac, filter_lc, cover;
};

// A stored key is the key plus one: 0 is the empty slot, and a candidate of score +0.0 whose name comes first (all
// bits zero) stays a key like any other.  (No key is all ones: a score is finite.)
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
// The wave's N best stored keys, descending, lane i holding place i (lanes >= N hold 0); k: the same stored key in
// every lane.  A key equal to one of the list goes behind it (a duplicated id: either order gives the same rows).
__device__ __forceinline__ void topn_insert(uint64_t &mine, uint64_t k, int lane, uint32_t N) {
    if (k <= shfl64(mine, (int)N - 1)) return;  // does not beat place N - 1 (0 while the list is not full)
    const int pos = __popcll(__ballot(lane < (int)N && mine >= k));
    const uint64_t up = shfl_up64(mine, 1);
    if (lane == pos) mine = k;
    else if (lane > pos) mine = up;
    if (lane >= (int)N) mine = 0;
}

__device__ __forceinline__ void write_row(const RankArgs &a, uint32_t q, uint32_t place, uint64_t stored) {
    const size_t at = (size_t)q * a.N + place;
    if (stored) {
        const uint64_t key = stored - 1;
        a.out_ids[at] = a.name_inv[(uint32_t)key];
        a.out_scores[at] = (uint32_t)(key >> 32);
    } else {
        a.out_ids[at] = 0;
        a.out_scores[at] = 0;
    }
}

// What a wave has after its share of a chunk: its N best stored keys (topn_insert), whether a candidate had
// denom == 0, and the volume it scored.  Every lane holds the same flags and counts.
struct WaveBest {
    uint64_t mine = 0;
    bool flagged = false;
    unsigned long long bases = 0;
    uint32_t pairs = 0;
};
// The per-candidate loop of both rank kernels: candidates i0 + wave, i0 + wave + 4 .. below i1 of the query whose
// tables are t, the id rows or lists at a.ids + c_base (no ids: every reference).
__device__ __forceinline__ void rank_candidates(const RankArgs &a, const QueryTables &t, uint64_t c_base, uint32_t i0, uint32_t i1,
                                                uint32_t lc_bit, int lane, int wave, WaveBest &wb) {
    for (uint32_t i = i0 + wave; i < i1; i += kCT / 64) {
        const uint32_t id = a.ids ? a.ids[c_base + i] : i;
        const bool valid = id < a.n_refs;
        const uint32_t *Bp = valid ? a.ref_ab + a.ref_off[id] : nullptr;
        const uint32_t lb = valid ? (uint32_t)(a.ref_off[id + 1] - a.ref_off[id]) : 0u;
        const sina_hip_match_counts m = classify_candidate(t, Bp, lb, valid, lc_bit, a.iupac, lane);
        if (!valid) continue;
        wb.pairs++;
        wb.bases += lb;
        const int32_t denom = cover_denominator(m, a.cover);  // (cseq_comparator::score: compare_dev.h)
        if (denom == 0) {  // the host's 0 / 0
            wb.flagged = true;
            continue;
        }
        const float score = __fdiv_rn((float)m.match, (float)denom);
        const uint64_t key = ((uint64_t)__float_as_uint(score) << 32) | a.name_rank[id];
        topn_insert(wb.mine, key + 1, lane, a.N);
    }
}
// The four waves' lists into one (s_keys: [kCT], all threads call): the place of this thread's key among them -- the
// number of keys that beat it, equal keys: the earlier slot first --, or N for a lane that holds no place of its list.
__device__ __forceinline__ uint32_t merged_place(uint64_t *s_keys, uint64_t mine, uint32_t tid, int lane, uint32_t N) {
    s_keys[tid] = mine;
    __syncthreads();
    if (lane >= (int)N) return N;
    uint32_t place = 0;
    for (int w = 0; w < kCT / 64; w++)
        for (uint32_t j = 0; j < N; j++) {
            const uint32_t slot = (uint32_t)w * 64 + j;
            const uint64_t o = s_keys[slot];
            place += (o > mine || (o == mine && slot < tid)) ? 1u : 0u;
        }
    return place;
}
// One wave folds the chunks' key rows of query q (rank_merge_kernel and its assembled twin): lane i ends with place i
__device__ __forceinline__ uint64_t merged_chunks(const RankArgs &a, uint32_t q, int lane) {
    const uint64_t *rows = a.keys + (size_t)q * a.chunks * a.N;
    const uint32_t total = a.chunks * a.N;
    uint64_t mine = 0;
    for (uint32_t base = 0; base < total; base += 64) {
        const uint64_t v = base + lane < total ? rows[base + lane] : 0;
        unsigned long long left = __ballot(v != 0);
        while (left) {
            const int j = __ffsll(left) - 1;
            left &= left - 1;
            topn_insert(mine, shfl64(v, j), lane, a.N);
        }
    }
    return mine;
}

__global__ void __launch_bounds__(kCT) rank_kernel(RankArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_tmp[8];
    __shared__ uint32_t s_scal[3];
    __shared__ uint32_t s_n;
    __shared__ uint64_t s_keys[kCT];
    const uint32_t q = blockIdx.x / a.chunks, ch = blockIdx.x % a.chunks, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    uint64_t c_base = 0;
    uint32_t n;
    if (a.cand_off) {
        c_base = a.cand_off[q];
        n = (uint32_t)(a.cand_off[q + 1] - c_base);
    } else if (a.row_n) {
        c_base = (uint64_t)q * a.stride;
        n = a.row_n[q];
        if (n == 0xFFFFFFFFu) n = 0;
        if (n > a.stride) n = a.stride;
    } else {
        n = a.n_refs;
    }
    const uint32_t i0 = ch * a.chunk;
    if (i0 >= n) {  // (the whole workgroup: nothing of this query falls into the chunk)
        if (a.chunks == 1) {
            if (tid < a.N) write_row(a, q, tid, 0);
            if (tid == 0) a.out_n[q] = 0;
        } else if (tid < a.N) {
            a.keys[((size_t)q * a.chunks + ch) * a.N + tid] = 0;
        }
        return;
    }
    const uint32_t i1 = a.chunk < n - i0 ? i0 + a.chunk : n;

    const uint32_t *A = a.q_ab + a.q_off[q];
    const uint32_t la = (uint32_t)(a.q_off[q + 1] - a.q_off[q]);
    const uint32_t lc_bit = a.filter_lc ? 0x10u : 0u;
    const QueryTables t = build_query_tables(smem, s_tmp, s_scal, A, la, a.width, lc_bit);
    if (tid == 0) s_n = 0;

    WaveBest wb;
    rank_candidates(a, t, c_base, i0, i1, lc_bit, lane, wave, wb);
    const uint64_t mine = wb.mine;
    const bool flagged = wb.flagged;
    const unsigned long long bases = wb.bases;
    const uint32_t pairs = wb.pairs;
    if (lane == 0) {
        if (flagged) atomicOr(&a.out_flag[q], 1u);
        if (pairs) {
            atomicAdd(&a.cnt[0], (unsigned long long)pairs);
            atomicAdd(&a.cnt[1], bases);
        }
    }

    // the four lists into one: a key's place is the number of keys that beat it (equal keys: the earlier slot first)
    {
        const uint32_t place = merged_place(s_keys, mine, tid, lane, a.N);
        if (place < a.N) {
            if (a.chunks == 1) {
                write_row(a, q, place, mine);
                if (mine) atomicAdd(&s_n, 1u);
            } else {
                a.keys[((size_t)q * a.chunks + ch) * a.N + place] = mine;
            }
        }
    }
    if (a.chunks == 1) {
        __syncthreads();
        if (tid == 0) a.out_n[q] = s_n;
    }
}

// one wave per query: the chunks' key rows into the final rows
__global__ void __launch_bounds__(64) rank_merge_kernel(RankArgs a) {
    const uint32_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const uint64_t mine = merged_chunks(a, q, lane);
    if (lane < (int)a.N) write_row(a, q, lane, mine);
    const uint32_t filled = __popcll(__ballot(lane < (int)a.N && mine != 0));
    if (lane == 0) a.out_n[q] = filled;
}

// ---- the same ranking where the device assembles: the query is what assemble_kernel has just left in
// the launch range's out_pos, its candidates the id rows the call's k-mer search left on the device.  r.ids / r.row_n
// point at the range's first row; r.q_ab, r.q_off, r.out_* and r.cnt are not used.
struct RankAssembledArgs {
    RankArgs r;
    const QDesc *qd;
    const sina_hip_align_out *out;
    const uint32_t *out_pos;
    uint32_t *rows;  // [n][kRankRowWords], zero before the launch: n, flags, 64 ids, 64 score bit patterns
    uint32_t max_l;  // longest query of the range: the tables' mask bytes
};
constexpr uint32_t kRowRanked = 2u, kRowNan = 1u;  // flag bits of a row's word 1

// Which queries of a range are ranked (the same for every thread of a workgroup): finished by the assembly -- a longer
// one than max_l never is, and would overrun the mask bytes -- and with every base of the input kept: the candidates
// come from the input's k-mers, the host searches with the aligned sequence's.
__device__ __forceinline__ bool ranked_here(const RankAssembledArgs &a, uint32_t q) {
    const sina_hip_align_out *o = a.out + q;
    return o->status == 0 && o->assembled != 0 && o->n_out <= a.max_l && o->n_out == a.qd[q].L;
}
__device__ __forceinline__ void write_assembled(uint32_t *row, const RankArgs &r, uint32_t place, uint64_t stored) {
    if (!stored) return;  // (the row was zero)
    const uint64_t key = stored - 1;
    row[2 + place] = r.name_inv[(uint32_t)key];
    row[2 + kRankMaxResult + place] = (uint32_t)(key >> 32);
}

__global__ void __launch_bounds__(kCT) rank_assembled_kernel(RankAssembledArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_tmp[8];
    __shared__ uint32_t s_scal[3];
    __shared__ uint32_t s_n;
    __shared__ uint64_t s_keys[kCT];
    const RankArgs &r = a.r;
    const uint32_t q = blockIdx.x / r.chunks, ch = blockIdx.x % r.chunks, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    if (!ranked_here(a, q)) return;  // (its row stays zero: not ranked)
    uint32_t *row = a.rows + (size_t)q * kRankRowWords;
    const uint64_t c_base = (uint64_t)q * r.stride;
    uint32_t n = r.row_n[q];
    if (n == 0xFFFFFFFFu) n = 0;
    if (n > r.stride) n = r.stride;
    const uint32_t i0 = ch * r.chunk;
    if (i0 >= n) {  // (the whole workgroup: nothing of this query falls into the chunk)
        if (r.chunks == 1) {
            if (tid == 0) atomicOr(&row[1], kRowRanked);  // ranked, no rows
        } else if (tid < r.N) {
            r.keys[((size_t)q * r.chunks + ch) * r.N + tid] = 0;
        }
        return;
    }
    const uint32_t i1 = r.chunk < n - i0 ? i0 + r.chunk : n;

    const uint32_t lc_bit = r.filter_lc ? 0x10u : 0u;
    const QueryTables t = build_query_tables(smem, s_tmp, s_scal, a.out_pos + a.qd[q].q_off, a.out[q].n_out, r.width, lc_bit);
    if (tid == 0) s_n = 0;

    WaveBest wb;
    rank_candidates(r, t, c_base, i0, i1, lc_bit, lane, wave, wb);
    if (lane == 0 && wb.flagged) atomicOr(&row[1], kRowNan);

    const uint32_t place = merged_place(s_keys, wb.mine, tid, lane, r.N);
    if (place < r.N) {
        if (r.chunks == 1) {
            write_assembled(row, r, place, wb.mine);
            if (wb.mine) atomicAdd(&s_n, 1u);
        } else {
            r.keys[((size_t)q * r.chunks + ch) * r.N + place] = wb.mine;
        }
    }
    if (r.chunks == 1) {
        __syncthreads();
        if (tid == 0) {
            row[0] = s_n;
            atomicOr(&row[1], kRowRanked);
        }
    }
}

// one wave per query: the chunks' key rows into the final row
__global__ void __launch_bounds__(64) rank_merge_assembled_kernel(RankAssembledArgs a) {
    const uint32_t q = blockIdx.x;
    const int lane = threadIdx.x;
    if (!ranked_here(a, q)) return;
    uint32_t *row = a.rows + (size_t)q * kRankRowWords;
    const uint64_t mine = merged_chunks(a.r, q, lane);
    if (lane < (int)a.r.N) write_assembled(row, a.r, lane, mine);
    const uint32_t filled = __popcll(__ballot(lane < (int)a.r.N && mine != 0));
    if (lane == 0) {
        row[0] = filled;
        atomicOr(&row[1], kRowRanked);
    }
}

// the grid of a launch range of bq queries with up to `stride` candidates each (SINA_HIP_TEST=rank_chunk=N applies)
RankPlan rank_assembled_plan(const sina_hip_ctx *c, uint32_t bq, uint32_t stride) {
    const std::string chunk_knob = test_knob("rank_chunk");
    const uint32_t forced = chunk_knob.empty() ? 0u : std::max(1u, (uint32_t)strtoul(chunk_knob.c_str(), nullptr, 10));
    return rank_plan(bq, stride, (uint32_t)c->n_cu, kRankChunkFloor, forced);
}

}  // namespace

static_assert(RankRider::row_bytes == 4 * (size_t)kRankRowWords, "ctx.h and rank_plan.h disagree on the row");

// (before the range's launches: it may allocate) the key scratch of a range with few queries
int reserve_rank_assembled(sina_hip_ctx *c, uint32_t bq) {
    if (!c->inplace[kInplaceRank].active || bq == 0) return 0;
    const RankPlan pl = rank_assembled_plan(c, bq, c->rider.stride);
    return c->r_keys.reserve(std::max<uint64_t>(rank_scratch_bytes(bq, pl, c->rider.N), 8));
}

int launch_rank_assembled(sina_hip_ctx *c, const BtArgs &b, uint32_t q_base, uint32_t max_l, uint32_t *rows, hipStream_t s) {
    if (b.nq == 0) return 0;
    const RankRider &rr = c->rider;
    const size_t lds = compare_table_bytes(b.width, max_l);
    if (lds > kCompareMaxLds) SH_FAIL_LIMIT("align_rank: alignment too wide for the device comparison");  // (align_call::begin_rank asked)
    const RankPlan pl = rank_assembled_plan(c, b.nq, rr.stride);
    if (pl.chunk == 0) SH_FAIL("align_rank: too many queries for one launch");
    if (c->r_keys.cap < rank_scratch_bytes(b.nq, pl, rr.N)) SH_FAIL("align_rank: key scratch not reserved");
    RankAssembledArgs a{};
    a.r.ref_ab = c->st->ref_ab.as<uint32_t>();
    a.r.ref_off = c->st->ref_off.as<uint64_t>();
    a.r.ids = rr.ids.as<uint32_t>() + (size_t)q_base * rr.stride;
    a.r.row_n = rr.n.as<uint32_t>() + q_base;
    a.r.name_rank = c->st->name_rank.as<uint32_t>();
    a.r.name_inv = c->st->name_inv.as<uint32_t>();
    a.r.keys = c->r_keys.as<uint64_t>();
    a.r.width = b.width;
    a.r.n_refs = c->st->n_refs;
    a.r.stride = rr.stride;
    a.r.chunk = pl.chunk;
    a.r.chunks = pl.chunks;
    a.r.N = rr.N;
    a.r.iupac = rr.iupac;
    a.r.filter_lc = rr.filter_lc;
    a.r.cover = rr.cover;
    a.qd = b.qd;
    a.out = b.out;
    a.out_pos = b.out_pos;
    a.rows = rows;
    a.max_l = max_l;
    if (allow_full_lds(reinterpret_cast<const void *>(rank_assembled_kernel))) return 1;
    SH_CHECK(hipMemsetAsync(rows, 0, RankRider::row_bytes * b.nq, s));
    hipLaunchKernelGGL(rank_assembled_kernel, dim3((unsigned)((uint64_t)b.nq * pl.chunks)), dim3(kCT), lds, s, a);
    SH_CHECK(hipGetLastError());
    if (pl.chunks > 1) {
        hipLaunchKernelGGL(rank_merge_assembled_kernel, dim3(b.nq), dim3(64), 0, s, a);
        SH_CHECK(hipGetLastError());
    }
    return 0;
}

// nq queries (packed aligned bases d_qab at d_qoff[q], device memory) against their candidates -- d_ids + d_coff
// (lists), d_ids + d_rown with `stride` (rows), or neither (every reference) --, at most M per query: the N best of each
// into out_ids / out_scores [nq * N] and out_n / out_flag [nq] (host memory).  Queued behind what the context's stream
// holds; returns when the results are on the host.
int rank_launch(sina_hip_ctx *c, const uint32_t *d_qab, const uint64_t *d_qoff, uint32_t nq, const uint32_t *d_ids,
                const uint64_t *d_coff, const uint32_t *d_rown, uint32_t stride, uint32_t M, uint32_t max_la, int iupac,
                int filter_lc, int cover, uint32_t N, uint32_t *out_ids, float *out_scores, uint32_t *out_n, uint32_t *out_flag) {
    if (nq == 0) return 0;
    if (M == 0) {
        memset(out_n, 0, 4 * (size_t)nq);
        memset(out_flag, 0, 4 * (size_t)nq);
        return 0;
    }
    const size_t lds = compare_table_bytes(c->st->width, max_la);
    if (lds > kCompareMaxLds) SH_FAIL_LIMIT("compare_rank: alignment too wide for the device comparison");
    // (SINA_HIP_TEST=rank_chunk=N: chunks of N candidates, so that a test can cut ten candidates into several)
    const std::string chunk_knob = test_knob("rank_chunk");
    const uint32_t forced = chunk_knob.empty() ? 0u : std::max(1u, (uint32_t)strtoul(chunk_knob.c_str(), nullptr, 10));
    const RankPlan pl = rank_plan(nq, M, (uint32_t)c->n_cu, kRankChunkFloor, forced);
    if (pl.chunk == 0) SH_FAIL("compare_rank: too many queries for one launch");
    hipStream_t s = c->stream;
    const size_t rows = (size_t)nq * N;
    if (c->r_ids.reserve(4 * rows) || c->r_scores.reserve(4 * rows) || c->r_n.reserve(4 * (size_t)nq) ||
        c->r_flag.reserve(4 * (size_t)nq) || c->r_cnt.reserve(16) ||
        c->r_keys.reserve(std::max<uint64_t>(rank_scratch_bytes(nq, pl, N), 8)))
        return 1;
    SH_CHECK(hipMemsetAsync(c->r_flag.p, 0, 4 * (size_t)nq, s));
    SH_CHECK(hipMemsetAsync(c->r_cnt.p, 0, 16, s));
    RankArgs a;
    a.ref_ab = c->st->ref_ab.as<uint32_t>();
    a.ref_off = c->st->ref_off.as<uint64_t>();
    a.q_ab = d_qab;
    a.q_off = d_qoff;
    a.ids = d_ids;
    a.cand_off = d_coff;
    a.row_n = d_rown;
    a.name_rank = c->st->name_rank.as<uint32_t>();
    a.name_inv = c->st->name_inv.as<uint32_t>();
    a.keys = c->r_keys.as<uint64_t>();
    a.out_ids = c->r_ids.as<uint32_t>();
    a.out_scores = c->r_scores.as<uint32_t>();
    a.out_n = c->r_n.as<uint32_t>();
    a.out_flag = c->r_flag.as<uint32_t>();
    a.cnt = c->r_cnt.as<unsigned long long>();
    a.width = c->st->width;
    a.n_refs = c->st->n_refs;
    a.stride = stride;
    a.chunk = pl.chunk;
    a.chunks = pl.chunks;
    a.N = N;
    a.iupac = iupac;
    a.filter_lc = filter_lc ? 1 : 0;
    a.cover = cover;
    if (allow_full_lds(reinterpret_cast<const void *>(rank_kernel))) return 1;
    {
        heavy_launch hl(c, s, kHeavyKmer);  // (a device-filling kernel: ctx.h)
        const hipStream_t hs = hl.stream();
        SH_CHECK(hipEventRecord(c->ev[6], hs));
        hipLaunchKernelGGL(rank_kernel, dim3((unsigned)((uint64_t)nq * pl.chunks)), dim3(kCT), lds, hs, a);
        SH_CHECK(hipGetLastError());
        if (pl.chunks > 1) {
            hipLaunchKernelGGL(rank_merge_kernel, dim3(nq), dim3(64), 0, hs, a);
            SH_CHECK(hipGetLastError());
        }
        SH_CHECK(hipEventRecord(c->ev[7], hs));
        if (hl.done()) return 1;
    }
    if (download(c, 9, c->r_ids.p, 4 * rows, s) || download(c, 10, c->r_scores.p, 4 * rows, s) ||
        download(c, 11, c->r_n.p, 4 * (size_t)nq, s) || download(c, 0, c->r_flag.p, 4 * (size_t)nq, s) ||
        download(c, 5, c->r_cnt.p, 16, s))
        return 1;
    SH_CHECK(wait_stream(c, s));
    memcpy(out_ids, c->h_stage[9].p, 4 * rows);
    memcpy(out_scores, c->h_stage[10].p, 4 * rows);
    memcpy(out_n, c->h_stage[11].p, 4 * (size_t)nq);
    memcpy(out_flag, c->h_stage[0].p, 4 * (size_t)nq);
    unsigned long long cnt[2];
    memcpy(cnt, c->h_stage[5].p, 16);
    float ms = 0;
    SH_CHECK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
    c->use[kUseRank].add(ms, cnt[0], cnt[1], pl.chunks > 1 ? 2 : 1);
    return 0;
}

// what both ranking entries refuse before anything runs
int rank_check_rules(const char *who, sina_hip_ctx *c, int iupac_rule, int cover_rule, uint32_t max_result) {
    if (iupac_rule < 0 || iupac_rule > 2) SH_FAIL(std::string(who) + ": unknown iupac rule");
    if (cover_rule < 0 || cover_rule > SINA_CMP_COVER_NOGAP) SH_FAIL(std::string(who) + ": unknown cover rule");
    if (max_result < 1 || max_result > kRankMaxResult) SH_FAIL(std::string(who) + ": max_result outside 1..64");
    if (!c->st->have_refs) SH_FAIL(std::string(who) + ": upload references first");
    if (!c->st->have_name_order) SH_FAIL(std::string(who) + ": upload the name order first");
    return 0;
}

}  // namespace sina_hip

using namespace sina_hip;

extern "C" int sina_hip_upload_name_order(sina_hip_ctx *c, const uint32_t *rank, uint32_t n) {
    if (!c || !rank) SH_FAIL("upload_name_order: null argument");
    if (!c->owns_store) SH_FAIL("upload_name_order: a forked context cannot change the reference store");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->st->have_refs) SH_FAIL("upload_name_order: upload references first");
    if (n != c->st->n_refs) SH_FAIL("upload_name_order: one rank per reference");
    std::vector<uint32_t> inv(n, 0xFFFFFFFFu);
    for (uint32_t id = 0; id < n; id++) {
        if (rank[id] >= n || inv[rank[id]] != 0xFFFFFFFFu) SH_FAIL("upload_name_order: not a permutation of 0..n_refs-1");
        inv[rank[id]] = id;
    }
    SH_CHECK(hipSetDevice(c->device));
    c->st->have_name_order = false;
    if (c->st->name_rank.reserve(4 * std::max<size_t>(n, 1)) || c->st->name_inv.reserve(4 * std::max<size_t>(n, 1))) return 1;
    SH_CHECK(hipMemcpy(c->st->name_rank.p, rank, 4 * (size_t)n, hipMemcpyHostToDevice));
    SH_CHECK(hipMemcpy(c->st->name_inv.p, inv.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
    c->st->have_name_order = true;
    return 0;
}

extern "C" int sina_hip_compare_rank(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq,
                                      const uint32_t *cand_ids, const uint64_t *cand_off, int iupac_rule, int filter_lowercase,
                                      int cover_rule, uint32_t max_result, uint32_t *out_ids, float *out_scores, uint32_t *out_n,
                                      uint32_t *out_flag) {
    if (!c || !q_ab || !q_off || !out_ids || !out_scores || !out_n || !out_flag) SH_FAIL("compare_rank: null argument");
    if (cand_ids && !cand_off) SH_FAIL("compare_rank: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    sina_hip_hint_guard hints(c);
    if (rank_check_rules("compare_rank", c, iupac_rule, cover_rule, max_result)) return 1;
    if (nq == 0) return 0;
    uint64_t ncand = 0, max_n = c->st->n_refs;
    if (cand_ids) {
        max_n = 0;
        for (uint32_t q = 0; q < nq; q++) {
            if (cand_off[q + 1] < cand_off[q]) SH_FAIL("compare_rank: candidate offsets descend");
            max_n = std::max<uint64_t>(max_n, cand_off[q + 1] - cand_off[q]);
        }
        if (max_n >= 0xFFFFFFFFull) SH_FAIL("compare_rank: candidate list too long");
        ncand = cand_off[nq] - cand_off[0];
        for (uint64_t i = 0; i < ncand; i++)
            if (cand_ids[cand_off[0] + i] >= c->st->n_refs) SH_FAIL("compare_rank: reference id out of range");
    }
    if (match_check_queries("compare_rank", q_ab, q_off, nq)) return 1;
    uint32_t max_la = 0;
    std::vector<uint64_t> qrel(nq + 1), crel(cand_ids ? nq + 1 : 0);
    for (uint32_t q = 0; q <= nq; q++) {
        qrel[q] = q_off[q] - q_off[0];
        if (cand_ids) crel[q] = cand_off[q] - cand_off[0];
        if (q < nq) max_la = std::max<uint32_t>(max_la, (uint32_t)(q_off[q + 1] - q_off[q]));
    }
    if (compare_table_bytes(c->st->width, max_la) > kCompareMaxLds)
        SH_FAIL_LIMIT("compare_rank: alignment too wide for the device comparison");
    SH_CHECK(hipSetDevice(c->device));
    const uint64_t nqa = qrel[nq];
    hipStream_t s = c->stream;
    if (c->s_qab.reserve(4 * std::max<uint64_t>(nqa, 1)) || c->s_qoff.reserve(8 * ((uint64_t)nq + 1))) return 1;
    if (upload(c, 1, c->s_qab.p, q_ab + q_off[0], 4 * nqa, s) || upload(c, 2, c->s_qoff.p, qrel.data(), 8 * ((uint64_t)nq + 1), s))
        return 1;
    if (cand_ids) {
        if (c->s_cand.reserve(4 * std::max<uint64_t>(ncand, 1)) || c->s_coff.reserve(8 * ((uint64_t)nq + 1))) return 1;
        if (upload(c, 3, c->s_cand.p, cand_ids + cand_off[0], 4 * ncand, s) ||
            upload(c, 4, c->s_coff.p, crel.data(), 8 * ((uint64_t)nq + 1), s))
            return 1;
    }
    // (results through vectors of the call's own: the outputs stay untouched if the launch fails)
    std::vector<uint32_t> ids((size_t)nq * max_result), n(nq), flag(nq);
    std::vector<float> sc((size_t)nq * max_result);
    if (rank_launch(c, c->s_qab.as<uint32_t>(), c->s_qoff.as<uint64_t>(), nq, cand_ids ? c->s_cand.as<uint32_t>() : nullptr,
                    cand_ids ? c->s_coff.as<uint64_t>() : nullptr, nullptr, 0, (uint32_t)max_n, max_la, iupac_rule, filter_lowercase,
                    cover_rule, max_result, ids.data(), sc.data(), n.data(), flag.data()))
        return 1;
    memcpy(out_ids, ids.data(), 4 * ids.size());
    memcpy(out_scores, sc.data(), 4 * sc.size());
    memcpy(out_n, n.data(), 4 * (size_t)nq);
    memcpy(out_flag, flag.data(), 4 * (size_t)nq);
    return 0;
}

extern "C" int sina_hip_rank_stats(sina_hip_ctx *c, double *kernel_ms, uint64_t *pairs, uint64_t *cand_bases, uint64_t *launches) {
    if (!c || !kernel_ms || !pairs || !cand_bases || !launches) SH_FAIL("rank_stats: null argument");
    return read_use(c, kUseRank, kernel_ms, pairs, cand_bases, launches);
}

// ---- the ranking that rides on an align call (rank_assembled_kernel): its switch, rows and counters
extern "C" int sina_hip_align_rank(sina_hip_ctx *c, int on, unsigned k, int nofast, uint32_t kmer_candidates, int iupac_rule,
                                    int filter_lowercase, int cover_rule, uint32_t max_result) {
    if (!c) SH_FAIL("align_rank: null ctx");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!on) {
        c->inplace[kInplaceRank].on = false;
        return 0;
    }
    // (the rules alone: what the store lacks never fails a call -- the align calls then run as without the switch)
    if (iupac_rule < 0 || iupac_rule > 2) SH_FAIL("align_rank: unknown iupac rule");
    if (cover_rule < 0 || cover_rule > SINA_CMP_COVER_NOGAP) SH_FAIL("align_rank: unknown cover rule");
    if (max_result < 1 || max_result > kRankMaxResult) SH_FAIL("align_rank: max_result outside 1..64");
    if (k < 1 || k > 12) SH_FAIL("align_rank: k must be in 1..12");
    if (kmer_candidates == 0) SH_FAIL("align_rank: kmer_candidates must be at least 1");
    if (kmer_big_select(c->st->have_refs ? std::min(kmer_candidates, std::max(c->st->n_refs, 1u)) : kmer_candidates))
        SH_FAIL_LIMIT("align_rank: more than 4096 candidates per query");
    RankRider &rr = c->rider;
    rr.k = k;
    rr.nofast = nofast ? 1u : 0u;
    rr.cands = kmer_candidates;
    rr.iupac = iupac_rule;
    rr.filter_lc = filter_lowercase ? 1 : 0;
    rr.cover = cover_rule;
    rr.N = max_result;
    c->inplace[kInplaceRank].on = true;
    return 0;
}

extern "C" const uint32_t *sina_hip_staged_rank(sina_hip_ctx *c) {
    if (!c) {
        set_error("staged_rank: null ctx");
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    return c->inplace[kInplaceRank].staged();
}

extern "C" int sina_hip_rank_inplace_stats(sina_hip_ctx *c, double *kernel_ms, uint64_t *sequences, uint64_t *pairs, uint64_t *launches) {
    if (!c || !kernel_ms || !sequences || !pairs || !launches) SH_FAIL("rank_inplace_stats: null argument");
    return read_use(c, kUseRankInplace, kernel_ms, sequences, pairs, launches);
}
