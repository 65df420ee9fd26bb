// The orientation of --turn queries on the GPU: turn_orient_kernel and turn_pick_kernel with their
// launchers.  kmer_launch.hip drives them around the count and select kernels of a call with a turn request
// (sina_hip_kmer_topk_turn); their counters are the context's use[kUseTurn].
//
// turn_orient_kernel.  What it computes: for every query of the call (len mask bytes at src + roff[q]) its n tried
// variants, variant x in orientation o = order[x] at dst + n roff[q] + x len: byte i is the query's byte i, or byte
// len - 1 - i where o is reversed, complemented (base_iupac::complement: bits 1 <-> 8 and 2 <-> 4, the case bit kept)
// where o is complemented.  How it maps to the hardware: one workgroup per query; its threads take the aligned dwords
// of dst a variant touches, a dword per thread and step, consecutive threads consecutive dwords.  A dword's four
// source bytes lie in two aligned dwords of src (a query starts at any byte): both are loaded, shifted together as 64
// bits, byte-swapped for a reversed variant and complemented four bytes at a time in the register.  A dword all of
// whose bytes are the variant's is stored whole; the variant's first and last dword may hold a neighbour's bytes (the
// variant before or behind, the next query's) and are stored byte by byte, the variant's bytes only.  No LDS, no
// barrier, no atomics.  Loads beyond the source's words are clamped to its last word; the bytes they give belong to
// no variant.
//
// turn_pick_kernel.  What it computes: for every query of a launch range whose select is final, the top-1 score of
// each of its n variants' rows (entry 0, or 0 for an empty row) into the four scores by orientation (untried: 0), the
// pick -- over o = 0 .. 3 the first strictly largest score above 0, else 0 (src/famfinder.cpp:344-378) -- and the
// winner's row (max ids, max scores, its length) as row q of a compact range of bq rows.  How it maps: one wave per
// query, kTurnPickQueriesPerWg waves to a workgroup; every lane reads the n scores (uniform addresses: scalar loads),
// the lanes copy the row in steps of 64 entries.  Row q n + x lies at or behind row q, and a workgroup's writes would
// overtake another's reads: the compact rows are buffers of this unit's own (sina_hip_ctx::t_ids, t_scores, t_n).
#include "common.h"
#include "ctx.h"
#include "turn_plan.h"

namespace sina_hip {
namespace {

struct OrientArgs {
    const uint32_t *src;   // the call's mask bytes as aligned dwords ...
    uint64_t src_words;    // ... this many of them
    const uint64_t *roff;  // [nq + 1] the queries' offsets in bytes, from 0
    uint8_t *dst;          // the variants, n times the source's bytes
    uint32_t nq, n, order;  // order: orientation of variant x in bits 2x, 2x + 1 (turn_order_word)
};

// bytes a .. a + 3 of the source as one little-endian word (a >= -3; what lies outside the source is unspecified)
__device__ __forceinline__ uint32_t source4(const OrientArgs &a, long long at) {
    const long long w = at >> 2, last = (long long)a.src_words - 1;
    const long long w0 = w < 0 ? 0 : (w > last ? last : w), w1 = w + 1 < 0 ? 0 : (w + 1 > last ? last : w + 1);
    const uint64_t both = ((uint64_t)a.src[w1] << 32) | a.src[w0];
    return (uint32_t)(both >> (8 * (unsigned)(at & 3)));
}
// base_iupac::complement on four mask bytes at once
__device__ __forceinline__ uint32_t complement4(uint32_t v) {
    return ((v & 0x02020202u) << 1) | ((v & 0x04040404u) >> 1) | ((v & 0x01010101u) << 3) | ((v & 0x08080808u) >> 3) | (v & 0x10101010u);
}

__global__ void __launch_bounds__(kTurnOrientThreads) turn_orient_kernel(OrientArgs a) {
    const uint32_t q = blockIdx.x;
    if (q >= a.nq) return;
    const uint64_t s = a.roff[q], len = a.roff[q + 1] - s;
    if (len == 0) return;
    for (uint32_t x = 0; x < a.n; x++) {
        const uint32_t o = (a.order >> (2 * x)) & 3u;
        const uint64_t d = (uint64_t)a.n * s + (uint64_t)x * len;  // the variant's bytes: d .. d + len - 1 of dst
        const uint64_t w_first = d >> 2, w_last = (d + len - 1) >> 2;
        for (uint64_t w = w_first + threadIdx.x; w <= w_last; w += kTurnOrientThreads) {
            const long long i0 = (long long)(4 * w) - (long long)d;  // the variant's byte the dword starts with: -3 .. len - 1
            uint32_t v;
            if (o & 1) v = __builtin_bswap32(source4(a, (long long)s + (long long)len - 1 - i0 - 3));
            else v = source4(a, (long long)s + i0);
            if (o & 2) v = complement4(v);
            if (i0 >= 0 && i0 + 3 < (long long)len) {
                *reinterpret_cast<uint32_t *>(a.dst + 4 * w) = v;
            } else {  // the variant's head or tail: its own bytes only
                for (int j = 0; j < 4; j++)
                    if (i0 + j >= 0 && i0 + j < (long long)len) a.dst[4 * w + j] = (uint8_t)(v >> (8 * j));
            }
        }
    }
}

struct PickArgs {
    const uint32_t *ids;  // the range's select rows: [bq n][max] ...
    const float *scores;
    const uint32_t *n_in;  // ... and their lengths [bq n]
    uint32_t *out_ids;     // the winners' rows [bq][max] ...
    float *out_scores;
    uint32_t *out_n;       // ... their lengths [bq] ...
    uint32_t *meta;        // ... and [bq][5]: the orientation, the four scores' bits
    uint32_t bq, n, max;
};

__global__ void __launch_bounds__(kTurnPickThreads) turn_pick_kernel(PickArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * kTurnPickQueriesPerWg + (threadIdx.x >> 6);
    if (q >= a.bq) return;  // (the whole wave)
    // the four orientations' top-1 scores (untried: 0) and the pick, in registers: o is a constant of the unrolled loop
    float score[4];
    uint32_t best = 0, best_x = 0;
    float top = 0.f;
#pragma unroll
    for (uint32_t o = 0; o < 4; o++) {
        const uint32_t x = kTurnVariantOf[o];
        score[o] = 0.f;
        if (x < a.n) {
            const size_t row = (size_t)q * a.n + x;
            const uint32_t len = a.n_in[row];
            if (len != 0 && len != 0xFFFFFFFFu) score[o] = a.scores[row * a.max];
        }
        if (score[o] > top) {
            top = score[o];
            best = o;
            best_x = x;
        }
    }
    // (best is a tried orientation: an untried one scores 0 and never beats top; 0 is variant 0 of every call)
    const size_t from = ((size_t)q * a.n + best_x) * a.max, to = (size_t)q * a.max;
    for (uint32_t i = lane; i < a.max; i += 64) {
        a.out_ids[to + i] = a.ids[from + i];
        a.out_scores[to + i] = a.scores[from + i];
    }
    if (lane == 0) {
        a.out_n[q] = a.n_in[(size_t)q * a.n + best_x];
        uint32_t *m = a.meta + (size_t)q * 5;
        m[0] = best;
        for (uint32_t o = 0; o < 4; o++) m[1 + o] = __float_as_uint(score[o]);
    }
}

}  // namespace

int turn_orient_launch(sina_hip_ctx *c, const uint32_t *d_src, uint64_t n_bases, const uint64_t *d_roff, uint32_t nq, uint32_t n, uint8_t *d_dst,
                       hipStream_t s) {
    OrientArgs a;
    a.src = d_src;
    a.src_words = (n_bases + 3) / 4;
    a.roff = d_roff;
    a.dst = d_dst;
    a.nq = nq;
    a.n = n;
    a.order = turn_order_word(n);
    if (a.src_words == 0) return 0;  // (queries of no bases: no variant has a byte)
    hipLaunchKernelGGL(turn_orient_kernel, dim3(turn_orient_grid(nq)), dim3(kTurnOrientThreads), 0, s, a);
    SH_CHECK(hipGetLastError());
    return 0;
}

int turn_pick_launch(sina_hip_ctx *c, const uint32_t *d_ids, const float *d_scores, const uint32_t *d_n, uint32_t bq, uint32_t n, uint32_t max,
                     hipStream_t s) {
    if (c->t_ids.reserve((size_t)bq * max * 4) || c->t_scores.reserve((size_t)bq * max * 4) || c->t_n.reserve((size_t)bq * 4) ||
        c->t_meta.reserve((size_t)bq * 20))
        return 1;
    PickArgs a;
    a.ids = d_ids;
    a.scores = d_scores;
    a.n_in = d_n;
    a.out_ids = c->t_ids.as<uint32_t>();
    a.out_scores = c->t_scores.as<float>();
    a.out_n = c->t_n.as<uint32_t>();
    a.meta = c->t_meta.as<uint32_t>();
    a.bq = bq;
    a.n = n;
    a.max = max;
    hipLaunchKernelGGL(turn_pick_kernel, dim3(turn_pick_grid(bq)), dim3(kTurnPickThreads), 0, s, a);
    SH_CHECK(hipGetLastError());
    return 0;
}

}  // namespace sina_hip

using namespace sina_hip;

extern "C" int sina_hip_turn_stats(sina_hip_ctx *c, double *kernel_ms, uint64_t *queries, uint64_t *turned, uint64_t *launches) {
    if (!c || !kernel_ms || !queries || !turned || !launches) SH_FAIL("turn_stats: null argument");
    return read_use(c, kUseTurn, kernel_ms, queries, turned, launches);
}
