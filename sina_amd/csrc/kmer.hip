// K-mer reference search on gfx950: device index build, shared-k-mer counting,
// top-k selection.
//
// What it computes (reference src/kmer.h, src/idset.h, src/kmer_search.cpp:
// 152-276,366-420; spec in SURVEY.md Appendix A.1):
//   K(seq)  = k-mers over windows of k unambiguous bases ending at base index
//             e, k-1 <= e <= len-2 (the window ending on the last base is never
//             produced, kmer.h:188-201); "fast" keeps windows starting with A.
//   index   : reference r is in postings(v) iff v in set(K(r)); ids ascending.
//   score   = sum over K(query) WITH multiplicity of [r in postings(v)], int16.
//   top-k   : (score desc, id desc), i.e. std::greater<pair<int16,int>>.
//
// How it maps to the hardware: integer work on data that sits in L2 / Infinity Cache.
//   count : one 1024-thread workgroup per query.  Every query k-mer keeps a cursor into its
//           ascending posting list; the references are processed in tiles of 32768 whose int16
//           counters live in LDS (two per 32-bit word); a wave streams a list from its cursor with
//           2 x 1 KiB loads in flight into LDS atomics -- no search -- and the tile is written out
//           once.  Lists longer than 1/64 of the references are kept a second time as bitmaps and
//           counted bit-sliced in registers (carry-save adders, no atomics).
//   select: one workgroup per query: the cut score by an 8-way search on "how many scores are >= t"
//           (reductions over 16-byte loads; an LDS histogram serialises on the few low bins every
//           lane hits) -> ordered compaction (ties keep the LARGEST ids) -> bitonic sort of the
//           <= 4096 survivors.  More than 4096 wanted: the same cut search and ordered compaction leave the survivors
//           as 64-bit keys in a per-query segment in HBM, one segmented radix sort orders every segment of the
//           launch range, a small kernel unpacks the keys (kmer_select_big_kernel).
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstring>
#include <type_traits>

#include "common.h"
#include "ctx.h"
#include "kmer_plan.h"
#include "match_plan.h"
#include "compare_dev.h"
#include "rank_plan.h"

namespace sina_hip {
namespace {

constexpr int kCountThreads = 1024;
constexpr int kTileRefs = 32768;            // refs per LDS histogram tile (64 KiB)
constexpr int kWide = 2;                    // 1 KiB loads a wave of the count kernel keeps in flight
constexpr int kMaxQueryLen = (int)SINA_HIP_MAX_QUERY_LEN;  // k-mer list capacity in LDS: 64 KiB tile + 9 B per base <= 160 KiB
static_assert((size_t)kTileRefs * 2 + ((size_t)kMaxQueryLen + 63) / 64 * 64 * 9 + 64 <= 160 * 1024, "LDS of the count kernel");
// the long count kernel: a query of up to SINA_HIP_MAX_LONG_QUERY_LEN bases in chunks of
// kLongChunk windows, each chunk with the k-mer list capacity of the fast kernel -- and its k - 1 <= 11 bases before
// the chunk's first window end in qb[] (the 64 bytes more)
constexpr int kMaxLongQueryLen = (int)SINA_HIP_MAX_LONG_QUERY_LEN;
constexpr int kLongChunk = (int)SINA_HIP_KMER_LONG_CHUNK;
constexpr int kLongQbExtra = 64;
static_assert(kLongChunk <= kMaxQueryLen && kMaxLongQueryLen <= 32767, "a chunk fits the fast kernel's lists; int16 scores");
static_assert((size_t)kTileRefs * 2 + (size_t)kMaxQueryLen * 9 + 64 + kLongQbExtra <= 160 * 1024, "LDS of the long count kernel");
constexpr int kSelThreads = 256;
constexpr int kSelMax = (int)kKmerSelMax;      // candidates sortable in LDS

__device__ __forceinline__ bool ambig(uint32_t m) { return __popc(m & 0xfu) > 1; }

// k-mer ending at base e of a sequence of iupac masks (bases must be unambiguous
// and non-gap).  Returns false if the window is not a valid k-mer.
__device__ __forceinline__ bool kmer_at(const uint8_t *m, uint32_t len, uint32_t e, unsigned k, bool fast,
                                        uint32_t *out) {
    if (e + 1 < k || e + 2 > len) return false;  // need k bases and e <= len-2
    uint32_t v = 0;
    for (unsigned i = 0; i < k; i++) {
        const uint32_t b = m[e + 1 - k + i] & 0xfu;
        if (__popc(b) != 1) return false;
        v = (v << 2) | (uint32_t)(__ffs(b) - 1);
    }
    if (fast && (v >> (2 * (k - 1))) != 0) return false;  // prefix_filter(k, 1, BASE_A)
    *out = v;
    return true;
}

// ---------------------------------------------------------------- index build

// one (kmer << 32 | ref) key per valid window of every reference; invalid
// windows emit ~0 (sorted to the end, dropped).
__global__ void ref_kmer_keys(const uint32_t *ref_ab, const uint64_t *ref_off, uint32_t n_refs, unsigned k,
                              bool fast, uint64_t *keys) {
    const uint32_t r = blockIdx.x;
    const uint64_t b = ref_off[r], e = ref_off[r + 1];
    const uint32_t len = (uint32_t)(e - b);
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) {
        uint64_t key = ~0ull;
        if (i + 1 >= k && i + 2 <= len) {
            uint32_t v = 0;
            bool ok = true;
            for (unsigned x = 0; x < k; x++) {
                const uint32_t m = (ref_ab[b + i + 1 - k + x] >> 24) & 0xfu;
                if (__popc(m) != 1) {
                    ok = false;
                    break;
                }
                v = (v << 2) | (uint32_t)(__ffs(m) - 1);
            }
            if (ok && fast && (v >> (2 * (k - 1))) != 0) ok = false;
            if (ok) key = ((uint64_t)v << 32) | r;
        }
        keys[b + i] = key;
    }
}

// after sorting: flag first occurrence of each (kmer, ref) key
__global__ void mark_unique(const uint64_t *keys, uint64_t n, uint32_t *flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t kx = keys[i];
    flag[i] = (kx != ~0ull && (i == 0 || keys[i - 1] != kx)) ? 1u : 0u;
}

__global__ void scatter_unique(const uint64_t *keys, const uint32_t *flag, const uint32_t *pos, uint64_t n,
                               uint32_t *ids, uint32_t *counts) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const uint64_t kx = keys[i];
    ids[pos[i]] = (uint32_t)kx;
    atomicAdd(&counts[(uint32_t)(kx >> 32)], 1u);
}

// ---------------------------------------------------------------- count

struct CountArgs {
    const uint8_t *qmask;
    const uint64_t *qoff;
    const uint32_t *idx_off;
    const uint32_t *idx_ids;
    int16_t *scores;  // [nq][stride]
    uint32_t *nkq;    // [nq] number of query k-mers (upper bound of any score)
    unsigned long long *postings;
    uint32_t n_refs, stride, kmax;
    unsigned k;
    int fast;
    // dense posting lists as bitmaps (see ensure_dense): bitmap number per k-mer or kNoDense, words per bitmap
    const uint32_t *dense_id;
    const uint32_t *dense_bits;
    uint32_t dense_words;
    // CAND (kmer_count_kernel<true>): instead of the score row, the references that can still be among the top
    // `topm` -- keys (score + 32768) << 32 | id, at most cand_cap per query; cand_n[q] = how many there were
    unsigned long long *cand;
    uint32_t *cand_n;
    uint32_t cand_cap, topm;
};

constexpr uint32_t kNoDense = 0xFFFFFFFFu;
constexpr uint32_t kMaxDenseQ = 1023;  // dense k-mers of one query counted bit-sliced in 10 planes
static_assert(kTileRefs / 32 == kCountThreads, "one bitmap word of the tile per thread");

// ---- dense lists: which k-mers, and their bitmaps
__global__ void mark_dense(const uint32_t *idx_off, uint32_t n_kmers, uint32_t thresh, uint32_t *dense_id,
                           uint32_t *counter) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_kmers) return;
    const uint32_t len = idx_off[v + 1] - idx_off[v];
    dense_id[v] = (len > thresh) ? atomicAdd(counter, 1u) : kNoDense;
}
__global__ void fill_dense(const uint32_t *idx_off, const uint32_t *idx_ids, const uint32_t *dense_id,
                           uint32_t n_kmers, uint32_t *bits, uint32_t words) {
    // one wave per k-mer (most leave at once)
    const uint32_t v = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (v >= n_kmers) return;
    const uint32_t d = dense_id[v];
    if (d == kNoDense) return;
    uint32_t *b = bits + (size_t)d * words;
    for (uint32_t x = idx_off[v] + lane; x < idx_off[v + 1]; x += 64) {
        const uint32_t r = idx_ids[x];
        atomicOr(&b[r >> 5], 1u << (r & 31));
    }
}

// One workgroup (16 waves) per query.  Every query k-mer keeps a cursor into its (ascending)
// posting list; the reference range is processed in tiles of kTileRefs whose int16 counters
// live in LDS (two per 32-bit word).  For a tile, a wave takes a k-mer, streams postings from
// its cursor (kWide loads of 1 KiB in flight, four consecutive postings per lane), bumps the LDS
// counters of those below the tile end (a prefix, the lists being sorted) and advances the
// cursor: there is no search, and the tile is written out once.  (64 VGPRs: two workgroups per CU.)
// CAND: the score row never leaves the chip.  Top-M by (score desc, id desc) only needs the references whose score
// reaches the M-th largest score -- and tile 0 alone already holds M references that reach t0 = the M-th largest of
// its 1024 per-thread maxima (each maximum is the score of a different reference), so the final cut is t0 or more:
// every tile hands the references with score >= t0 (a few dozen per tile; ties included) to a candidate list, and
// kmer_select_cand_kernel sorts that list.  Saves the row's write and the select kernel's two passes over it
// (2 + 4 bytes per reference and query: at 500 000 references 3 MB per query, and the 2 GiB score matrix that cut
// a 9216-query search into five launches).  More candidates than the list holds (a giant group of equal scores):
// cand_n says so and the host repeats the launch with the score rows.
template <bool CAND>
__global__ void __launch_bounds__(kCountThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) kmer_count_kernel(CountArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t n_kmers, next_kmer, n_dense_q;
    __shared__ uint32_t c_cnt[8], c_ncand;
    __shared__ int c_t0;
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem);                 // [kTileRefs/2]
    uint32_t *cur = hist + kTileRefs / 2;                                // [kmax]
    uint32_t *end = cur + a.kmax;                                        // [kmax]
    uint8_t *qb = reinterpret_cast<uint8_t *>(end + a.kmax);             // [kmax] query masks
    // bitmap numbers of the query's dense k-mers: from the top of cur[] downwards (cursor slots grow
    // from the bottom; together they are at most kmax k-mers) -- a third array would cost the second
    // workgroup per CU
    uint32_t *dtop = cur + a.kmax - 1;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63;
    const uint8_t *qm = a.qmask + a.qoff[q];
    const uint32_t len = (uint32_t)(a.qoff[q + 1] - a.qoff[q]);
    if (tid == 0) {
        n_kmers = n_dense_q = 0;
        c_ncand = 0;
        c_t0 = 0;
    }
    for (uint32_t i = tid; i < len; i += kCountThreads) qb[i] = qm[i];
    __syncthreads();
    unsigned long long mine = 0;
    for (uint32_t e = tid; e < len; e += kCountThreads) {
        uint32_t v;
        if (kmer_at(qb, len, e, a.k, a.fast != 0, &v)) {
            const uint32_t lo = a.idx_off[v], hi = a.idx_off[v + 1];
            if (lo != hi) {
                // a k-mer of a conserved region is in a large share of the references: its list comes
                // as a bitmap and is counted without atomics (below); everything else by cursor
                const uint32_t did = a.dense_id ? a.dense_id[v] : kNoDense;
                uint32_t dslot = kMaxDenseQ;
                if (did != kNoDense) dslot = atomicAdd(&n_dense_q, 1u);
                if (dslot < kMaxDenseQ) {
                    *(dtop - dslot) = did;
                } else {
                    const uint32_t slot = atomicAdd(&n_kmers, 1u);
                    cur[slot] = lo;
                    end[slot] = hi;
                }
                mine += hi - lo;
            }
        }
    }
    __syncthreads();
    const uint32_t nk = n_kmers;
    const uint32_t nd = min(n_dense_q, kMaxDenseQ);
    const uint32_t ntiles = (a.n_refs + kTileRefs - 1) / kTileRefs;
    int16_t *row = a.scores + (size_t)q * a.stride;
    for (uint32_t t = 0; t < ntiles; t++) {
        const uint32_t tile_lo = t * kTileRefs;
        const uint32_t tile_hi = min(tile_lo + (uint32_t)kTileRefs, a.n_refs);
#include "kmer_count_tile.inc"
        if constexpr (!CAND) {
            // tile scores out: two int16 per 32-bit store (row stride is even)
            uint32_t *dst = reinterpret_cast<uint32_t *>(row + tile_lo);
            const uint32_t words = (tile_hi - tile_lo + 1) / 2;
            for (uint32_t i = tid; i < words; i += kCountThreads) dst[i] = hist[i];
            __syncthreads();
        } else {
            // my 32 references of the tile: words 16 tid .. 16 tid + 15, taken as they are read (pair g of lane l in
            // step (g - l) mod 8, a 64-bit access each: the lanes of a wave spread over the LDS banks) -- kept in an
            // array they would be indexed by the lane: sixteen selects per word
            const uint32_t my_lo = tile_lo + 32u * tid;
            if (t == 0) {
                // t0: the topm-th largest of the 1024 per-thread maxima (8-way search: seven ballots per pass)
                int mx = -1;
#pragma unroll
                for (int gg = 0; gg < 8; gg++) {
                    const int g = (gg + lane) & 7;
                    const uint2 wv = *reinterpret_cast<const uint2 *>(&hist[16 * tid + 2 * g]);
                    const uint32_t id0 = my_lo + 4u * (uint32_t)g;
                    if (id0 < a.n_refs) mx = max(mx, (int)(wv.x & 0xffffu));
                    if (id0 + 1 < a.n_refs) mx = max(mx, (int)(wv.x >> 16));
                    if (id0 + 2 < a.n_refs) mx = max(mx, (int)(wv.y & 0xffffu));
                    if (id0 + 3 < a.n_refs) mx = max(mx, (int)(wv.y >> 16));
                }
                // (no score exceeds the number of the query's k-mers with a posting: every one adds at most 1 to a reference)
                int lo = 0, hi = (int)(nk + nd) + 1;  // count(max >= lo) >= topm > count(max >= hi)
                for (int guard = 0; guard < 8 && hi - lo > 1; ++guard) {
                    if (tid < 8) c_cnt[tid] = 0;
                    __syncthreads();
                    int th[7];
#pragma unroll
                    for (int x = 0; x < 7; x++) {
                        const int tx = lo + (int)(((long long)(hi - lo) * (x + 1)) / 8);
                        th[x] = tx > lo ? tx : lo + 1;
                        const uint32_t c = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(mx >= th[x]));
                        if (lane == 0 && c) atomicAdd(&c_cnt[x], c);
                    }
                    __syncthreads();
                    int nlo = lo, nhi = hi;
                    bool hi_set = false;
#pragma unroll
                    for (int x = 0; x < 7; x++) {
                        if (th[x] >= hi) continue;
                        if (c_cnt[x] >= a.topm) nlo = th[x];
                        else if (!hi_set) {
                            nhi = th[x];
                            hi_set = true;
                        }
                    }
                    lo = nlo;
                    hi = nhi;
                    __syncthreads();
                }
                if (tid == 0) c_t0 = lo;
                __syncthreads();
            }
            const int t0 = c_t0;
#pragma unroll
            for (int gg = 0; gg < 8; gg++) {
                const int g = (gg + lane) & 7;
                const uint2 wv = *reinterpret_cast<const uint2 *>(&hist[16 * tid + 2 * g]);
                // (nearly always none of the four reaches t0: one comparison of the largest decides)
                const int v4[4] = {(int)(wv.x & 0xffffu), (int)(wv.x >> 16), (int)(wv.y & 0xffffu), (int)(wv.y >> 16)};
                if (max(max(v4[0], v4[1]), max(v4[2], v4[3])) < t0) continue;
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const uint32_t id = my_lo + 4u * (uint32_t)g + (uint32_t)h;
                    if (id < a.n_refs && v4[h] >= t0) {
                        const uint32_t slot = atomicAdd(&c_ncand, 1u);
                        if (slot < a.cand_cap)
                            a.cand[(size_t)q * a.cand_cap + slot] = ((unsigned long long)(uint32_t)(v4[h] + 32768) << 32) | id;
                    }
                }
            }
            __syncthreads();
        }
    }
    if constexpr (CAND) {
        if (tid == 0) a.cand_n[q] = c_ncand;
    }
    // postings visited = sum of the list lengths of the query's k-mers (each read once)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if (lane == 0 && mine) atomicAdd(a.postings, mine);
    if (tid == 0) a.nkq[q] = (uint32_t)((len > a.k) ? len - a.k : 0);
}

// Queries of more than kMaxQueryLen bases.  The scores are sums over the query's windows, so the windows are counted
// in chunks of kLongChunk (by the index of their last base: a window belongs to the chunk of that base and reads the up
// to k - 1 bases before the chunk with it, so an ambiguous base there invalidates it as anywhere).  Per chunk the
// cursor / bitmap lists are built anew in the LDS of a fast-kernel query of kMaxQueryLen bases, the tiles are counted
// as there, and the chunks after the first ADD their tile to the score row: a 32-bit add of two 16-bit counters --
// no total exceeds 32767, the low half never carries -- on a row that sits in L2.  Score rows only (no CAND).  (Its
// LDS leaves room for one workgroup per CU, four waves per SIMD: no cap at 64 VGPRs as the fast kernel has for its two.)
__global__ void __launch_bounds__(kCountThreads) kmer_count_long_kernel(CountArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t n_kmers, next_kmer, n_dense_q;
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem);                         // as in kmer_count_kernel, kmax = kMaxQueryLen
    uint32_t *cur = hist + kTileRefs / 2;
    uint32_t *end = cur + a.kmax;
    uint8_t *qb = reinterpret_cast<uint8_t *>(end + a.kmax);                     // [kmax + kLongQbExtra]
    uint32_t *dtop = cur + a.kmax - 1;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63;
    const uint8_t *qm = a.qmask + a.qoff[q];
    const uint32_t len = (uint32_t)(a.qoff[q + 1] - a.qoff[q]);
    const uint32_t ntiles = (a.n_refs + kTileRefs - 1) / kTileRefs;
    int16_t *row = a.scores + (size_t)q * a.stride;
    unsigned long long mine = 0;
    for (uint32_t e0 = 0; e0 < len; e0 += kLongChunk) {
        // windows ending on bases e0 .. e1 - 1; qb[] holds bases b0 .. e1 - 1
        const uint32_t e1 = min(len, e0 + (uint32_t)kLongChunk);
        const uint32_t b0 = e0 + 1 >= a.k ? e0 + 1 - a.k : 0u;
        if (tid == 0) n_kmers = n_dense_q = 0;  // (every thread has read the last chunk's: the tile loop synchronises)
        for (uint32_t i = b0 + tid; i < e1; i += kCountThreads) qb[i - b0] = qm[i];
        __syncthreads();
        for (uint32_t e = e0 + tid; e < e1; e += kCountThreads) {
            uint32_t v;
            // (len - b0, e - b0: the window on the query's last base is dropped, none at an inner chunk end)
            if (kmer_at(qb, len - b0, e - b0, a.k, a.fast != 0, &v)) {
                const uint32_t lo = a.idx_off[v], hi = a.idx_off[v + 1];
                if (lo != hi) {
                    const uint32_t did = a.dense_id ? a.dense_id[v] : kNoDense;
                    uint32_t dslot = kMaxDenseQ;
                    if (did != kNoDense) dslot = atomicAdd(&n_dense_q, 1u);
                    if (dslot < kMaxDenseQ) {
                        *(dtop - dslot) = did;
                    } else {
                        const uint32_t slot = atomicAdd(&n_kmers, 1u);
                        cur[slot] = lo;
                        end[slot] = hi;
                    }
                    mine += hi - lo;
                }
            }
        }
        __syncthreads();
        const uint32_t nk = n_kmers;
        const uint32_t nd = min(n_dense_q, kMaxDenseQ);
        for (uint32_t t = 0; t < ntiles; t++) {
            const uint32_t tile_lo = t * kTileRefs;
            const uint32_t tile_hi = min(tile_lo + (uint32_t)kTileRefs, a.n_refs);
#include "kmer_count_tile.inc"
            uint32_t *dst = reinterpret_cast<uint32_t *>(row + tile_lo);
            const uint32_t words = (tile_hi - tile_lo + 1) / 2;
            if (e0 == 0) {
                for (uint32_t i = tid; i < words; i += kCountThreads) dst[i] = hist[i];
            } else {
                for (uint32_t i = tid; i < words; i += kCountThreads) dst[i] += hist[i];
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if (lane == 0 && mine) atomicAdd(a.postings, mine);
    if (tid == 0) a.nkq[q] = (uint32_t)((len > a.k) ? len - a.k : 0);
}

// ---------------------------------------------------------------- select

struct SelectArgs {
    const int16_t *scores;  // [nq][stride]
    const uint32_t *nkq;    // [nq] upper bound of the scores of query q
    uint32_t *out_ids;      // [nq][max]
    float *out_scores;
    uint32_t *out_n;
    uint32_t n_refs, stride, max;
    unsigned long long *keys;  // kmer_select_big_kernel: [nq][max] survivors, unordered
};

__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *wsum, uint32_t *total) {
    // exclusive scan over the workgroup (kSelThreads), wave64 ballot-free version
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (int w = 0; w < kSelThreads / 64; w++) {
        if (w < wave) base += wsum[w];
        tot += wsum[w];
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

// Top-M of one query's score row, M = min(max, n_refs), order (score desc, id desc)
// (kmer_search.cpp:405-418 partial_sort on pair<score, id>).  The cut score is found by bisection
// on "how many scores are >= t" -- pure reductions over 16-byte vector loads of a row that sits in
// L2 (200 KB for 100k references), no atomics on a histogram whose low bins every lane hits --
// then one ordered pass emits everything above the cut plus the ties with the LARGEST ids.
// (kTopMax: the largest score a row can hold -- the fast count kernel's query length, or the long one's)
// BIG (kmer_select_big_kernel, M > kSelMax): the same cut, the same ordered pass -- the survivors, exactly M of them,
// go to the query's segment of a.keys instead of cand[] (which only serves the short cut's histogram then), a wave
// taking one run of slots per 64 vectors; sorting and unpacking are left to the launches behind the kernel.
template <int kTopMax, bool BIG>
__device__ __forceinline__ void kmer_select_body(const SelectArgs &a) {
    __shared__ unsigned long long cand[kSelMax];
    __shared__ uint32_t wsum[kSelThreads / 64];
    __shared__ uint32_t sh_slot;
    const uint32_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t n_refs = a.n_refs;
    const int16_t *sc = a.scores + (size_t)q * a.stride;  // stride % 8 == 0: rows are 16-byte aligned
    const uint4 *sc8 = reinterpret_cast<const uint4 *>(sc);
    const uint32_t nvec = (n_refs + 7) / 8;
    const uint32_t M = min(a.max, n_refs);
    const int top = (int)min(a.nkq[q], (uint32_t)kTopMax);  // no score can exceed the k-mer count

    // f(value, index) over the 8 scores of vector i; entries past n_refs are skipped
    auto for8 = [&](uint32_t i, auto &&f) {
        const uint4 v = sc8[i];
        const uint32_t wds[4] = {v.x, v.y, v.z, v.w};
        const uint32_t base = 8 * i;
        if (base + 8 <= n_refs) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                f((int)(int16_t)(wds[j] & 0xffffu), base + 2 * j);
                f((int)(int16_t)(wds[j] >> 16), base + 2 * j + 1);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (base + 2 * j < n_refs) f((int)(int16_t)(wds[j] & 0xffffu), base + 2 * j);
                if (base + 2 * j + 1 < n_refs) f((int)(int16_t)(wds[j] >> 16), base + 2 * j + 1);
            }
        }
    };
    auto block_sum = [&](uint32_t x) -> uint32_t {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        __syncthreads();  // wsum free again
        if ((tid & 63) == 0) wsum[tid >> 6] = x;
        __syncthreads();
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kSelThreads / 64; w++) t += wsum[w];
        return t;
    };
    // invariant: count(>= lo) >= M > count(>= hi).  Each pass over the row (it sits in L2) counts
    // against kWays - 1 thresholds at once: log_8 instead of log_2 passes.
    constexpr int kWays = 8;
    int lo = 0, hi = top + 1;
    uint32_t c_hi = 0;
    uint32_t n_ge_cut = 0;  // how many scores reach the cut, if the short cut below found it (else 0)
    // Long rows first try a short cut: a histogram of every 16th vector places a threshold T0 that
    // about 2 M + 128 scores of the whole row should reach -- few enough that a histogram of the
    // scores >= T0 over the WHOLE row has no hot bins (the bulk of a row is small scores, which is
    // what rules a plain LDS histogram out).  If at least M scores turn out to reach T0, the cut and
    // the number of scores above it come out of that histogram: two passes instead of four or five;
    // otherwise the search below starts from [0, T0).  The histogram borrows cand[] (unused so far).
    constexpr uint32_t kSample = 16;
    if (nvec >= 2048 && top < 2 * kSelMax) {  // (a query of more k-mers than bins: the general search below)
        uint32_t *hist = reinterpret_cast<uint32_t *>(cand);  // bins 0..top
        __shared__ int f_t;
        __shared__ uint32_t f_above, f_at;
        const uint32_t nb = (uint32_t)top + 1;
        // largest bin t whose suffix count (bins >= t) reaches `target`: f_t (-1: there is none),
        // f_above = count in the bins above t, f_at = count in bin t
        auto suffix_find = [&](uint32_t target) {
            const uint32_t chunk = (nb + kSelThreads - 1) / kSelThreads;
            const uint32_t rb = min(nb, (uint32_t)tid * chunk), re = min(nb, rb + chunk);  // reversed bin index
            uint32_t sum = 0;
            for (uint32_t r = rb; r < re; r++) sum += hist[nb - 1 - r];
            if (tid == 0) f_t = -1;
            uint32_t total;
            const uint32_t excl = block_excl_scan(sum, wsum, &total);  // (synchronises)
            if (excl < target && excl + sum >= target) {
                uint32_t run = excl;
                for (uint32_t r = rb; r < re; r++) {
                    const uint32_t h = hist[nb - 1 - r];
                    if (run + h >= target) {
                        f_t = (int)(nb - 1 - r);
                        f_above = run;
                        f_at = h;
                        break;
                    }
                    run += h;
                }
            }
            __syncthreads();
        };
        for (uint32_t i = tid; i < nb; i += kSelThreads) hist[i] = 0;
        __syncthreads();
        for (uint32_t i = (uint32_t)tid * kSample; i < nvec; i += kSelThreads * kSample)
            for8(i, [&](int v, uint32_t) {
                if (v > 0) atomicAdd(&hist[min(v, top)], 1u);
            });
        __syncthreads();
        const uint32_t target_s = 2 * M / kSample + 8;
        suffix_find(target_s);
        const int T0 = f_t;
        const bool usable = T0 >= 1 && f_above + f_at <= 8 * target_s;  // (not one giant group of equal scores)
        __syncthreads();
        if (usable) {
            for (uint32_t i = tid; i < nb; i += kSelThreads) hist[i] = 0;
            __syncthreads();
            for (uint32_t i = tid; i < nvec; i += kSelThreads)
                for8(i, [&](int v, uint32_t) {
                    if (v >= T0) atomicAdd(&hist[min(v, top)], 1u);
                });
            __syncthreads();
            suffix_find(M);
            if (f_t >= 0) {  // at least M scores reach T0: the cut is among them
                lo = f_t;
                hi = f_t + 1;
                c_hi = f_above;
                n_ge_cut = f_above + f_at;
            } else {  // fewer: count(>= T0) < M, the cut is below T0
                uint32_t part = 0;
                for (uint32_t i = tid; i < nb; i += kSelThreads) part += hist[i];
                hi = T0;
                c_hi = block_sum(part);
            }
            __syncthreads();
        }
    }
    for (int guard = 0; guard < 20 && hi - lo > 1; ++guard) {
        int th[kWays - 1];
        uint32_t c[kWays - 1];
#pragma unroll
        for (int x = 0; x < kWays - 1; x++) {
            // ascending thresholds strictly inside (lo, hi); duplicates at the top when the gap is small
            const int t = lo + (int)(((long long)(hi - lo) * (x + 1)) / kWays);
            th[x] = t > lo ? t : lo + 1;
            c[x] = 0;
        }
        for (uint32_t i = tid; i < nvec; i += kSelThreads)
            for8(i, [&](int v, uint32_t) {
#pragma unroll
                for (int x = 0; x < kWays - 1; x++) c[x] += (v >= th[x]) ? 1u : 0u;
            });
#pragma unroll
        for (int x = 0; x < kWays - 1; x++) c[x] = block_sum(c[x]);
        // the largest threshold that still has M scores at or above it becomes lo, the next one hi
        int nlo = lo, nhi = hi;
        uint32_t nc_hi = c_hi;
        bool hi_set = false;
#pragma unroll
        for (int x = 0; x < kWays - 1; x++) {
            if (th[x] >= hi) continue;
            if (c[x] >= M) {
                nlo = th[x];
            } else if (!hi_set) {
                nhi = th[x];
                nc_hi = c[x];
                hi_set = true;
            }
        }
        lo = nlo;
        hi = nhi;
        c_hi = nc_hi;
    }
    const int cut = lo;
    const uint32_t acc = c_hi;  // scores > cut: all taken

    // Few enough scores at or above the cut to sort them all: take every one of them -- the sort below
    // orders by (score, id) descending, so the first M are the ones above the cut plus the ties with
    // the LARGEST ids -- in one unordered pass.
    const bool take_all = !BIG && n_ge_cut != 0 && n_ge_cut <= (uint32_t)kSelMax;
    if (take_all) {
        __syncthreads();
        if (tid == 0) sh_slot = 0;
        __syncthreads();
        for (uint32_t i = tid; i < nvec; i += kSelThreads)
            for8(i, [&](int v, uint32_t id) {
                if (v >= cut) {
                    const uint32_t slot = atomicAdd(&sh_slot, 1u);
                    cand[slot] = ((unsigned long long)(uint32_t)(v + 32768) << 32) | id;
                }
            });
    } else {
    // Ordered pass: which ties (score == cut) to take -- those with the largest ids.  A wave owns
    // a contiguous range of vectors and reads it 64 vectors (1 KiB, coalesced) at a time; the rank
    // of a tie in id order is (ties in earlier waves) + (earlier iterations) + (lower lanes).
    constexpr int kSelWaves = kSelThreads / 64;
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t vw = ((nvec + kSelWaves - 1) / kSelWaves + 63) / 64 * 64;  // vectors per wave
    const uint32_t w0 = min(nvec, (uint32_t)wave * vw), w1 = min(nvec, w0 + vw);
    uint32_t my_eq = 0;
    for (uint32_t i = w0 + lane; i < w1; i += 64) for8(i, [&](int v, uint32_t) { my_eq += (v == cut) ? 1u : 0u; });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) my_eq += __shfl_xor(my_eq, off);  // ties in my wave's range
    __syncthreads();
    if (lane == 0) wsum[wave] = my_eq;
    if (tid == 0) sh_slot = 0;
    __syncthreads();
    uint32_t tot_eq = 0, run = 0;  // run: ties before the vectors of this iteration
    for (int w = 0; w < kSelWaves; w++) {
        if (w < wave) run += wsum[w];
        tot_eq += wsum[w];
    }
    const uint32_t skip_eq = tot_eq - (M - acc);  // ties to skip: the smallest ids
    for (uint32_t i0 = w0; i0 < w1; i0 += 64) {
        const uint32_t i = i0 + lane;
        uint32_t c = 0;
        if (i < w1) for8(i, [&](int v, uint32_t) { c += (v == cut) ? 1u : 0u; });
        uint32_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(incl, off);
            if (lane >= off) incl += y;
        }
        uint32_t eq_rank = run + incl - c;
        run += __shfl(incl, 63);
        if constexpr (BIG) {
            // how many this lane's vector gives -> its run of slots in the segment: one atomic per wave and iteration
            uint32_t mine = 0, er = eq_rank;
            if (i < w1)
                for8(i, [&](int v, uint32_t) {
                    bool take = v > cut;
                    if (v == cut) take = er++ >= skip_eq;
                    mine += take ? 1u : 0u;
                });
            uint32_t tin = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t y = __shfl_up(tin, off);
                if (lane >= off) tin += y;
            }
            const uint32_t wave_n = __shfl(tin, 63);
            uint32_t base = 0;
            if (lane == 0 && wave_n) base = atomicAdd(&sh_slot, wave_n);
            uint32_t slot = __shfl(base, 0) + tin - mine;
            unsigned long long *seg = a.keys + (size_t)q * M;
            if (i < w1 && mine)
                for8(i, [&](int v, uint32_t id) {
                    bool take = v > cut;
                    if (v == cut) take = eq_rank++ >= skip_eq;
                    if (take) {
                        if (slot < M) seg[slot] = ((unsigned long long)(uint32_t)(v + 32768) << 32) | id;
                        slot++;
                    }
                });
            continue;
        }
        if (i < w1)
            for8(i, [&](int v, uint32_t id) {
                bool take = v > cut;
                if (v == cut) {
                    take = eq_rank >= skip_eq;
                    eq_rank++;
                }
                if (take) {
                    const uint32_t slot = atomicAdd(&sh_slot, 1u);
                    // sort key: score (biased) high, id low -> descending order = (score desc, id desc)
                    if (slot < kSelMax) cand[slot] = ((unsigned long long)(uint32_t)(v + 32768) << 32) | id;
                }
            });
    }
    }
    if constexpr (BIG) return;  // (sorted and unpacked behind the kernel; the unpack kernel writes out_n)
    __syncthreads();
    const uint32_t out_base = sh_slot;
    const uint32_t n = min(out_base, (uint32_t)kSelMax);
    uint32_t P = 1;
    while (P < n) P <<= 1;
    for (uint32_t i = n + threadIdx.x; i < P; i += kSelThreads) cand[i] = 0ull;
    __syncthreads();
    // bitonic sort, descending
    for (uint32_t k2 = 2; k2 <= P; k2 <<= 1) {
        for (uint32_t j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (uint32_t i = threadIdx.x; i < P; i += kSelThreads) {
                const uint32_t ixj = i ^ j2;
                if (ixj > i) {
                    const unsigned long long x = cand[i], y = cand[ixj];
                    const bool desc = ((i & k2) == 0);
                    if (desc ? (x < y) : (x > y)) {
                        cand[i] = y;
                        cand[ixj] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < M; i += kSelThreads) {
        if (i < n) {
            const unsigned long long c = cand[i];
            a.out_ids[(size_t)q * a.max + i] = (uint32_t)c;
            a.out_scores[(size_t)q * a.max + i] = (float)((int)(uint32_t)(c >> 32) - 32768);
        }
    }
    if (threadIdx.x == 0) a.out_n[q] = n < M ? n : M;
}
template <int kTopMax>
__global__ void __launch_bounds__(kSelThreads) kmer_select_kernel(SelectArgs a) {
    kmer_select_body<kTopMax, false>(a);
}
template <int kTopMax>
__global__ void __launch_bounds__(kSelThreads) kmer_select_big_kernel(SelectArgs a) {
    kmer_select_body<kTopMax, true>(a);
}
// sorted keys of a launch range ([nq][M], every segment descending) -> ids, scores, out_n
__global__ void kmer_unpack_keys(const unsigned long long *keys, uint32_t nq, uint32_t M, uint32_t *out_ids, float *out_scores,
                                 uint32_t *out_n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq) out_n[i] = M;
    if (i >= (uint64_t)nq * M) return;
    const unsigned long long c = keys[i];
    out_ids[i] = (uint32_t)c;
    out_scores[i] = (float)((int)(uint32_t)(c >> 32) - 32768);
}
// segment q of the keys: [q M, (q + 1) M)
struct BigSegOffset {
    uint32_t M;
    __host__ __device__ uint32_t operator()(uint32_t q) const { return q * M; }
};
// every segment is longer than any warp or block sort takes: one workgroup per segment, radix passes of 8 bits, and no
// partition of the segments by length (which reads its counts back on the host in the middle of the launch)
using BigSortConfig = rocprim::segmented_radix_sort_config<8, rocprim::kernel_config<256, 16>>;

// Top-M out of the candidate list kmer_count_kernel<true> left for the query: a bitonic sort of its keys (score,
// id) descending.  out_n = 0xFFFFFFFF: the list overflowed -- the host repeats the launch with the score rows.
struct SelectCandArgs {
    const unsigned long long *cand;
    const uint32_t *cand_n;
    uint32_t cand_cap;
    uint32_t *out_ids;
    float *out_scores;
    uint32_t *out_n;
    uint32_t max;
};
__global__ void __launch_bounds__(kSelThreads) kmer_select_cand_kernel(SelectCandArgs a) {
    __shared__ unsigned long long cand[kSelMax];
    const uint32_t q = blockIdx.x;
    const uint32_t have = a.cand_n[q];
    if (have > a.cand_cap) {
        if (threadIdx.x == 0) a.out_n[q] = 0xFFFFFFFFu;
        return;
    }
    const uint32_t n = have, M = a.max;
    uint32_t P = 1;
    while (P < n) P <<= 1;
    for (uint32_t i = threadIdx.x; i < P; i += kSelThreads) cand[i] = i < n ? a.cand[(size_t)q * a.cand_cap + i] : 0ull;
    __syncthreads();
    for (uint32_t k2 = 2; k2 <= P; k2 <<= 1) {
        for (uint32_t j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (uint32_t i = threadIdx.x; i < P; i += kSelThreads) {
                const uint32_t ixj = i ^ j2;
                if (ixj > i) {
                    const unsigned long long x = cand[i], y = cand[ixj];
                    const bool desc = ((i & k2) == 0);
                    if (desc ? (x < y) : (x > y)) {
                        cand[i] = y;
                        cand[ixj] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < M; i += kSelThreads) {
        if (i < n) {
            const unsigned long long c = cand[i];
            a.out_ids[(size_t)q * a.max + i] = (uint32_t)c;
            a.out_scores[(size_t)q * a.max + i] = (float)((int)(uint32_t)(c >> 32) - 32768);
        }
    }
    if (threadIdx.x == 0) a.out_n[q] = n < M ? n : M;
}

}  // namespace

static int index_ready(sina_hip_ctx *c) {
    if (!c->st->have_refs) SH_FAIL("k-mer search: no references uploaded");
    if (!c->st->have_index) SH_FAIL("k-mer search: no index (call sina_hip_build_index / upload_index)");
    return 0;
}

// Posting lists longer than 1/64 of the references (k-mers of conserved regions: a few hundred per
// query hold 97 % of its postings) as bitmaps over the references, zero-padded to whole tiles, for
// the count kernel's atomic-free path.  (By bytes a bitmap breaks even with a list at 1/32; the bitmaps of all
// queries in flight are the same few thousand and come out of L2 / MALL, the lists out of HBM: 1/64 .. 1/128
// measured 4 % faster at 100 000 references, 9 % at 500 000 -- tools/perf_kmer_dense.py.)  Built from the CSR index by the first search after the
// index changed (also when the index arrived by broadcast), under the store's mutex.
static int ensure_dense(sina_hip_ctx *c) {
    sina_hip_store *st = c->st;
    std::lock_guard<std::mutex> lk(st->aux_mu);
    if (st->dense_ready) return 0;
    hipStream_t s = c->stream;
    const uint32_t nk = 1u << (2 * st->k);
    uint32_t div_ = 64;
    if (const std::string e_ = test_knob("dense_div"); !e_.empty()) div_ = (uint32_t)std::max(1, atoi(e_.c_str()));
    const uint32_t thresh = std::max<uint32_t>(256u, st->n_refs / div_);
    const uint32_t ntiles = (st->n_refs + kTileRefs - 1) / kTileRefs;
    st->dense_words = ntiles * (uint32_t)(kTileRefs / 32);
    sina_hip::DevBuf counter;
    if (st->dense_id.reserve_exact(4 * (size_t)nk) || counter.reserve_exact(4)) return 1;
    SH_CHECK(hipMemsetAsync(counter.p, 0, 4, s));
    hipLaunchKernelGGL(mark_dense, dim3((nk + 255) / 256), dim3(256), 0, s, st->idx_off.as<uint32_t>(), nk, thresh,
                       st->dense_id.as<uint32_t>(), counter.as<uint32_t>());
    SH_CHECK(hipGetLastError());
    SH_CHECK(hipStreamSynchronize(s));
    uint32_t nd = 0;
    SH_CHECK(hipMemcpy(&nd, counter.p, 4, hipMemcpyDeviceToHost));
    counter.release();
    st->n_dense = nd;
    if (nd) {
        const size_t bytes = 4 * (size_t)nd * st->dense_words;
        if (st->dense_bits.reserve_exact(bytes)) return 1;
        SH_CHECK(hipMemsetAsync(st->dense_bits.p, 0, bytes, s));
        hipLaunchKernelGGL(fill_dense, dim3((unsigned)(((uint64_t)nk * 64 + 255) / 256)), dim3(256), 0, s,
                           st->idx_off.as<uint32_t>(), st->idx_ids.as<uint32_t>(), st->dense_id.as<uint32_t>(), nk,
                           st->dense_bits.as<uint32_t>(), st->dense_words);
        SH_CHECK(hipGetLastError());
    }
    SH_CHECK(hipStreamSynchronize(s));  // (other contexts' streams read it next)
    st->dense_ready = true;
    return 0;
}

// counts + selects for nq queries whose masks are already on the device
// (the candidate-list path, kmer_count_kernel<true>: at least two tiles of references -- tile 0 must hold `max`
// of them --, a top-M small enough for the list; SINA_HIP_TEST=kmer_rows=1 keeps the score rows)
constexpr uint32_t kCandCap = 4096, kCandMaxM = 128;
static bool kmer_cand_path(const sina_hip_ctx *c, uint32_t max) {
    return max <= kCandMaxM && c->st->n_refs >= 2u * (uint32_t)kTileRefs && atoi(test_knob("kmer_rows").c_str()) == 0;
}
// long_path: the queries of this range are longer than kMaxQueryLen -- the long count kernel and its select kernel,
// score rows only
// big select (max > kSelMax; the caller has clipped max to n_refs, so M = max): kmer_select_big_kernel leaves every
// query's M survivors as keys in its segment, one segmented radix sort -- descending over the 48 bits a key can have
// -- orders all segments of the range, kmer_unpack_keys writes ids, scores and out_n.  Keys, their double buffer and
// rocPRIM's temporary storage are context buffers that only grow: sized here, before anything is launched.
static int kmer_topk_device(sina_hip_ctx *c, const uint8_t *d_qmask, const uint64_t *d_qoff, uint32_t nq,
                            uint32_t max, uint32_t max_qlen, bool want_scores_only, bool cand_path, bool long_path = false) {
    hipStream_t s = c->stream;
    const uint32_t stride = (c->st->n_refs + 7u) & ~7u;  // rows 16-byte aligned (vector loads in the select kernel)
    const bool big = !want_scores_only && !cand_path && max > (uint32_t)kSelMax;
    using seg_iter = rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, BigSegOffset, uint32_t>;
    const seg_iter seg_begin(rocprim::counting_iterator<uint32_t>(0), BigSegOffset{max});
    const size_t n_keys = (size_t)nq * max;
    size_t sort_tmp = 0;
    if (big) {
        if (n_keys > 0x7FFFFFFFull) SH_FAIL("kmer_topk: a launch range of the big select holds more than 2^31 candidates");
        if (c->k_big_keys.reserve(2 * 8 * n_keys)) return 1;
        rocprim::double_buffer<unsigned long long> kb(c->k_big_keys.as<unsigned long long>(), c->k_big_keys.as<unsigned long long>() + n_keys);
        SH_CHECK(rocprim::segmented_radix_sort_keys_desc<BigSortConfig>(nullptr, sort_tmp, kb, (unsigned)n_keys, nq, seg_begin,
                                                                        seg_begin + 1, 0u, 48u, s));
        if (c->k_big_tmp.reserve(sort_tmp + 16)) return 1;
    }
    if ((!cand_path && c->k_scores.reserve((size_t)nq * stride * 2 + 64)) || c->k_tmp2.reserve(8) || c->k_tmp0.reserve(4 * (size_t)nq) ||
        (cand_path && (c->k_tmp1.reserve(8 * (size_t)nq * kCandCap) || c->k_out_n.reserve((size_t)nq * 4))))
        return 1;
    SH_CHECK(hipMemsetAsync(c->k_tmp2.p, 0, 8, s));
    CountArgs ca;
    ca.qmask = d_qmask;
    ca.qoff = d_qoff;
    ca.idx_off = c->st->idx_off.as<uint32_t>();
    ca.idx_ids = c->st->idx_ids.as<uint32_t>();
    ca.scores = c->k_scores.as<int16_t>();
    ca.nkq = c->k_tmp0.as<uint32_t>();
    ca.postings = c->k_tmp2.as<unsigned long long>();
    ca.n_refs = c->st->n_refs;
    ca.stride = stride;
    ca.kmax = long_path ? (uint32_t)kMaxQueryLen : (max_qlen + 63u) & ~63u;
    ca.k = c->st->k;
    ca.fast = c->st->nofast ? 0 : 1;
    if (ensure_dense(c)) return 1;
    ca.dense_id = c->st->n_dense ? c->st->dense_id.as<uint32_t>() : nullptr;
    ca.dense_bits = c->st->dense_bits.as<uint32_t>();
    ca.dense_words = c->st->dense_words;
    ca.cand = cand_path ? c->k_tmp1.as<unsigned long long>() : nullptr;
    ca.cand_n = cand_path ? c->k_out_n.as<uint32_t>() : nullptr;  // (kmer_select_cand_kernel turns it into out_n in place)
    ca.cand_cap = kCandCap;
    ca.topm = max;
    const size_t clds = (size_t)kTileRefs * 2 + (size_t)ca.kmax * 9 + 64 + (long_path ? kLongQbExtra : 0);
    if (allow_full_lds(reinterpret_cast<const void *>(kmer_count_kernel<false>)) ||
        allow_full_lds(reinterpret_cast<const void *>(kmer_count_kernel<true>)) ||
        (long_path && allow_full_lds(reinterpret_cast<const void *>(kmer_count_long_kernel))))
        return 1;
    heavy_launch hl(c, s, kHeavyKmer);  // (count + select: device-filling kernels, ctx.h)
    const hipStream_t hs = hl.stream();
    SH_CHECK(hipEventRecord(c->ev[3], hs));
    if (long_path) hipLaunchKernelGGL(kmer_count_long_kernel, dim3(nq), dim3(kCountThreads), clds, hs, ca);
    else if (cand_path) hipLaunchKernelGGL(kmer_count_kernel<true>, dim3(nq), dim3(kCountThreads), clds, hs, ca);
    else hipLaunchKernelGGL(kmer_count_kernel<false>, dim3(nq), dim3(kCountThreads), clds, hs, ca);
    SH_CHECK(hipGetLastError());
    SH_CHECK(hipEventRecord(c->ev[4], hs));
    if (cand_path) {
        if (c->k_out_ids.reserve((size_t)nq * max * 4) || c->k_out_scores.reserve((size_t)nq * max * 4)) return 1;
        SelectCandArgs sc;
        sc.cand = ca.cand;
        sc.cand_n = ca.cand_n;
        sc.cand_cap = kCandCap;
        sc.out_ids = c->k_out_ids.as<uint32_t>();
        sc.out_scores = c->k_out_scores.as<float>();
        sc.out_n = c->k_out_n.as<uint32_t>();
        sc.max = max;
        hipLaunchKernelGGL(kmer_select_cand_kernel, dim3(nq), dim3(kSelThreads), 0, hs, sc);
        SH_CHECK(hipGetLastError());
    } else if (!want_scores_only) {
        if (c->k_out_ids.reserve((size_t)nq * max * 4) || c->k_out_scores.reserve((size_t)nq * max * 4) ||
            c->k_out_n.reserve((size_t)nq * 4))
            return 1;
        SelectArgs sa;
        sa.scores = ca.scores;
        sa.nkq = ca.nkq;
        sa.stride = stride;
        sa.out_ids = c->k_out_ids.as<uint32_t>();
        sa.out_scores = c->k_out_scores.as<float>();
        sa.out_n = c->k_out_n.as<uint32_t>();
        sa.n_refs = c->st->n_refs;
        sa.max = max;
        sa.keys = big ? c->k_big_keys.as<unsigned long long>() : nullptr;
        // (the rows of the long count kernel hold scores of up to 32757: the search for the cut starts above them)
        if (big && long_path) hipLaunchKernelGGL(kmer_select_big_kernel<kMaxLongQueryLen>, dim3(nq), dim3(kSelThreads), 0, hs, sa);
        else if (big) hipLaunchKernelGGL(kmer_select_big_kernel<kMaxQueryLen>, dim3(nq), dim3(kSelThreads), 0, hs, sa);
        else if (long_path) hipLaunchKernelGGL(kmer_select_kernel<kMaxLongQueryLen>, dim3(nq), dim3(kSelThreads), 0, hs, sa);
        else hipLaunchKernelGGL(kmer_select_kernel<kMaxQueryLen>, dim3(nq), dim3(kSelThreads), 0, hs, sa);
        SH_CHECK(hipGetLastError());
        if (big) {
            rocprim::double_buffer<unsigned long long> kb(sa.keys, sa.keys + n_keys);
            SH_CHECK(rocprim::segmented_radix_sort_keys_desc<BigSortConfig>(c->k_big_tmp.p, sort_tmp, kb, (unsigned)n_keys, nq, seg_begin,
                                                                            seg_begin + 1, 0u, 48u, hs));
            hipLaunchKernelGGL(kmer_unpack_keys, dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, hs, kb.current(), nq, max,
                               sa.out_ids, sa.out_scores, sa.out_n);
            SH_CHECK(hipGetLastError());
        }
    }
    SH_CHECK(hipEventRecord(c->ev[5], hs));
    return hl.done();
}

}  // namespace sina_hip

using namespace sina_hip;

extern "C" {

int sina_hip_upload_index(sina_hip_ctx *c, unsigned k, int nofast, const uint32_t *offsets, const uint32_t *ids,
                          uint64_t n_postings) {
    if (!c || !offsets || (!ids && n_postings)) SH_FAIL("upload_index: null argument");
    if (k < 1 || k > 12) SH_FAIL("upload_index: k must be in 1..12");
    if (!c->owns_store) SH_FAIL("upload_index: a forked context cannot change the reference store");
    std::lock_guard<std::mutex> lk(c->mu);
    SH_CHECK(hipSetDevice(c->device));
    const uint64_t nk = 1ull << (2 * k);
    if (c->st->idx_off.reserve(4 * (nk + 1)) || c->st->idx_ids.reserve(4 * std::max<uint64_t>(n_postings, 1))) return 1;
    SH_CHECK(hipMemcpyAsync(c->st->idx_off.p, offsets, 4 * (nk + 1), hipMemcpyHostToDevice, c->stream));
    if (n_postings)
        SH_CHECK(hipMemcpyAsync(c->st->idx_ids.p, ids, 4 * n_postings, hipMemcpyHostToDevice, c->stream));
    SH_CHECK(hipStreamSynchronize(c->stream));
    c->st->k = k;
    c->st->nofast = nofast ? 1 : 0;
    c->st->n_postings = n_postings;
    c->st->have_index = true;
    c->st->dense_ready = false;
    return 0;
}

int sina_hip_download_index(sina_hip_ctx *c, uint32_t *offsets, uint32_t *ids) {
    if (!c || !offsets) SH_FAIL("download_index: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->st->have_index) SH_FAIL("download_index: no index");
    if (!ids && c->st->n_postings) SH_FAIL("download_index: null ids");
    SH_CHECK(hipSetDevice(c->device));
    const uint64_t nk = 1ull << (2 * c->st->k);
    SH_CHECK(hipMemcpy(offsets, c->st->idx_off.p, 4 * (nk + 1), hipMemcpyDeviceToHost));
    if (c->st->n_postings) SH_CHECK(hipMemcpy(ids, c->st->idx_ids.p, 4 * c->st->n_postings, hipMemcpyDeviceToHost));
    return 0;
}

int sina_hip_build_index(sina_hip_ctx *c, unsigned k, int nofast) {
    if (!c) SH_FAIL("build_index: null ctx");
    if (k < 1 || k > 12) SH_FAIL("build_index: k must be in 1..12");
    if (!c->owns_store) SH_FAIL("build_index: a forked context cannot change the reference store");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->st->have_refs) SH_FAIL("build_index: upload references first");
    SH_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint64_t n = c->st->total_bases;
    const uint64_t nk = 1ull << (2 * k);
    if (n >= (1ull << 32)) SH_FAIL("build_index: more than 2^32 reference bases");
    DevBuf keys_in, keys_out, flag, pos, tmp;
    int rc = 1;
    do {
        if (keys_in.reserve(8 * std::max<uint64_t>(n, 1)) || keys_out.reserve(8 * std::max<uint64_t>(n, 1)) ||
            flag.reserve(4 * std::max<uint64_t>(n, 1)) || pos.reserve(4 * std::max<uint64_t>(n, 1)))
            break;
        if (c->st->n_refs)
            hipLaunchKernelGGL(ref_kmer_keys, dim3(c->st->n_refs), dim3(256), 0, s, c->st->ref_ab.as<uint32_t>(),
                               c->st->ref_off.as<uint64_t>(), c->st->n_refs, k, nofast == 0, keys_in.as<uint64_t>());
        size_t tb = 0;
        const int end_bit = 32 + 2 * (int)k;
        // (rocPRIM directly; only the bits a key can have: k-mer << 32 | reference id)
        if (rocprim::radix_sort_keys(nullptr, tb, keys_in.as<uint64_t>(), keys_out.as<uint64_t>(), (size_t)n, 0u,
                                     (unsigned)end_bit, s) != hipSuccess)
            break;
        if (tmp.reserve(tb + 16)) break;
        if (n && rocprim::radix_sort_keys(tmp.p, tb, keys_in.as<uint64_t>(), keys_out.as<uint64_t>(), (size_t)n, 0u,
                                          (unsigned)end_bit, s) != hipSuccess)
            break;
        const unsigned blocks = (unsigned)((n + 255) / 256);
        if (n) hipLaunchKernelGGL(mark_unique, dim3(blocks), dim3(256), 0, s, keys_out.as<uint64_t>(), n,
                                  flag.as<uint32_t>());
        size_t tb2 = 0;
        if (rocprim::exclusive_scan(nullptr, tb2, flag.as<uint32_t>(), pos.as<uint32_t>(), 0u, (size_t)n,
                                    rocprim::plus<uint32_t>(), s) != hipSuccess)
            break;
        if (tmp.reserve(tb2 + 16)) break;
        if (n && rocprim::exclusive_scan(tmp.p, tb2, flag.as<uint32_t>(), pos.as<uint32_t>(), 0u, (size_t)n,
                                         rocprim::plus<uint32_t>(), s) != hipSuccess)
            break;
        uint32_t last_flag = 0, last_pos = 0;
        if (n) {
            if (hipMemcpyAsync(&last_flag, flag.as<uint32_t>() + (n - 1), 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(&last_pos, pos.as<uint32_t>() + (n - 1), 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess)
                break;
        }
        const uint64_t np = (uint64_t)last_flag + last_pos;
        DevBuf counts;
        if (counts.reserve(4 * (nk + 1)) || c->st->idx_off.reserve(4 * (nk + 1)) ||
            c->st->idx_ids.reserve(4 * std::max<uint64_t>(np, 1))) {
            counts.release();
            break;
        }
        bool ok = hipMemsetAsync(counts.p, 0, 4 * (nk + 1), s) == hipSuccess;
        if (ok && n)
            hipLaunchKernelGGL(scatter_unique, dim3(blocks), dim3(256), 0, s, keys_out.as<uint64_t>(),
                               flag.as<uint32_t>(), pos.as<uint32_t>(), n, c->st->idx_ids.as<uint32_t>(),
                               counts.as<uint32_t>());
        size_t tb3 = 0;
        ok = ok && rocprim::exclusive_scan(nullptr, tb3, counts.as<uint32_t>(), c->st->idx_off.as<uint32_t>(), 0u,
                                           (size_t)(nk + 1), rocprim::plus<uint32_t>(), s) == hipSuccess;
        ok = ok && tmp.reserve(tb3 + 16) == 0;
        ok = ok && rocprim::exclusive_scan(tmp.p, tb3, counts.as<uint32_t>(), c->st->idx_off.as<uint32_t>(), 0u,
                                           (size_t)(nk + 1), rocprim::plus<uint32_t>(), s) == hipSuccess;
        ok = ok && hipStreamSynchronize(s) == hipSuccess;
        counts.release();
        if (!ok) break;
        c->st->k = k;
        c->st->nofast = nofast ? 1 : 0;
        c->st->n_postings = np;
        c->st->have_index = true;
        c->st->dense_ready = false;
        rc = 0;
    } while (0);
    keys_in.release();
    keys_out.release();
    flag.release();
    pos.release();
    tmp.release();
    if (rc) {
        hipError_t e = hipGetLastError();
        set_error(std::string("build_index failed: ") + hipGetErrorString(e));
    }
    return rc;
}

// sina_hip_kmer_topk / _any behind their checks (c->mu held, 1 <= max <= n_refs): queries 0 .. n_fast - 1 on the fast
// count kernel (none of them longer than kMaxQueryLen), queries n_fast .. nq - 1 -- every one of them longer -- on the
// long kernel, in launch ranges of their own
// q_ab / out_match (sina_hip_kmer_topk_match; else null): the queries' packed aligned bases, one per mask byte, and
// where every range's match counts go (match.hip), [nq * max] like out_ids
// rk (sina_hip_kmer_topk_rank; else null): the rules under which every range's candidates are ranked where the select
// left them (rank.hip); out_ids / out_scores are then [nq * rk->N] rows of the rank kernel, out_n its counts, and no id
// or k-mer score of the select is copied out
struct RankReq {
    int iupac, filter_lc, cover;
    uint32_t N;
    uint32_t *out_flag;  // [nq]
};
static int kmer_topk_run(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t n_fast,
                         uint32_t max, uint32_t *out_ids, float *out_scores, uint32_t *out_n, const uint32_t *q_ab = nullptr,
                         uint16_t *out_match = nullptr, const RankReq *rk = nullptr) {
    uint32_t max_qlen = 1;
    for (uint32_t q = 0; q < n_fast; q++) max_qlen = std::max<uint32_t>(max_qlen, (uint32_t)(qoff[q + 1] - qoff[q]));
    hipStream_t s = c->stream;
    const uint64_t nqm = qoff[nq] - qoff[0];
    // sub-batches bound the [nq][n_refs] int16 score matrix to ~2 GiB
    uint32_t per = (uint32_t)std::max<uint64_t>(1, ((uint64_t)2 << 30) / (2ull * std::max<uint32_t>(c->st->n_refs, 1)));
    // ... and, for the big select, keys + outputs to kBigSelBudget (kmer_plan.h; SINA_HIP_TEST=big_sel_bytes=N: a test's budget)
    const bool big = max > (uint32_t)kSelMax;
    if (big) {
        uint64_t budget = kBigSelBudget;
        if (const std::string e_ = test_knob("big_sel_bytes"); !e_.empty()) budget = std::min<uint64_t>(kBigSelBudget, strtoull(e_.c_str(), nullptr, 10));
        per = std::min(per, big_select_range(nq, max, budget));
    }
    if (c->qmask.reserve(std::max<uint64_t>(nqm, 1)) || c->k_qoff.reserve(8 * ((uint64_t)nq + 1))) return 1;
    std::vector<uint64_t> rel(nq + 1);
    for (uint32_t q = 0; q <= nq; q++) rel[q] = qoff[q] - qoff[0];
    if (upload(c, 7, c->qmask.p, qmask + qoff[0], nqm, s) || upload(c, 8, c->k_qoff.p, rel.data(), 8 * ((uint64_t)nq + 1), s))
        return 1;
    if ((out_match || rk) && (c->s_qab.reserve(4 * std::max<uint64_t>(nqm, 1)) || upload(c, 1, c->s_qab.p, q_ab + qoff[0], 4 * nqm, s))) return 1;
    // one launch range: kernels, results back through pinned staging, statistics; *overflow = a candidate list of the
    // range did not hold its query's candidates (nothing was copied out then: the caller repeats the range with rows)
    auto run_range = [&](uint32_t q0, uint32_t bq, bool cand_path, bool *overflow, bool long_path = false) -> int {
        if (kmer_topk_device(c, c->qmask.as<uint8_t>(), c->k_qoff.as<uint64_t>() + q0, bq, max, max_qlen, false, cand_path, long_path)) return 1;
        // (the kernels have finished: kmer_topk_device waits for the heavy stream)
        if ((!rk && (download(c, 9, c->k_out_ids.p, (size_t)bq * max * 4, s) || download(c, 10, c->k_out_scores.p, (size_t)bq * max * 4, s))) ||
            download(c, 11, c->k_out_n.p, (size_t)bq * 4, s) || download(c, 0, c->k_tmp2.p, 8, s))
            return 1;
        SH_CHECK(wait_stream(c, s));
        *overflow = false;
        if (cand_path) {
            const uint32_t *n = static_cast<const uint32_t *>(c->h_stage[11].p);
            for (uint32_t q = 0; q < bq && !*overflow; q++) *overflow = n[q] == 0xFFFFFFFFu;
        }
        unsigned long long visited = 0;
        memcpy(&visited, c->h_stage[0].p, 8);
        float ms = 0, ms2 = 0;
        SH_CHECK(hipEventElapsedTime(&ms, c->ev[3], c->ev[4]));
        SH_CHECK(hipEventElapsedTime(&ms2, c->ev[4], c->ev[5]));
        {
            std::lock_guard<std::mutex> slk(c->st->stats_mu);
            c->st->stats.kmer_count_ms += ms;
            c->st->stats.kmer_select_ms += ms2;
            c->st->stats.kmer_launches++;
            if (!*overflow) {
                c->st->stats.postings += visited;
                c->st->stats.kmer_queries += bq;
            }
        }
        if (*overflow) return 0;
        if (long_path) c->path_queries[kPathLong] += bq;
        if (big) c->path_queries[kPathBigSelect] += bq;
        if (rk) {  // the range's select is final: its candidates ranked, ids and lengths read where they lie
            uint32_t max_la = 0;
            for (uint32_t q = q0; q < q0 + bq; q++) max_la = std::max<uint32_t>(max_la, (uint32_t)(qoff[q + 1] - qoff[q]));
            return rank_launch(c, c->s_qab.as<uint32_t>(), c->k_qoff.as<uint64_t>() + q0, bq, c->k_out_ids.as<uint32_t>(), nullptr,
                               c->k_out_n.as<uint32_t>(), max, max, max_la, rk->iupac, rk->filter_lc, rk->cover, rk->N,
                               out_ids + (size_t)q0 * rk->N, out_scores + (size_t)q0 * rk->N, out_n + q0, rk->out_flag + q0);
        }
        memcpy(out_ids + (size_t)q0 * max, c->h_stage[9].p, (size_t)bq * max * 4);
        memcpy(out_scores + (size_t)q0 * max, c->h_stage[10].p, (size_t)bq * max * 4);
        memcpy(out_n + q0, c->h_stage[11].p, (size_t)bq * 4);
        if (out_match) {  // the range's select is final: its candidates' match counts, ids and lengths read where they lie
            const size_t row_bytes = (size_t)bq * max * 2;
            if (c->m_out.reserve(row_bytes)) return 1;
            SH_CHECK(hipMemsetAsync(c->m_out.p, 0, row_bytes, s));
            if (match_launch(c, c->s_qab.as<uint32_t>(), c->k_qoff.as<uint64_t>() + q0, bq, c->k_out_ids.as<uint32_t>(),
                             c->k_out_n.as<uint32_t>(), max, c->m_out.as<uint16_t>(), static_cast<const uint32_t *>(c->h_stage[9].p),
                             static_cast<const uint32_t *>(c->h_stage[11].p)) ||
                download(c, 5, c->m_out.p, row_bytes, s))
                return 1;
            SH_CHECK(wait_stream(c, s));
            memcpy(out_match + (size_t)q0 * max, c->h_stage[5].p, row_bytes);
        }
        return 0;
    };
    const bool cand_path = kmer_cand_path(c, max);
    const uint32_t per_cand = 16384;  // (candidate lists: 32 KB per query)
    for (uint32_t q0 = 0; q0 < n_fast; q0 += cand_path ? per_cand : per) {
        const uint32_t bq = std::min(cand_path ? per_cand : per, n_fast - q0);
        bool overflow = false;
        if (run_range(q0, bq, cand_path, &overflow)) return 1;
        if (overflow)  // a giant group of equal scores somewhere in the range: the score rows and the full select
            for (uint32_t r0 = q0; r0 < q0 + bq; r0 += per) {
                bool dummy = false;
                if (run_range(r0, std::min(per, q0 + bq - r0), false, &dummy)) return 1;
            }
    }
    for (uint32_t q0 = n_fast; q0 < nq; q0 += per) {
        bool dummy = false;
        if (run_range(q0, std::min(per, nq - q0), false, &dummy, true)) return 1;
    }
    return 0;
}

// any: queries of up to kMaxLongQueryLen bases (sina_hip_kmer_topk_any), the longer ones behind the others for
// kmer_topk_run and back into the caller's order
static int kmer_topk_checked(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t max,
                             uint32_t *out_ids, float *out_scores, uint32_t *out_n, bool any, const uint32_t *q_ab = nullptr,
                             uint16_t *out_match = nullptr, const RankReq *rk = nullptr) {
    if (!c || !qmask || !qoff || !out_ids || !out_scores || !out_n) SH_FAIL("kmer_topk: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    sina_hip_hint_guard hints(c);
    if (index_ready(c)) return 1;
    if (out_match && match_table_bytes(c->st->width) > kMatchMaxLds)
        SH_FAIL_LIMIT("kmer_topk_match: alignment too wide for the device match count");
    if (rk) {
        if (rank_check_rules("kmer_topk_rank", c, rk->iupac, rk->cover, rk->N)) return 1;
        uint32_t max_la = 0;
        for (uint32_t q = 0; q < nq; q++) max_la = std::max<uint32_t>(max_la, (uint32_t)(qoff[q + 1] - qoff[q]));
        if (compare_table_bytes(c->st->width, max_la) > kCompareMaxLds)
            SH_FAIL_LIMIT("kmer_topk_rank: alignment too wide for the device comparison");
        if (std::min(max, c->st->n_refs) > (uint32_t)kSelMax)
            SH_FAIL_LIMIT("kmer_topk_rank: more than 4096 candidates per query");
    }
    if (nq == 0) return 0;
    SH_CHECK(hipSetDevice(c->device));
    if (max > c->st->n_refs) max = c->st->n_refs;
    if (max == 0) {
        memset(out_n, 0, sizeof(uint32_t) * nq);
        if (rk) memset(rk->out_flag, 0, sizeof(uint32_t) * nq);
        return 0;
    }
    uint32_t n_long = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const uint64_t len = qoff[q + 1] - qoff[q];
        if (!any && len > (uint64_t)kMaxQueryLen) SH_FAIL("kmer_topk: query longer than SINA_HIP_MAX_QUERY_LEN bases");
        if (len > (uint64_t)kMaxLongQueryLen) SH_FAIL_LIMIT("kmer_topk_any: query longer than SINA_HIP_MAX_LONG_QUERY_LEN bases");
        n_long += len > (uint64_t)kMaxQueryLen;
    }
    if (n_long == 0) return kmer_topk_run(c, qmask, qoff, nq, nq, max, out_ids, out_scores, out_n, q_ab, out_match, rk);
    const uint32_t n_fast = nq - n_long;
    const uint32_t row = rk ? rk->N : max;  // entries of an output row
    std::vector<uint32_t> order(nq);  // order[slot] = the caller's query
    for (uint32_t q = 0, f = 0, l = n_fast; q < nq; q++) order[qoff[q + 1] - qoff[q] > (uint64_t)kMaxQueryLen ? l++ : f++] = q;
    std::vector<uint64_t> off(nq + 1, 0);
    for (uint32_t x = 0; x < nq; x++) off[x + 1] = off[x] + (qoff[order[x] + 1] - qoff[order[x]]);
    std::vector<uint8_t> mask(off[nq]);
    for (uint32_t x = 0; x < nq; x++) memcpy(mask.data() + off[x], qmask + qoff[order[x]], off[x + 1] - off[x]);
    std::vector<uint32_t> ids((size_t)nq * row), n(nq), fl(rk ? nq : 0);
    std::vector<float> sc((size_t)nq * row);
    std::vector<uint32_t> ab(q_ab ? off[nq] : 0);  // (the packed bases and the match rows move with their queries)
    std::vector<uint16_t> mt(out_match ? (size_t)nq * max : 0);
    if (q_ab)
        for (uint32_t x = 0; x < nq; x++) memcpy(ab.data() + off[x], q_ab + qoff[order[x]], 4 * (off[x + 1] - off[x]));
    RankReq rk2;
    if (rk) {
        rk2 = *rk;
        rk2.out_flag = fl.data();
    }
    if (kmer_topk_run(c, mask.data(), off.data(), nq, n_fast, max, ids.data(), sc.data(), n.data(), q_ab ? ab.data() : nullptr,
                      out_match ? mt.data() : nullptr, rk ? &rk2 : nullptr))
        return 1;
    for (uint32_t x = 0; x < nq; x++) {
        if (out_match) memcpy(out_match + (size_t)order[x] * max, mt.data() + (size_t)x * max, (size_t)max * 2);
        memcpy(out_ids + (size_t)order[x] * row, ids.data() + (size_t)x * row, (size_t)row * 4);
        memcpy(out_scores + (size_t)order[x] * row, sc.data() + (size_t)x * row, (size_t)row * 4);
        out_n[order[x]] = n[x];
        if (rk) rk->out_flag[order[x]] = fl[x];
    }
    return 0;
}

static int kmer_scores_checked(sina_hip_ctx *c, const uint8_t *qmask, uint32_t qlen, int16_t *scores, bool any) {
    if (!c || !qmask || !scores) SH_FAIL("kmer_scores: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (index_ready(c)) return 1;
    if (!any && qlen > (uint32_t)kMaxQueryLen) SH_FAIL("kmer_scores: query longer than SINA_HIP_MAX_QUERY_LEN bases");
    if (qlen > (uint32_t)kMaxLongQueryLen) SH_FAIL_LIMIT("kmer_scores_any: query longer than SINA_HIP_MAX_LONG_QUERY_LEN bases");
    const bool long_path = qlen > (uint32_t)kMaxQueryLen;
    SH_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint64_t rel[2] = {0, qlen};
    if (c->qmask.reserve(std::max<uint32_t>(qlen, 1)) || c->k_qoff.reserve(16)) return 1;
    SH_CHECK(hipMemcpyAsync(c->qmask.p, qmask, qlen, hipMemcpyHostToDevice, s));
    SH_CHECK(hipMemcpyAsync(c->k_qoff.p, rel, 16, hipMemcpyHostToDevice, s));
    if (kmer_topk_device(c, c->qmask.as<uint8_t>(), c->k_qoff.as<uint64_t>(), 1, 1, std::max<uint32_t>(qlen, 1), true, false, long_path)) return 1;
    if (long_path) c->path_queries[kPathLong]++;
    SH_CHECK(hipMemcpyAsync(scores, c->k_scores.p, (size_t)c->st->n_refs * 2, hipMemcpyDeviceToHost, s));
    SH_CHECK(hipStreamSynchronize(s));
    return 0;
}

int sina_hip_kmer_topk(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t max,
                       uint32_t *out_ids, float *out_scores, uint32_t *out_n) {
    return kmer_topk_checked(c, qmask, qoff, nq, max, out_ids, out_scores, out_n, false);
}
int sina_hip_kmer_topk_any(sina_hip_ctx *c, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t max,
                           uint32_t *out_ids, float *out_scores, uint32_t *out_n) {
    return kmer_topk_checked(c, qmask, qoff, nq, max, out_ids, out_scores, out_n, true);
}
int sina_hip_kmer_topk_match(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t max,
                             uint32_t *out_ids, float *out_scores, uint32_t *out_n, uint16_t *out_match) {
    if (!c || !q_ab || !q_off || !out_ids || !out_scores || !out_n || !out_match) SH_FAIL("kmer_topk_match: null argument");
    if (match_check_queries("kmer_topk_match", q_ab, q_off, nq)) return 1;
    // the mask bytes the count kernel reads, one per packed word; offsets from the first query's first base
    const uint64_t b = q_off[0], e = q_off[nq];
    std::vector<uint8_t> mask(e - b + 1);
    for (uint64_t i = b; i < e; i++) mask[i - b] = (uint8_t)(q_ab[i] >> 24);
    std::vector<uint64_t> rel(nq + 1);
    for (uint32_t q = 0; q <= nq; q++) rel[q] = q_off[q] - b;
    return kmer_topk_checked(c, mask.data(), rel.data(), nq, max, out_ids, out_scores, out_n, true, q_ab + b, out_match);
}
int sina_hip_kmer_topk_rank(sina_hip_ctx *c, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t kmer_candidates,
                            int iupac_rule, int filter_lowercase, int cover_rule, uint32_t max_result, uint32_t *out_ids,
                            float *out_scores, uint32_t *out_n, uint32_t *out_flag) {
    if (!c || !q_ab || !q_off || !out_ids || !out_scores || !out_n || !out_flag) SH_FAIL("kmer_topk_rank: null argument");
    if (match_check_queries("kmer_topk_rank", q_ab, q_off, nq)) return 1;
    const uint64_t b = q_off[0], e = q_off[nq];
    std::vector<uint8_t> mask(e - b + 1);
    for (uint64_t i = b; i < e; i++) mask[i - b] = (uint8_t)(q_ab[i] >> 24);
    std::vector<uint64_t> rel(nq + 1);
    for (uint32_t q = 0; q <= nq; q++) rel[q] = q_off[q] - b;
    // (results through vectors of the call's own: the outputs stay untouched if a range fails)
    std::vector<uint32_t> ids((size_t)nq * std::max(max_result, 1u)), n(nq), fl(nq);
    std::vector<float> sc(ids.size());
    const RankReq rk{iupac_rule, filter_lowercase ? 1 : 0, cover_rule, max_result, fl.data()};
    if (kmer_topk_checked(c, mask.data(), rel.data(), nq, kmer_candidates, ids.data(), sc.data(), n.data(), true, q_ab + b, nullptr, &rk))
        return 1;
    memcpy(out_ids, ids.data(), 4 * (size_t)nq * max_result);
    memcpy(out_scores, sc.data(), 4 * (size_t)nq * max_result);
    memcpy(out_n, n.data(), 4 * (size_t)nq);
    memcpy(out_flag, fl.data(), 4 * (size_t)nq);
    return 0;
}
int sina_hip_kmer_scores(sina_hip_ctx *c, const uint8_t *qmask, uint32_t qlen, int16_t *scores) {
    return kmer_scores_checked(c, qmask, qlen, scores, false);
}
int sina_hip_kmer_scores_any(sina_hip_ctx *c, const uint8_t *qmask, uint32_t qlen, int16_t *scores) {
    return kmer_scores_checked(c, qmask, qlen, scores, true);
}
int sina_hip_long_queries(sina_hip_ctx *c, uint64_t *n) {
    if (!c || !n) SH_FAIL("long_queries: null argument");
    return read_path_queries(c, kPathLong, n);
}

int sina_hip_big_select_queries(sina_hip_ctx *c, uint64_t *n) {
    if (!c || !n) SH_FAIL("big_select_queries: null argument");
    return read_path_queries(c, kPathBigSelect, n);
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

}  // extern "C"
