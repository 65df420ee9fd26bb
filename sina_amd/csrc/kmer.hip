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
//
// This unit: the count and select kernels, their argument structs and one launcher per stage (launch_kmer_count,
// launch_kmer_select: common.h).  The index and the dense bitmaps are kmer_index.hip's, the driver of a search call
// is kmer_launch.hip, and every decision either takes -- geometry, paths, launch ranges -- is kmer_plan.h's.
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <type_traits>

#include "common.h"
#include "ctx.h"
#include "kmer_plan.h"

namespace sina_hip {
namespace {

constexpr int kCountThreads = 1024;
constexpr int kWide = 2;                    // 1 KiB loads a wave of the count kernel keeps in flight
constexpr int kMaxQueryLen = (int)SINA_HIP_MAX_QUERY_LEN;  // k-mer list capacity in LDS: 64 KiB tile + 9 B per base <= 160 KiB
static_assert(kmer_count_lds(kmer_kmax(kMaxQueryLen, kKmerRows), kKmerRows) <= 160 * 1024, "LDS of the count kernel");
// the long count kernel: a query of up to SINA_HIP_MAX_LONG_QUERY_LEN bases in chunks of
// kLongChunk windows, each chunk with the k-mer list capacity of the fast kernel -- and its k - 1 <= 11 bases before
// the chunk's first window end in qb[] (the 64 bytes more)
constexpr int kMaxLongQueryLen = (int)SINA_HIP_MAX_LONG_QUERY_LEN;
constexpr int kLongChunk = (int)SINA_HIP_KMER_LONG_CHUNK;
static_assert(kLongChunk <= kMaxQueryLen && kMaxLongQueryLen <= 32767, "a chunk fits the fast kernel's lists; int16 scores");
static_assert(kmer_count_lds(kmer_kmax(0, kKmerLong), kKmerLong) <= 160 * 1024, "LDS of the long count kernel");
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
    // dense posting lists as bitmaps (kmer_index.hip, ensure_dense): bitmap number per k-mer or kNoDense, words per bitmap
    const uint32_t *dense_id;
    const uint32_t *dense_bits;
    uint32_t dense_words;
    uint32_t dense_zero;  // number of the all-zero bitmap behind the lists' (no k-mer's: pads a query's list to eights)
    // CAND (kmer_count_kernel<true>): instead of the score row, the references that can still be among the top
    // `topm` -- keys (score + 32768) << 32 | id, at most cand_cap per query; cand_n[q] = how many there were
    unsigned long long *cand;
    uint32_t *cand_n;
    uint32_t cand_cap, topm;
};

constexpr uint32_t kMaxDenseQ = 1023;  // dense k-mers of one query counted bit-sliced in 10 planes
static_assert(kTileRefs / 32 == kCountThreads, "one bitmap word of the tile per thread");

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

// The big select's sort: the range's nq segments of M keys each, descending over the 48 bits a key can have.
// tmp == nullptr: only the size of rocPRIM's temporary storage.
hipError_t big_sort(void *tmp, size_t &tmp_bytes, rocprim::double_buffer<unsigned long long> &kb, uint32_t nq, uint32_t M,
                    hipStream_t s) {
    using seg_iter = rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, BigSegOffset, uint32_t>;
    const seg_iter seg_begin(rocprim::counting_iterator<uint32_t>(0), BigSegOffset{M});
    return rocprim::segmented_radix_sort_keys_desc<BigSortConfig>(tmp, tmp_bytes, kb, (unsigned)((size_t)nq * M), nq, seg_begin,
                                                                  seg_begin + 1, 0u, 48u, s);
}

}  // namespace

// ---------------------------------------------------------------- launchers (common.h)
// The range's buffers -- the context's k_* scratch -- are reserved by the driver (kmer_launch.hip, reserve_range).

int launch_kmer_count(sina_hip_ctx *c, const KmerLaunch &l, hipStream_t s) {
    const sina_hip_store *st = c->st;
    const bool cand = l.path == kKmerCand;
    const CountArgs a{l.qmask, l.qoff, st->idx_off.as<uint32_t>(), st->idx_ids.as<uint32_t>(), c->k_scores.as<int16_t>(), c->k_tmp0.as<uint32_t>(),
                      c->k_tmp2.as<unsigned long long>(), st->n_refs, (uint32_t)kmer_row_stride(st->n_refs), kmer_kmax(l.max_qlen, l.path), st->k,
                      st->nofast ? 0 : 1, st->n_dense ? st->dense_id.as<uint32_t>() : nullptr, st->dense_bits.as<uint32_t>(), st->dense_words, st->n_dense,
                      // (the candidate lists; kmer_select_cand_kernel turns cand_n into out_n in place)
                      cand ? c->k_tmp1.as<unsigned long long>() : nullptr, cand ? c->k_out_n.as<uint32_t>() : nullptr, kCandCap, l.max};
    void (*kernel)(CountArgs) = l.path == kKmerLong ? kmer_count_long_kernel : (cand ? kmer_count_kernel<true> : kmer_count_kernel<false>);
    if (allow_full_lds(reinterpret_cast<const void *>(kernel))) return 1;
    hipLaunchKernelGGL(kernel, dim3(l.nq), dim3(kCountThreads), kmer_count_lds(a.kmax, l.path), s, a);
    SH_CHECK(hipGetLastError());
    return 0;
}

// big select (l.big; the caller has clipped max to n_refs, so M = max): keys, their double buffer and rocPRIM's
// temporary storage are context buffers that only grow -- sized here, before anything of the range is launched
int reserve_kmer_big_select(sina_hip_ctx *c, KmerLaunch *l) {
    l->big_tmp_bytes = 0;
    if (!l->big) return 0;
    const size_t n_keys = (size_t)l->nq * l->max;
    if (n_keys > 0x7FFFFFFFull) SH_FAIL("kmer_topk: a launch range of the big select holds more than 2^31 candidates");
    if (c->k_big_keys.reserve(2 * 8 * n_keys)) return 1;
    rocprim::double_buffer<unsigned long long> kb(c->k_big_keys.as<unsigned long long>(), c->k_big_keys.as<unsigned long long>() + n_keys);
    SH_CHECK(big_sort(nullptr, l->big_tmp_bytes, kb, l->nq, l->max, c->stream));
    return c->k_big_tmp.reserve(l->big_tmp_bytes + 16);
}

// Candidate lists: kmer_select_cand_kernel.  Score rows: kmer_select_kernel, or kmer_select_big_kernel leaving every
// query's M survivors as keys in its segment, one segmented radix sort over all segments of the range, and
// kmer_unpack_keys writing ids, scores and out_n.
int launch_kmer_select(sina_hip_ctx *c, const KmerLaunch &l, hipStream_t s) {
    if (l.path == kKmerCand) {
        const SelectCandArgs a{c->k_tmp1.as<unsigned long long>(), c->k_out_n.as<uint32_t>(), kCandCap, c->k_out_ids.as<uint32_t>(),
                               c->k_out_scores.as<float>(), c->k_out_n.as<uint32_t>(), l.max};
        hipLaunchKernelGGL(kmer_select_cand_kernel, dim3(l.nq), dim3(kSelThreads), 0, s, a);
        SH_CHECK(hipGetLastError());
        return 0;
    }
    const SelectArgs a{c->k_scores.as<int16_t>(), c->k_tmp0.as<uint32_t>(), c->k_out_ids.as<uint32_t>(), c->k_out_scores.as<float>(),
                       c->k_out_n.as<uint32_t>(), c->st->n_refs, (uint32_t)kmer_row_stride(c->st->n_refs), l.max,
                       l.big ? c->k_big_keys.as<unsigned long long>() : nullptr};
    // (the rows of the long count kernel hold scores of up to 32757: the search for the cut starts above them)
    const bool lng = l.path == kKmerLong;
    void (*kernel)(SelectArgs) = l.big ? (lng ? kmer_select_big_kernel<kMaxLongQueryLen> : kmer_select_big_kernel<kMaxQueryLen>)
                                       : (lng ? kmer_select_kernel<kMaxLongQueryLen> : kmer_select_kernel<kMaxQueryLen>);
    hipLaunchKernelGGL(kernel, dim3(l.nq), dim3(kSelThreads), 0, s, a);
    SH_CHECK(hipGetLastError());
    if (l.big) {
        const size_t n_keys = (size_t)l.nq * l.max;
        size_t tmp_bytes = l.big_tmp_bytes;
        rocprim::double_buffer<unsigned long long> kb(a.keys, a.keys + n_keys);
        SH_CHECK(big_sort(c->k_big_tmp.p, tmp_bytes, kb, l.nq, l.max, s));
        hipLaunchKernelGGL(kmer_unpack_keys, dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, s, kb.current(), l.nq, l.max,
                           a.out_ids, a.out_scores, a.out_n);
        SH_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace sina_hip
