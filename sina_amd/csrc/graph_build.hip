// Family DAG build on the GPU + sina_hip_align_families.
//
// What it computes: mseq::mseq + sort + reduce_edges for every query's family
// (reference src/mseq.cpp:47-118, src/graph.h:332-357,451-488; spec SURVEY.md A.3):
//   * one node per (alignment column, IUPAC character incl. case) that occurs in the
//     family; node ids ascend with the column and, inside a column, with the family
//     index of the first reference showing that character;
//   * node weight from the number of references sharing the node (mseq.cpp:113);
//   * edge a->b whenever some reference has consecutive bases in nodes a, b; per node
//     the predecessor ids ascending and unique; sources / sinks implicit.
//
// How it maps to the hardware: one workgroup per query; the alignment is walked in tiles of
// kTC occupied columns.  Every step inside a tile is parallel over the family's BASES in the tile
// ("entries": member j's bases from its cursor on, a contiguous stretch of at most kTC; a wave takes
// 64 consecutive slots of one member, so the member's cursor / length / offset are scalars) and
// meets the other members of a column only through LDS atomics -- no thread ever walks the F members
// of a column (rounds 2-4 did: one thread per column for the nodes, one per node for the edges, 37 %
// of the kernel's time in loops of F iterations that a third of the threads sat out):
//   1. occupied-column bitmap in LDS (atomicOr per base), prefix-popcount -> dense
//      column index ("rank") of every alignment column;
//   2. per tile, per entry: tile column, character -> the column's set of characters (atomicOr);
//   3. nodes per column = popcount, block scan -> node ids of the columns; per entry atomicMin of the
//      member index into its (column, character) slot: the order of first appearance in the family
//      (exact reference order) is the rank of that minimum among the column's characters -- one
//      thread per column sorts its handful of minima;
//   4. per entry: its node, its predecessor's node (the entry to its left, or what the member carried
//      over from earlier tiles); member count and raw edge count of the node by atomicAdd; the
//      predecessor as ONE BIT of a 64-bit word per node (bit d-1: the node d ids back -- ids ascend
//      with the column, so the set bits from the top down are the predecessors ascending and unique);
//      the few predecessors further back than 64 ids (long deletions) by rounds of atomicMin; the entries of
//      member 0 also leave their node in chain_rows -- the chain the DP wave's scout pass walks (mesh_dp.hip);
//   5. one thread per node writes record and predecessor list; atomicMin / atomicMax collect the
//      successor minimum column (for --insertion=forbid) and the last successor;
//   6. sinks and fence flags; LDS-slot / spill-row assignment for the DP kernel by liveness
//      (sequential over the rows: 16 lanes, a segment each) -- the other waves find the row skip's column maxima
//      meanwhile; predecessor entries, the finished record and the row skip's bound in one pass over the rows.  What
//      these steps change of a row is one LDS word until then (a DAG too large for that: in global memory).
// HBM traffic: the family's bases twice (bitmap, entries) and the DAG once.
// All arithmetic is integer except the node weight, which is looked up in a table the
// HOST computed with the reference's own mixed double/float expression.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "common.h"
#include "ctx.h"

namespace sina_hip {
namespace {

#ifndef SINA_GRAPH_THREADS
#define SINA_GRAPH_THREADS 512
#endif
#ifndef SINA_GRAPH_MINWAVES
#define SINA_GRAPH_MINWAVES 8  // (4 workgroups of 8 waves per CU: <= 64 VGPRs, 38.5 KB of LDS each for families of 40)
#endif
constexpr int kGT = SINA_GRAPH_THREADS;  // threads per workgroup (the phases are latency-bound: more loads in flight per LDS byte)
constexpr uint32_t kNoPrev = 0xFFFFu;
constexpr int kMaxFam = kFamilyMax;
#ifndef SINA_GRAPH_KTC
#define SINA_GRAPH_KTC 128  // (a multiple of 64: a wave takes 64 consecutive entry slots of one member)
#endif
#ifndef SINA_GRAPH_TNW
#define SINA_GRAPH_TNW 512  // nodes whose per-node words are in LDS at a time (a tile with more takes them in column-aligned windows)
#endif
constexpr int kTC = SINA_GRAPH_KTC;  // occupied columns per LDS tile (< 255: tile columns are bytes, 255 = none)
constexpr int kTNW = SINA_GRAPH_TNW;
static_assert(kTC % 64 == 0 && kTC < 255 && kTNW >= 32 && kTNW % 2 == 0, "tile geometry");
static_assert((kMaxFam * (kTC / 64) + SINA_GRAPH_THREADS / 64 - 1) / (SINA_GRAPH_THREADS / 64) <= 64, "far-entry flags of a wave fit 64 bits");

#ifdef SINA_DP_PROFILE
// profiling build (make PROFILE=1): per-phase s_memtime totals of thread 0, tools/perf_graph.py
__device__ unsigned long long g_graph_prof[16];
#define GP_DECL unsigned long long gp_[16] = {}; unsigned long long gt_ = __builtin_amdgcn_s_memtime();
#define GP(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); gp_[i] += t_ - gt_; gt_ = t_; }
#define GP_FLUSH if (threadIdx.x == 0) { for (int i_ = 0; i_ < 16; i_++) atomicAdd(&g_graph_prof[i_], gp_[i_]); }
#else
#define GP_DECL
#define GP(i)
#define GP_FLUSH
#endif

struct GraphArgs {
    const uint32_t *ref_ab;
    const uint64_t *ref_off;
    const uint32_t *fam_ids;   // concatenated
    const uint64_t *fam_off;   // [nq+1]
    const uint64_t *pred_off;  // [nq] offset of this query's pred area
    const float *wtab;         // [(kMaxFam+1) * (kMaxFam+1)]: weight for (F, count)
    uint4 *rec;                // [nq][ncap]
    uint32_t *node_pos;        // [nq][ncap]
    uint32_t *succ_min;        // [nq][ncap]
    uint32_t *far_mark;        // [nq][ncap] last successor row of every node (0: none)
    uint32_t *pred;            // per query area of total-family-bases entries
    uint2 *pred4;              // [nq][ncap] ids of every node's first four predecessors (step 8; common.h, pred4_pack)
    uint32_t *sizes;          // [nq][kBuiltWords]: N, raw edge entries, n_spill, status, first sink row, gmin, chain length (common.h, kBuiltN ...)
    uint16_t *chain_rows;      // [nq][ncap]: the node of every base of member 0, in base order (the DP wave's scout pass walks this chain)
    uint32_t width, ncap;
    uint32_t tile_bytes;       // LDS bytes of the tile tables (reused by the slot allocation) = bitmap_off
    uint32_t bitmap_off;       // LDS offset of the occupied-column bitmap (behind the tile tables)
    uint32_t member_off;       // LDS offset of the per-member records (behind the bitmap and its ranks)
    uint32_t member_cap;
    uint32_t fam_cap;          // rows of the entry table in LDS: the launch's largest family
    int W;                     // DP ring depth: edges longer than this need a spill row
    int want_smin;             // succ_min is read by somebody (--insertion=forbid, the debug entry): else it is not touched at all
    uint2 *reach;              // [nq][ncap] or nullptr: the DP kernel's row-skip bound (step 9; units: common.h): {R(m), last successor | C(m) << 16}
    float kappa64;             // ... 64 * 1.0001 * (largest match gain per unit of node weight)
};

// per family member, in LDS
struct Member {
    uint64_t beg;            // offset of its bases in the store
    uint32_t len;
    uint32_t cur, curn;      // first base at/after the tile, ... after it
    uint32_t carry, carryn;  // node of the last base before the tile, ... of the last base in it
    uint32_t id;
};
static_assert(sizeof(Member) == 32, "LDS layout");
// LDS offsets of the tables whose size is a compile-time constant
constexpr uint32_t kOCpos = 0;
constexpr uint32_t kONbase = kOCpos + 4 * kTC;
constexpr uint32_t kOPres = kONbase + 4 * (kTC + 2);
constexpr uint32_t kOWA = kOPres + 4 * kTC;
constexpr uint32_t kOWC = kOWA + 4 * kTNW;
constexpr uint32_t kOWD = kOWC + 4 * kTNW;
constexpr uint32_t kOWB = (kOWD + 4 * kTNW + 7) & ~7u;
constexpr uint32_t kOLi = kOWB + 8 * kTNW;
constexpr uint32_t kONn = kOLi + 32 * kTC;
constexpr uint32_t kONfar = kONn + kTC;
constexpr uint32_t kOMask = kONfar + kTNW;
constexpr uint32_t kONcol = kOMask + kTNW;
constexpr uint32_t kOE = (kONcol + kTNW + 15) & ~15u;
// A column's nodes are keyed by the base's CHARACTER (mseq.cpp:92-96), and masks 0 and 16 are both '.': where a column
// shows both, merge_dot16 gives the entries of mask 16 the key 0 and this bit, "mask 16"; the spare word behind nbaseT's
// kTC + 1 says that some column of the family so far was merged (reference stores hold no such bases)
constexpr int kELower0Bit = 14;
constexpr uint32_t kODot16 = kTC + 1;

// exclusive scan of in[0..n) into out[0..n) (may alias if same type); returns the total.
template <typename In, typename Out>
__device__ uint32_t block_exscan(const In *in, Out *out, uint32_t n, uint32_t *tmp) {
    const uint32_t tid = threadIdx.x;
    const uint32_t chunk = (n + kGT - 1) / kGT;
    const uint32_t b = min(n, tid * chunk), e = min(n, b + chunk);
    uint32_t s = 0;
    for (uint32_t i = b; i < e; i++) s += (uint32_t)in[i];
    // exclusive scan of the kGT partial sums (wave shuffle + 4 wave totals)
    uint32_t x = s;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) tmp[wave] = x;
    __syncthreads();
    uint32_t base = 0, total = 0;
    for (int w = 0; w < kGT / 64; w++) {
        if (w < wave) base += tmp[w];
        total += tmp[w];
    }
    uint32_t run = base + x - s;
    __syncthreads();
    for (uint32_t i = b; i < e; i++) {
        const uint32_t v = (uint32_t)in[i];
        out[i] = (Out)run;
        run += v;
    }
    __syncthreads();
    return total;
}

// the same with the input behind a function of the index
template <typename Get, typename Out>
__device__ uint32_t block_exscan_f(uint32_t n, Get get, Out *out, uint32_t *tmp) {
    const uint32_t tid = threadIdx.x;
    const uint32_t chunk = (n + kGT - 1) / kGT;
    const uint32_t b = min(n, tid * chunk), e = min(n, b + chunk);
    uint32_t s = 0;
    for (uint32_t i = b; i < e; i++) s += get(i);
    uint32_t x = s;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) tmp[wave] = x;
    __syncthreads();
    uint32_t base = 0, total = 0;
    for (int w = 0; w < kGT / 64; w++) {
        if (w < wave) base += tmp[w];
        total += tmp[w];
    }
    uint32_t run = base + x - s;
    __syncthreads();
    for (uint32_t i = b; i < e; i++) {
        const uint32_t v = get(i);
        out[i] = (Out)run;
        run += v;
    }
    __syncthreads();
    return total;
}

// inclusive scan of v[0..n) in place; returns the total.
__device__ uint32_t block_incscan(uint32_t *v, uint32_t n, uint32_t *tmp) {
    const uint32_t tid = threadIdx.x;
    const uint32_t chunk = (n + kGT - 1) / kGT;
    const uint32_t b = min(n, tid * chunk), e = min(n, b + chunk);
    uint32_t s = 0;
    for (uint32_t i = b; i < e; i++) s += v[i];
    uint32_t x = s;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) tmp[wave] = x;
    __syncthreads();
    uint32_t base = 0, total = 0;
    for (int w = 0; w < kGT / 64; w++) {
        if (w < wave) base += tmp[w];
        total += tmp[w];
    }
    uint32_t run = base + x - s;
    for (uint32_t i = b; i < e; i++) {  // (a thread's own stretch: nobody else reads or writes it before the barrier)
        run += v[i];
        v[i] = run;
    }
    __syncthreads();
    return total;
}

// A row's code in LDS, steps 6-8 of the DAGs whose rows fit the tile tables' space.  In front of step 7: the row's last
// successor | kCdSink | kCdFence; behind it: where the finished DP row is kept -- an LDS slot, or kCdSpilled | spill row
// (fewer than 65 536), or kCdNone (handed to the next row in registers) -- with the two flags still in place.
constexpr uint32_t kCdSpilled = 1u << 16, kCdNone = 1u << 17, kCdSink = 1u << 30, kCdFence = 1u << 31;
__device__ __forceinline__ uint32_t row_of_code(uint32_t c) {  // rec.w of a code
    return (c & kCdNone) ? kRowNone : (c & kCdSpilled) ? (kRowSpilled | (c & 0xFFFFu)) : (c & 0xFFFFu);
}

// Step 7 for one segment, the rows [b, e): get(m) is row m's code in front of the step, put(m, that, code) takes the code
// behind it (without the flags); K slots are searched, W of them exist.  Returns the segment's spill rows.
template <int K, typename Get, typename Put>
__device__ __forceinline__ uint32_t slot_walk(uint32_t b, uint32_t e, int W, Get get, Put put) {
    uint32_t fa[K];  // last successor of the row in slot x (0: empty)
#pragma unroll
    for (int x = 0; x < K; x++) fa[x] = (x < W) ? 0u : 0xFFFFFFFFu;
    uint32_t nsp = 0;
    for (uint32_t m = b; m < e; m++) {
        const uint32_t cd = get(m);
        const uint32_t l = cd & 0xFFFFu;
        uint32_t c = kCdNone;
        if (!(cd & kCdSink) && l != m + 1) {  // (a row only the next row reads is handed over in registers)
            // (a row with a successor beyond kFarLds, or in a later segment, is always a spill row)
            const bool may_slot = !(cd & kCdFence) && l < e;
            uint32_t slot = K;
#pragma unroll
            for (int x = K - 1; x >= 0; x--) slot = (may_slot && fa[x] <= m) ? (uint32_t)x : slot;
#pragma unroll
            for (int x = 0; x < K; x++) fa[x] = (slot == (uint32_t)x) ? l : fa[x];
            c = slot < (uint32_t)K ? slot : (kCdSpilled | nsp++);
        }
        put(m, cd, c);
    }
    return nsp;
}

// Step 2 of a tile as a function of its own: the kernel runs with 78 scalar registers at eight waves per SIMD and
// over a hundred live scalars -- inlined, this loop reloaded a dozen spilled ones per task; outlined, the caller's
// scalars are put aside once per tile.
__device__ __attribute__((noinline)) void fill_tile(const uint32_t *__restrict__ ref_ab, uint32_t bitmap_off, uint32_t member_off,
                                                    uint32_t nwords, uint32_t n_tasks, uint32_t c0, uint32_t tc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *cposT = reinterpret_cast<uint32_t *>(smem + kOCpos);
    uint32_t *presT = reinterpret_cast<uint32_t *>(smem + kOPres);
    uint16_t *eE = reinterpret_cast<uint16_t *>(smem + kOE);
    const uint32_t *bitmap = reinterpret_cast<const uint32_t *>(smem + bitmap_off);
    const uint16_t *wrank = reinterpret_cast<const uint16_t *>(bitmap + nwords);
    Member *mb = reinterpret_cast<Member *>(smem + member_off);
    constexpr uint32_t kEAbsent = 0x00FFu, kEFirst = 1u << 13;
    constexpr uint32_t kCH = kTC / 64, kNW = kGT / 64;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    auto rank = [&](uint32_t pos) -> uint32_t {
        return (uint32_t)wrank[pos >> 5] + __popc(bitmap[pos >> 5] & ((1u << (pos & 31)) - 1u));
    };
        // (latency-bound: eight tasks' loads are in flight per wave before the first is used)
        for (uint32_t t4 = wave; t4 < n_tasks; t4 += 8 * kNW) {
            uint32_t abv[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const uint32_t task = t4 + (uint32_t)u * kNW;
                abv[u] = 0xFFFFFFFFu;  // (no packed base looks like this: the mask byte has five bits)
                if (task < n_tasks) {
                    // (the member is the same for the whole wave: its cursor, length and offset on the scalar unit)
                    const uint32_t j = task / kCH;
                    const uint32_t cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)mb[j].cur);
                    const uint32_t len = (uint32_t)__builtin_amdgcn_readfirstlane((int)mb[j].len);
                    const uint64_t beg = mb[j].beg;
                    const uint64_t begs = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(beg >> 32)) << 32) |
                                          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)beg);
                    const uint32_t i = cur + (task % kCH) * 64u + lane;
                    if (i < len) abv[u] = ref_ab[begs + i];
                }
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const uint32_t task = t4 + (uint32_t)u * kNW;
                if (task >= n_tasks) continue;
                const uint32_t j = task / kCH, slot0 = (task % kCH) * 64u, slot = slot0 + lane;
                const uint32_t cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)mb[j].cur);
                uint32_t ev = kEAbsent;
                if (abv[u] != 0xFFFFFFFFu) {
                    const uint32_t ab = abv[u];
                    const uint32_t pos = ab & 0xFFFFFFu;
                    const uint32_t c = rank(pos) - c0;
                    if (c < tc) {
                        const uint32_t m = (ab >> 24) & 0x1Fu;
                        ev = c | (m << 8) | (cur + slot == 0 ? kEFirst : 0u);
                        atomicOr(&presT[c], 1u << m);
                        cposT[c] = pos;
                    }
                }
                eE[j * (uint32_t)kTC + slot] = (uint16_t)ev;
                // the member's last base in this tile moves its cursor (its bases in the tile are the first lanes of
                // its tasks)
                const uint32_t n_in = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(ev != kEAbsent));
                if (n_in && lane == 0) atomicMax(&mb[j].curn, cur + slot0 + n_in);
            }
        }
}

__device__ __forceinline__ uint32_t node_of_entry(uint32_t ev) {  // tile-local node of an entry: the column's first node + the place of its character
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t *nbaseT = reinterpret_cast<const uint32_t *>(smem + kONbase);
    const uint32_t *presT = reinterpret_cast<const uint32_t *>(smem + kOPres);
    const uint8_t *liOf = smem + kOLi;
    const uint32_t c = ev & 0xFFu, m = (ev >> 8) & 31u;
    const uint32_t b = nbaseT[c];
    return b + liOf[b + __popc(presT[c] & ((1u << m) - 1u))];
}
// The entries of mask 16 in the tile's merged columns (bit 16 of presT cleared while bit 0 is set) take the key 0.
__device__ __attribute__((noinline)) void merge_dot16(uint32_t n_tasks) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t *presT = reinterpret_cast<const uint32_t *>(smem + kOPres);
    uint16_t *eE = reinterpret_cast<uint16_t *>(smem + kOE);
    for (uint32_t e = threadIdx.x; e < n_tasks * 64u; e += kGT) {  // (entry e: member e / kTC, slot e % kTC)
        const uint32_t ev = eE[e];
        const uint32_t c = ev & 0xFFu;
        if (c != 0xFFu && ((ev >> 8) & 31u) == 16u && !(presT[c] & 0x10000u)) eE[e] = (uint16_t)((ev & ~(31u << 8)) | (1u << kELower0Bit));
    }
}
// A '.' node keeps the mask of its first member: 16, not 0, where that member shows it.  For the window of columns [ca, cb)
// whose first node is w0, after step 3 (wC: the first member of every node's character).  Outlined: reference stores hold no
// such base, and inlined the pass cost the kernel's hot loops registers.
__device__ __attribute__((noinline)) void fix_dot16(uint32_t n_tasks, uint32_t ca, uint32_t cb, uint32_t w0) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t *nbaseT = reinterpret_cast<const uint32_t *>(smem + kONbase);
    const uint32_t *wC = reinterpret_cast<const uint32_t *>(smem + kOWC);
    const uint16_t *eE = reinterpret_cast<const uint16_t *>(smem + kOE);
    uint8_t *maskN = smem + kOMask;
    for (uint32_t e = threadIdx.x; e < n_tasks * 64u; e += kGT) {  // (entry e: member e / kTC, slot e % kTC)
        const uint32_t ev = eE[e];
        const uint32_t c = ev & 0xFFu;
        // (an entry has no bit above kELower0Bit; '.' is the first of its column's characters)
        if (c >= ca && c < cb && (ev >> kELower0Bit) && wC[nbaseT[c] - w0] == e / (uint32_t)kTC) maskN[node_of_entry(ev) - w0] = 16;
    }
}
__global__ void __launch_bounds__(kGT) __attribute__((amdgpu_waves_per_eu(SINA_GRAPH_MINWAVES, SINA_GRAPH_MINWAVES))) family_graph_kernel(GraphArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_tmp[kGT / 64 + 8];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t nwords = (a.width + 31) / 32;
    const uint64_t f0 = a.fam_off[q];
    const uint32_t F = (uint32_t)(a.fam_off[q + 1] - f0);
    // LDS carve.  Everything whose size is known at compile time comes first: its addresses are immediates of the
    // LDS instructions, not scalars that have to stay live (the kernel runs with 100 SGPRs and spilled 109 more
    // when every table had a run-time base).
    uint32_t *cposT = reinterpret_cast<uint32_t *>(smem + kOCpos);          // [kTC] alignment column
    uint32_t *nbaseT = reinterpret_cast<uint32_t *>(smem + kONbase);        // [kTC + 2] first node of the column (tile-local); [tc] = nodes of the tile
    uint32_t *presT = reinterpret_cast<uint32_t *>(smem + kOPres);          // [kTC] the column's characters, bit m: mask value m occurs (where masks 0 and 16 meet, both '.', bit 0 stands for both)
    uint32_t *wA = reinterpret_cast<uint32_t *>(smem + kOWA);               // [kTNW] per node of the window: members | raw edges << 16
    uint32_t *wC = reinterpret_cast<uint32_t *>(smem + kOWC);               // [kTNW] first member of the node's character; then: smallest far predecessor not yet listed
    uint32_t *wD = reinterpret_cast<uint32_t *>(smem + kOWD);               // [kTNW] start of the CSR segment (raw entries before it in the window)
    unsigned long long *wB = reinterpret_cast<unsigned long long *>(smem + kOWB);  // [kTNW] predecessors at distance 1..64, a bit each
    uint8_t *liOf = smem + kOLi;                                            // [kTC * 32] by (column's first node + index of the character among the column's): place in family order
    uint8_t *nn = smem + kONn;                                              // [kTC] nodes per column
    uint8_t *nfarN = smem + kONfar;                                         // [kTNW] far predecessors listed so far
    uint8_t *maskN = smem + kOMask;                                         // [kTNW]
    uint8_t *ncolN = smem + kONcol;                                         // [kTNW] tile column of the node
    // entry (member j, slot): tile column | mask << 8 | "first base of the member" << 13 (merged columns: kELower0Bit above), kEAbsent (column 255): not in the tile
    uint16_t *eE = reinterpret_cast<uint16_t *>(smem + kOE);                // [fam_cap][kTC]
    // ... then what is sized by the launch: the occupied-column bitmap and its ranks, the family members
    uint32_t *bitmap = reinterpret_cast<uint32_t *>(smem + a.bitmap_off);   // [nwords]
    uint16_t *wrank = reinterpret_cast<uint16_t *>(bitmap + nwords);        // [nwords]
    Member *mb = reinterpret_cast<Member *>(smem + a.member_off);           // [member_cap >= 16: .id doubles as the slot allocator's per-segment counters]
    constexpr uint32_t kEFirst = 1u << 13;
    constexpr uint32_t kCH = kTC / 64, kNW = kGT / 64;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_tasks = F * kCH;  // (member, 64 slots) pairs, a wave each

    uint32_t *sz = a.sizes + kBuiltWords * (size_t)q;
    for (uint32_t j = tid; j < F; j += kGT) {
        const uint32_t id = a.fam_ids[f0 + j];
        mb[j].id = id;
        mb[j].beg = a.ref_off[id];
        mb[j].len = (uint32_t)(a.ref_off[id + 1] - a.ref_off[id]);
        mb[j].cur = mb[j].curn = 0;
        mb[j].carry = mb[j].carryn = kNoPrev;
    }
    for (uint32_t i = tid; i < nwords; i += kGT) bitmap[i] = 0;
    if (tid == 0) nbaseT[kODot16] = 0;
    __syncthreads();
    GP_DECL

    // 1. occupied columns
    // (latency-bound: eight members' loads are in flight per thread before the first is used)
    for (uint32_t j0 = 0; j0 < F; j0 += 8) {
        uint32_t maxlen = 0;
#pragma unroll
        for (int u = 0; u < 8; u++) maxlen = max(maxlen, j0 + u < F ? mb[j0 + u].len : 0u);
        for (uint32_t i = tid; i < maxlen; i += kGT) {
            uint32_t ab[8];
#pragma unroll
            for (int u = 0; u < 8; u++)
                ab[u] = (j0 + u < F && i < mb[j0 + u].len) ? a.ref_ab[mb[j0 + u].beg + i] : 0xFFFFFFFFu;
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (ab[u] != 0xFFFFFFFFu) {
                    const uint32_t pos = ab[u] & 0xFFFFFFu;
                    atomicOr(&bitmap[pos >> 5], 1u << (pos & 31));
                }
        }
    }
    __syncthreads();
    GP(0)
    // 2. dense column index: rank(pos) = wrank[pos >> 5] + popc(bits below)
    {
        const uint32_t chunk = (nwords + kGT - 1) / kGT;
        const uint32_t b = min(nwords, tid * chunk), e = min(nwords, b + chunk);
        uint32_t s = 0;
        for (uint32_t i = b; i < e; i++) s += __popc(bitmap[i]);
        uint32_t x = s;
        const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63) s_tmp[wave] = x;
        __syncthreads();
        uint32_t base = 0, total = 0;
        for (int w = 0; w < kGT / 64; w++) {
            if (w < wave) base += s_tmp[w];
            total += s_tmp[w];
        }
        uint32_t run = base + x - s;
        for (uint32_t i = b; i < e; i++) {
            wrank[i] = (uint16_t)run;
            run += __popc(bitmap[i]);
        }
        if (tid == 0) s_tmp[kGT / 64] = total;
    }
    __syncthreads();
    const uint32_t NC = s_tmp[kGT / 64];
    if (NC > 65535u) {  // (cannot be a valid DAG for the DP kernel anyway: more columns than row ids)
        if (tid == 0) {
            sz[kBuiltN] = NC;
            sz[kBuiltEdges] = sz[kBuiltSpill] = 0;
            sz[kBuiltStatus] = kBuiltNodeCap;
        }
        return;
    }
    auto rank = [&](uint32_t pos) -> uint32_t {
        return (uint32_t)wrank[pos >> 5] + __popc(bitmap[pos >> 5] & ((1u << (pos & 31)) - 1u));
    };
    uint4 *rec = a.rec + (size_t)q * a.ncap;
    uint32_t *node_pos = a.node_pos + (size_t)q * a.ncap;
    uint32_t *smin = a.succ_min + (size_t)q * a.ncap;
    uint32_t *last = a.far_mark + (size_t)q * a.ncap;
    uint32_t *pred = a.pred + a.pred_off[q];
    uint16_t *chain_rows = a.chain_rows + (size_t)q * a.ncap;
    // (smin / last of a node are initialised by the tile that creates it, right before the first successor can
    // touch them: clearing all ncap entries up front wrote four times what a 16S DAG uses)
    const float *wt = a.wtab + (size_t)F * (kMaxFam + 1);
    uint32_t N = 0, E = 0;  // running totals (uniform)
    GP(1)

    for (uint32_t c0 = 0; c0 < NC; c0 += kTC) {
        const uint32_t tc = min((uint32_t)kTC, NC - c0);
        for (uint32_t i = tid; i < (uint32_t)kTC; i += kGT) presT[i] = 0;
        __syncthreads();
        GP(2)
        // 2. the entries of this tile: member j's bases cur[j].. as long as their column is in the tile (a
        // contiguous stretch of at most kTC bases)
        fill_tile(a.ref_ab, a.bitmap_off, a.member_off, nwords, n_tasks, c0, tc);
        __syncthreads();
        for (uint32_t c = tid; c < tc; c += kGT) {
            uint32_t p = presT[c];
            if ((p & 0x10001u) == 0x10001u) {  // masks 0 and 16 in one column: one character, one node
                p &= ~0x10000u;
                presT[c] = p;
                nbaseT[kODot16] = 1u;
            }
            nn[c] = (uint8_t)__popc(p);
        }
        __syncthreads();
        if (nbaseT[kODot16]) {  // (uniform, rare)
            merge_dot16(n_tasks);
            __syncthreads();
        }
        GP(3)
        const uint32_t tn = block_exscan(nn, nbaseT, tc, s_tmp);
        if (tid == 0) nbaseT[tc] = tn;
        for (uint32_t ln = tid; ln < tn; ln += kGT)  // this tile's nodes: no successor seen yet
            if (N + ln < a.ncap) {
                last[N + ln] = 0;
                if (a.want_smin) smin[N + ln] = 0xFFFFFFFFu;
            }
        __syncthreads();
        GP(5)
        uint32_t te = 0;  // raw edge entries of the tile's windows so far
        for (uint32_t ca = 0; ca < tc;) {
            // the window: columns [ca, cb) -- as many as have their nodes' words in LDS together (nearly always the tile)
            const uint32_t w0 = nbaseT[ca];
            uint32_t cb = tc;
            if (tn - w0 > (uint32_t)kTNW) {
                uint32_t lo = ca + 1, hi = tc;  // (a column has at most 32 nodes: one always fits)
                while (lo < hi) {
                    const uint32_t mid = (lo + hi + 1) / 2;
                    if (nbaseT[mid] - w0 <= (uint32_t)kTNW) lo = mid;
                    else hi = mid - 1;
                }
                cb = lo;
            }
            const uint32_t wn = nbaseT[cb] - w0;
            for (uint32_t i = tid; i < wn; i += kGT) {
                wA[i] = 0;
                wB[i] = 0;
                wC[i] = 0xFFFFFFFFu;  // (first the smallest member index of the node's character, then the far predecessors)
                nfarN[i] = 0;
            }
            __syncthreads();
            // 3. first appearance of every (column, character) in family order
            for (uint32_t task = wave; task < n_tasks; task += kNW) {
                const uint32_t j = task / kCH, slot = (task % kCH) * 64u + lane;
                const uint32_t ev = eE[j * (uint32_t)kTC + slot];
                const uint32_t c = ev & 0xFFu;
                if (c >= ca && c < cb) {
                    const uint32_t m = (ev >> 8) & 31u;
                    atomicMin(&wC[nbaseT[c] + __popc(presT[c] & ((1u << m) - 1u)) - w0], j);
                }
            }
            __syncthreads();
            for (uint32_t c = ca + tid; c < cb; c += kGT) {
                const uint32_t base = nbaseT[c], k = nn[c];
                uint32_t pp = presT[c];
                for (uint32_t x = 0; x < k; x++) {
                    const uint32_t mj = wC[base - w0 + x];
                    uint32_t r = 0;
                    for (uint32_t y = 0; y < k; y++) r += (wC[base - w0 + y] < mj) ? 1u : 0u;
                    liOf[base + x] = (uint8_t)r;
                    maskN[base - w0 + r] = (uint8_t)(__ffs(pp) - 1);
                    ncolN[base - w0 + r] = (uint8_t)c;
                    pp &= pp - 1u;
                }
            }
            __syncthreads();
            if (nbaseT[kODot16]) {  // (uniform, rare) some member shows mask 16
                fix_dot16(n_tasks, ca, cb, w0);
                __syncthreads();
            }
            GP(4)
            // 4. members and raw edges per node; the predecessor of every entry.  An entry's node: the column's first
            // node + the place of its character (liOf is complete for this window and the ones before: the entry to
            // the left is in one of them)
            auto node_of = [&](uint32_t ev) -> uint32_t { return node_of_entry(ev); };
            unsigned long long farbits = 0;  // my entries (by round of the task loop) whose predecessor is more than 64 ids back
            {
                uint32_t it = 0;
                for (uint32_t task = wave; task < n_tasks; task += kNW, it++) {
                    const uint32_t j = task / kCH, slot = (task % kCH) * 64u + lane;
                    const uint32_t ev = eE[j * (uint32_t)kTC + slot];
                    const uint32_t c = ev & 0xFFu;
                    const bool mine = c >= ca && c < cb;
                    const uint32_t ln = mine ? node_of(ev) : 0u;
                    // (the entry to the left is the lane to the left, except for the first slot of a task)
                    uint32_t lnp = __shfl_up(ln, 1);
                    const bool left_mine = __shfl_up(mine ? 1 : 0, 1) != 0;
                    if (!mine) continue;
                    const uint32_t node = N + ln;
                    const bool first = (ev & kEFirst) != 0;
                    atomicAdd(&wA[ln - w0], first ? 1u : 0x10001u);
                    if (mb[j].cur + slot + 1 == mb[j].curn) mb[j].carryn = node;
                    // (member 0's chain: entry `slot` of the tile is its base cur + slot; a member has at most one base
                    // per column, so the index stays below the node count -- and below ncap unless the build overflows)
                    if (j == 0 && mb[0].cur + slot < a.ncap) chain_rows[mb[0].cur + slot] = (uint16_t)node;
                    if (!first) {
                        if (slot && (lane == 0 || !left_mine)) lnp = node_of(eE[j * (uint32_t)kTC + slot - 1]);
                        const uint32_t pn = slot ? N + lnp : mb[j].carry;
                        const uint32_t d = node - pn;
                        if (d <= 64u) atomicOr(&wB[ln - w0], 1ull << (d - 1u));
                        else farbits |= 1ull << it;
                    }
                }
            }
            for (uint32_t i = tid; i < wn; i += kGT) wC[i] = 0xFFFFFFFFu;  // (the first members have been read: barrier above)
            __syncthreads();
            GP(6)
            const uint32_t te_w = block_exscan_f(wn, [&](uint32_t i) { return wA[i] >> 16; }, wD, s_tmp);
            // far predecessors, smallest first: every round lists one per node
            while (__syncthreads_or(farbits != 0 ? 1 : 0)) {
                uint32_t it = 0;
                for (uint32_t task = wave; task < n_tasks; task += kNW, it++) {
                    if (!((farbits >> it) & 1ull)) continue;
                    const uint32_t j = task / kCH, slot = (task % kCH) * 64u + lane;
                    const uint32_t ln = node_of(eE[j * (uint32_t)kTC + slot]);
                    const uint32_t pn = slot ? N + node_of(eE[j * (uint32_t)kTC + slot - 1]) : mb[j].carry;
                    atomicMin(&wC[ln - w0], pn);
                }
                __syncthreads();
                it = 0;
                for (uint32_t task = wave; task < n_tasks; task += kNW, it++) {
                    if (!((farbits >> it) & 1ull)) continue;
                    const uint32_t j = task / kCH, slot = (task % kCH) * 64u + lane;
                    const uint32_t ln = node_of(eE[j * (uint32_t)kTC + slot]);
                    const uint32_t pn = slot ? N + node_of(eE[j * (uint32_t)kTC + slot - 1]) : mb[j].carry;
                    if (wC[ln - w0] == pn) farbits &= ~(1ull << it);
                }
                __syncthreads();
                for (uint32_t i = tid; i < wn; i += kGT) {
                    const uint32_t v = wC[i];
                    if (v == 0xFFFFFFFFu) continue;
                    const uint32_t node = N + w0 + i;
                    if (node < a.ncap) {
                        pred[E + te + wD[i] + nfarN[i]] = v;
                        if (a.want_smin) atomicMin(&smin[v], cposT[ncolN[i]]);
                        atomicMax(&last[v], node);
                    }
                    nfarN[i]++;
                    wC[i] = 0xFFFFFFFFu;
                }
            }
            // 5. node records + predecessor lists: the far ones are in place, the near ones are the set bits from the top down
            for (uint32_t i = tid; i < wn; i += kGT) {
                const uint32_t node = N + w0 + i;
                if (node >= a.ncap) continue;
                const uint32_t seg = E + te + wD[i];
                const uint32_t pos = cposT[ncolN[i]];
                uint32_t np = nfarN[i];
                unsigned long long bits = wB[i];
                while (bits) {
                    const uint32_t hi = 63u - (uint32_t)__clzll((long long)bits);
                    bits ^= 1ull << hi;
                    const uint32_t pa = node - (hi + 1u);
                    pred[seg + np] = pa;
                    np++;
                    if (a.want_smin) atomicMin(&smin[pa], pos);
                    atomicMax(&last[pa], node);
                }
                uint4 r;
                r.x = seg;
                r.y = __float_as_uint(wt[wA[i] & 0xFFFFu]);
                r.z = (np & 0xFFu) | ((uint32_t)maskN[i] << 8);
                r.w = kRowNone;
                rec[node] = r;
                node_pos[node] = pos;
            }
            te += te_w;
            ca = cb;
            __syncthreads();  // (the window's words are cleared for the next one)
        }
        for (uint32_t j = tid; j < F; j += kGT) {
            mb[j].cur = mb[j].curn;
            mb[j].carry = mb[j].carryn;
        }
        N += tn;
        E += te;
        __syncthreads();
        GP(7)
    }
    if (N > a.ncap || N > 65535u) {
        if (tid == 0) {
            sz[kBuiltN] = N;
            sz[kBuiltEdges] = sz[kBuiltSpill] = 0;
            sz[kBuiltStatus] = kBuiltNodeCap;
        }
        return;
    }
    GP(8)
    // 6. sinks, successor minimum, fence flag.  Where the rows' words fit the tile tables' space (in_lds: a 16S DAG
    // does) steps 6-8 keep what they change of a row in ONE LDS word, the row's code (kCd...), and step 8 stores the
    // finished record: rec is written whole by the tile loop and whole by step 8, not a word at a time by every step
    // in between.  Where they do not fit, the steps work on rec / last in global memory.
    const uint32_t seg_len = dp_slot_segment(N);
    const uint32_t n_seg = (N + seg_len - 1) / seg_len;
    uint32_t *codeL = reinterpret_cast<uint32_t *>(smem);  // (the tile tables' space: everything in front of the bitmap)
    const bool in_lds = (size_t)N * 4 <= a.tile_bytes;
    // ... and where a second word per row fits behind the codes, step 9's column maxima are found there BESIDE step 7's
    // walk (which is one wave's work), not behind it
    const bool beside = a.reach != nullptr && (size_t)N * 8 <= a.tile_bytes;
    uint32_t *cwL = codeL + N;
    constexpr int kSFirstSink = kGT / 64 + 1, kSGmin = kGT / 64 + 2, kSSpill = kGT / 64 + 3;  // (s_tmp)
    if (tid == 0) {
        s_tmp[kSFirstSink] = 0xFFFFFFFFu;  // first sink row
        s_tmp[kSGmin] = 0xFFFFFFFFu;       // smallest column maximum (step 9)
    }
    __syncthreads();
    for (uint32_t i = tid; i < N; i += kGT) {
        const uint32_t l = last[i];
        uint32_t cd = l;
        if (l == 0) {  // (a successor's id is greater than its predecessor's: never 0)
            cd |= kCdSink;
            atomicMin(&s_tmp[kSFirstSink], i);
            if (a.want_smin) smin[i] = 1000000u;  // "no successor" sentinel of mesh.h:480
        }
        if (l > i && l - i > (uint32_t)kFarLds) cd |= kCdFence;
        if (in_lds) codeL[i] = cd;
        else if (cd & (kCdSink | kCdFence)) rec[i].z |= ((cd & kCdSink) ? kRecSink : 0u) | ((cd & kCdFence) ? kRecFence : 0u);
    }
    // step 9's column maxima: the nodes of a column have consecutive ids, the thread of a column's FIRST node finds the
    // column's maximum and leaves it at that node, 0 at the column's others
    auto column_maxima = [&](uint32_t *cw, uint32_t first, uint32_t step) {
        for (uint32_t i = first; i < N; i += step) {
            const uint32_t pos = node_pos[i];
            if (i > 0 && node_pos[i - 1] == pos) continue;
            uint32_t mx = 0;
            for (uint32_t j = i; j < N && node_pos[j] == pos; j++) {
                mx = max(mx, prune_gain_units(__uint_as_float(rec[j].y), a.kappa64));
                cw[j] = 0;
            }
            cw[i] = mx;
            atomicMin(&s_tmp[kSGmin], mx);
        }
    };
    __syncthreads();
    GP(9)
    // 7. where every finished DP row is kept for its successors: LDS slots by liveness (first slot
    // whose row has seen its last successor), otherwise a spill row.  The greedy is sequential over
    // the rows, so the rows are cut into up to 16 segments that are allocated independently, one LANE
    // per segment: a row whose last successor lies in a later segment is kept in a spill row (three
    // or so per boundary), every segment starts with all slots free.  Spill rows are numbered in row
    // order (per-segment counts, prefix sum).  tests/util.py row_store_model states the same rule.
    // (the lanes walk their segments row by row: from LDS when the rows fit the tile tables' space --
    // a dependent global load per row was most of this step's time)
    if (wave == 0) {
        uint32_t nsp = 0;
        if (tid < n_seg) {
            const uint32_t b = tid * seg_len, e = min(N, b + seg_len);
            // (the walk is one dependent chain per lane in a CU that runs 31 other waves: every instruction waits its turn,
            // so the slot search is compiled for 4 slots -- the DP kernels keep 3 -- and for 8)
            auto walk = [&](auto kslots) {
                constexpr int K = decltype(kslots)::value;
                if (in_lds)
                    return slot_walk<K>(b, e, a.W, [&](uint32_t m) { return codeL[m]; },
                                        [&](uint32_t m, uint32_t cd, uint32_t c) { codeL[m] = (cd & (kCdSink | kCdFence)) | c; });
                return slot_walk<K>(b, e, a.W,
                                    [&](uint32_t m) {
                                        const uint32_t z = rec[m].z;
                                        return last[m] | ((z & kRecSink) ? kCdSink : 0u) | ((z & kRecFence) ? kCdFence : 0u);
                                    },
                                    [&](uint32_t m, uint32_t, uint32_t c) { rec[m].w = row_of_code(c); });
            };
            nsp = (a.W <= 4) ? walk(std::integral_constant<int, 4>()) : walk(std::integral_constant<int, 8>());
        }
        // the segments' first spill rows: a prefix sum over the (at most 16) lanes that walked; s_ids is free by now
        uint32_t x = nsp;
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const uint32_t y = __shfl_up(x, off);
            if (lane >= (uint32_t)off) x += y;
        }
        if (tid < n_seg) mb[tid].id = x - nsp;
        if (tid == 15) s_tmp[kSSpill] = x;
    } else if (beside) {
        column_maxima(cwL, tid - 64u, (uint32_t)kGT - 64u);
    }
    __syncthreads();
    const uint32_t tot = s_tmp[kSSpill];
    if (tid == 0) {
        sz[kBuiltN] = N;
        sz[kBuiltEdges] = E;
        sz[kBuiltSpill] = tot;
        sz[kBuiltStatus] = (tot > kMaxSpillRows) ? kBuiltSpillCap : 0u;
        sz[kBuiltFirstSink] = s_tmp[kSFirstSink];
        sz[kBuiltChainLen] = mb[0].len;
        if (beside) sz[kBuiltGmin] = s_tmp[kSGmin];
    }
    uint2 *pred4 = a.pred4 + (size_t)q * a.ncap;
    uint2 *rg = a.reach + (size_t)q * a.ncap;  // (used where a.reach is not null)
    if (in_lds) {
        // spill rows get their final numbers: segment base + number within the segment
        for (uint32_t i = tid; i < N; i += kGT) {
            const uint32_t c = codeL[i];
            if (c & kCdSpilled) codeL[i] = c + mb[i / seg_len].id;  // (fewer than 65 536 rows: no carry out of the number)
        }
        // (the scan's first barrier is also the one behind the numbering)
        uint32_t total = 0;
        if (beside) total = block_incscan(cwL, N, s_tmp);
        else __syncthreads();
        GP(10)
        // 8. predecessor entries for the DP kernel: id | (LDS slot or spill row) << 16 | spilled << 31; the first four
        // ids once more, by row, for the trace-back walk (pred4: N <= ncap here); the row's finished record; and, where
        // the column maxima are in (beside), step 9's bound of the row
        for (uint32_t i = tid; i < N; i += kGT) {
            const uint4 r = rec[i];
            const uint32_t cd = codeL[i];
            const uint32_t np = r.z & 0xFFu;
            uint32_t first_far = 0;
            uint32_t dist = np ? 0u : kRecDistFar;  // (ids ascend: the first predecessor is the furthest)
            uint32_t p4[4] = {0u, 0u, 0u, 0u};
            for (uint32_t x = 0; x < np; x++) {
                const uint32_t pa = pred[r.x + x];
                const uint32_t pc = codeL[pa];
                const bool sp = (pc & kCdSpilled) != 0;  // (kCdNone, kept in registers for this row: the number is 0, the entry's slot is not read)
                if (sp && first_far == 0) first_far = x + 1;
                dist = max(dist, i - pa);
                pred[r.x + x] = pa | ((pc & 0x7FFFu) << 16) | (sp ? kPredSpilled : 0u);
                if (x == 0) p4[0] = pa;
                else if (x == 1) p4[1] = pa;
                else if (x == 2) p4[2] = pa;
                else if (x == 3) p4[3] = pa;
            }
            uint4 o;
            o.x = r.x;
            o.y = r.y;
            o.z = r.z | ((cd & kCdSink) ? kRecSink : 0u) | ((cd & kCdFence) ? kRecFence : 0u) | (first_far << 24) |
                  (min(dist, kRecDistFar) << kRecDistShift);
            o.w = row_of_code(cd);
            rec[i] = o;
            pred4[i] = pred4_pack(p4[0], p4[1], p4[2], p4[3]);
            if (beside) rg[i] = uint2{total - cwL[i], last[i] | ((NC - 1u - rank(node_pos[i])) << 16)};
        }
        GP(11)
        // 9. the DP kernel's row-skip bound (common.h "the bound", mesh_dp.hip PRUNE): R(m) = what a path can still gain
        // right of node m's column = the sum, over the occupied columns right of it, of the column's best node's gain
        // (an edge always leads to a column further right, a path takes at most one node per column).  Integer units:
        // the sums are exact and do not depend on the order of the scan.  An INCLUSIVE scan of "maximum at the column's
        // first node, 0 at its others" gives every node of a column the total up to and including its column.
        // (here for the DAGs whose codes fit the tile tables' space but not the maxima beside them: step 8 was the last
        // reader of the codes)
        if (a.reach != nullptr && !beside) {
            __syncthreads();
            column_maxima(codeL, tid, (uint32_t)kGT);
            __syncthreads();
            if (tid == 0) sz[kBuiltGmin] = s_tmp[kSGmin];
            total = block_incscan(codeL, N, s_tmp);
            for (uint32_t i = tid; i < N; i += kGT)
                rg[i] = uint2{total - codeL[i], last[i] | ((NC - 1u - rank(node_pos[i])) << 16)};
        }
        GP(12)
    } else {
        for (uint32_t i = tid; i < N; i += kGT) {
            const uint32_t w = rec[i].w;
            if (w != kRowNone && (w & kRowSpilled)) rec[i].w = w + mb[i / seg_len].id;
        }
        __syncthreads();
        GP(10)
        // 8. as above, a predecessor's row from its record
        for (uint32_t i = tid; i < N; i += kGT) {
            const uint4 r = rec[i];
            const uint32_t np = r.z & 0xFFu;
            uint32_t first_far = 0;
            uint32_t dist = np ? 0u : kRecDistFar;
            uint32_t p4[4] = {0u, 0u, 0u, 0u};
            for (uint32_t x = 0; x < np; x++) {
                const uint32_t pa = pred[r.x + x];
                uint32_t pw = rec[pa].w;
                if (pw == kRowNone) pw = 0;  // (kept in registers for this row: the entry's slot is not read)
                const bool sp = (pw & kRowSpilled) != 0;
                if (sp && first_far == 0) first_far = x + 1;
                dist = max(dist, i - pa);
                pred[r.x + x] = pa | ((pw & 0x7FFFu) << 16) | (sp ? kPredSpilled : 0u);
                if (x == 0) p4[0] = pa;
                else if (x == 1) p4[1] = pa;
                else if (x == 2) p4[2] = pa;
                else if (x == 3) p4[3] = pa;
            }
            rec[i].z = r.z | (first_far << 24) | (min(dist, kRecDistFar) << kRecDistShift);
            pred4[i] = pred4_pack(p4[0], p4[1], p4[2], p4[3]);
        }
        GP(11)
        // 9. as above, with an exclusive scan and the thread of a column's first node storing the column's bounds
        if (a.reach != nullptr) {
            // (scratch: nobody reads succ_min in a launch that skips rows -- want_smin is --insertion=forbid; the debug
            // entry wants both and gets the last successors overwritten instead)
            uint32_t *cw = a.want_smin ? last : smin;
            column_maxima(cw, tid, (uint32_t)kGT);
            __syncthreads();
            if (tid == 0) sz[kBuiltGmin] = s_tmp[kSGmin];
            const uint32_t total = block_exscan(cw, cw, N, s_tmp);
            for (uint32_t i = tid; i < N; i += kGT) {
                const uint32_t pos = node_pos[i];
                if (i > 0 && node_pos[i - 1] == pos) continue;
                const uint32_t right = (i + 1 < N) ? total - cw[i + 1] : 0u;  // (cw[i + 1] = columns up to and including mine)
                const uint32_t cols_right = NC - 1u - rank(pos);                 // (the dense column index of step 2)
                for (uint32_t j = i; j < N && node_pos[j] == pos; j++) rg[j] = uint2{right, (a.want_smin ? 0u : last[j]) | (cols_right << 16)};
            }
        }
        GP(12)
    }
    GP_FLUSH
}

// LDS of one workgroup: the tile tables, the bitmap + ranks (offset: graph_bitmap_off), the member records behind them
size_t graph_bitmap_off(uint32_t max_family) { return ((size_t)kOE + 2 * (size_t)max_family * kTC + 15) & ~(size_t)15; }
size_t graph_lds_bytes(uint32_t width, uint32_t max_family) {
    const size_t nwords = (width + 31) / 32;
    return graph_bitmap_off(max_family) + ((6 * nwords + 15) & ~(size_t)15);
}
size_t graph_member_cap(uint32_t max_family) { return std::max<size_t>(16, (max_family + 1) & ~(size_t)1); }
size_t graph_lds_total(uint32_t width, uint32_t max_family) {
    return graph_lds_bytes(width, max_family) + sizeof(Member) * graph_member_cap(max_family);
}

}  // namespace
}  // namespace sina_hip

using namespace sina_hip;

namespace {

// Builds the DAGs of bq families (fam_off is absolute, first family = q0) into the context's
// rec / node_pos / succ_minpos / pred buffers; grows the per-query caps and retries on overflow.
int build_family_graphs(sina_hip_ctx *c, const uint32_t *fam_ids, const uint64_t *fam_off, uint32_t q0,
                        uint32_t bq, float fs_weight, int W, BuiltGraphs *bg, bool want_smin, float kappa64, bool for_dp) {
    hipStream_t s = c->stream;
    if (ensure_ref_off_host(c)) return 1;  // (a store that arrived by broadcast reads it back once)
    std::vector<uint64_t> foff(bq + 1), elems(bq, 0);
    uint32_t max_f = 1;
    bg->pred_off.assign(bq, 0);
    for (uint32_t q = 0; q <= bq; q++) foff[q] = fam_off[q0 + q] - fam_off[q0];
    for (uint32_t q = 0; q < bq; q++) {
        max_f = std::max<uint32_t>(max_f, (uint32_t)(foff[q + 1] - foff[q]));
        for (uint64_t x = fam_off[q0 + q]; x < fam_off[q0 + q + 1]; x++) {
            const uint32_t id = fam_ids[x];
            if (id >= c->st->n_refs) SH_FAIL("align_families: reference id out of range");
            elems[q] += c->st->ref_off_host[id + 1] - c->st->ref_off_host[id];
        }
        // (no base, no node: the DP wave would start its end-cell search at a row that does not exist -- refused here,
        // before anything is copied or launched, like an empty graph handed to sina_hip_align_graphs; the debug entries,
        // which align nothing, show the DAG of no node)
        if (for_dp && elems[q] == 0) SH_FAIL("align_families: a family without a single base");
    }
    // weight table: the reference's expression (mseq.cpp:113) evaluated on the host
    if (!(c->wtab_fs_weight == fs_weight) || !c->g_wtab.p) {
        std::vector<float> wt((size_t)(kMaxFam + 1) * (kMaxFam + 1), 0.f);
        const float weight = fs_weight;
        for (unsigned F = 1; F <= (unsigned)kMaxFam; F++)
            for (unsigned cnt = 0; cnt <= F; cnt++)
                wt[(size_t)F * (kMaxFam + 1) + cnt] =
                    (float)(1.0 / (double)(weight + 1) + (double)(weight * ((float)cnt / (float)F)));
        if (c->g_wtab.reserve(wt.size() * 4)) return 1;
        SH_CHECK(hipMemcpyAsync(c->g_wtab.p, wt.data(), wt.size() * 4, hipMemcpyHostToDevice, s));
        SH_CHECK(hipStreamSynchronize(s));
        c->wtab_fs_weight = fs_weight;
    }
    uint32_t ncap = std::min<uint32_t>(65535, 12288);
    for (int attempt = 0;; attempt++) {
        uint64_t pred_total = 0;
        for (uint32_t q = 0; q < bq; q++) {
            bg->pred_off[q] = pred_total;
            pred_total += elems[q] + 8;  // +8: slack behind every list
        }
        const size_t glds_tables = graph_lds_bytes(c->st->width, max_f);
        const size_t glds = graph_lds_total(c->st->width, max_f);
        if (glds > 160 * 1024) SH_FAIL_LIMIT("align_families: family too wide for the device DAG build");
        if (c->g_fam_ids.reserve(4 * std::max<uint64_t>(foff[bq], 1)) || c->g_fam_off.reserve(8 * ((uint64_t)bq + 1)) ||
            c->g_tmp1.reserve(8 * (uint64_t)bq) ||
            c->rec.reserve(sizeof(uint4) * (uint64_t)bq * ncap) || c->node_pos.reserve(4 * (uint64_t)bq * ncap) ||
            c->succ_minpos.reserve(4 * (uint64_t)bq * ncap) || c->g_tmp3.reserve(4 * (uint64_t)bq * ncap) ||
            c->pred.reserve(4 * pred_total) || c->pred4.reserve(sizeof(uint2) * (uint64_t)bq * ncap) || c->g_sizes.reserve(4 * kBuiltWords * (uint64_t)bq) ||
            c->scout.reserve(2 * (uint64_t)bq * ncap) ||
            (kappa64 > 0.f && c->rgain.reserve(8 * (uint64_t)bq * ncap)))
            return 1;
        if (upload(c, 1, c->g_fam_ids.p, fam_ids + fam_off[q0], 4 * foff[bq], s) ||
            upload(c, 2, c->g_fam_off.p, foff.data(), 8 * ((uint64_t)bq + 1), s) ||
            upload(c, 3, c->g_tmp1.p, bg->pred_off.data(), 8 * (uint64_t)bq, s))
            return 1;
        GraphArgs ga;
        ga.ref_ab = c->st->ref_ab.as<uint32_t>();
        ga.ref_off = c->st->ref_off.as<uint64_t>();
        ga.fam_ids = c->g_fam_ids.as<uint32_t>();
        ga.fam_off = c->g_fam_off.as<uint64_t>();
        ga.pred_off = c->g_tmp1.as<uint64_t>();
        ga.wtab = c->g_wtab.as<float>();
        ga.rec = c->rec.as<uint4>();
        ga.node_pos = c->node_pos.as<uint32_t>();
        ga.succ_min = c->succ_minpos.as<uint32_t>();
        ga.far_mark = c->g_tmp3.as<uint32_t>();
        ga.pred = c->pred.as<uint32_t>();
        ga.pred4 = c->pred4.as<uint2>();
        ga.sizes = c->g_sizes.as<uint32_t>();
        ga.chain_rows = c->scout.as<uint16_t>();
        ga.width = c->st->width;
        ga.ncap = ncap;
        ga.bitmap_off = (uint32_t)graph_bitmap_off(max_f);
        ga.tile_bytes = ga.bitmap_off;
        ga.member_off = (uint32_t)glds_tables;
        ga.member_cap = (uint32_t)graph_member_cap(max_f);
        ga.fam_cap = max_f;
        ga.W = W;
        ga.want_smin = want_smin ? 1 : 0;
        ga.reach = kappa64 > 0.f ? c->rgain.as<uint2>() : nullptr;
        ga.kappa64 = kappa64;
        if (allow_full_lds(reinterpret_cast<const void *>(family_graph_kernel))) return 1;
        bg->sizes.resize(kBuiltWords * (size_t)bq);
        {
            heavy_launch hl(c, s, kHeavyGraph);  // (a device-filling kernel: ctx.h)
            SH_CHECK(hipEventRecord(c->ev[6], hl.stream()));
            // The launch behind a DAG build waits for its END: the build's own drain is a millisecond, and a DP launch
            // that starts in it begins with a stagger it carries to its own end (measured: 142.1 k sequences/s with
            // the signal, 143.1 k without, DP 49.5 against 48.3 ms per launch; profiles/r04_chain_ab.txt).
            hipLaunchKernelGGL(family_graph_kernel, dim3(bq), dim3(kGT), glds, hl.stream(), ga);
            SH_CHECK(hipGetLastError());
            SH_CHECK(hipEventRecord(c->ev[7], hl.stream()));
            if (hl.done()) return 1;
        }
        if (download(c, 4, c->g_sizes.p, 4 * kBuiltWords * (uint64_t)bq, s)) return 1;
        SH_CHECK(wait_stream(c, s));
        memcpy(bg->sizes.data(), c->h_stage[4].p, 4 * kBuiltWords * (uint64_t)bq);
        float gms = 0;
        SH_CHECK(hipEventElapsedTime(&gms, c->ev[6], c->ev[7]));
        {
            uint64_t bytes = 0;  // algorithmic: the families' bases in, the DAGs out
            for (uint32_t q = 0; q < bq; q++)
                bytes += 4 * elems[q] + (uint64_t)bg->sizes[kBuiltWords * q + kBuiltN] * (16 + 4 + 8 + (kappa64 > 0.f ? 8 : 0)) +
                         4 * (uint64_t)bg->sizes[kBuiltWords * q + kBuiltEdges];
            std::lock_guard<std::mutex> slk(c->st->stats_mu);
            c->st->stats.graph_ms += gms;
            c->st->stats.graph_bytes += bytes;
            c->st->stats.graph_launches++;
        }
        uint32_t need_n = 0;
        for (uint32_t q = 0; q < bq; q++) {
            const uint32_t status = bg->sizes[kBuiltWords * q + kBuiltStatus];
            if (status == kBuiltNodeCap) need_n = std::max(need_n, bg->sizes[kBuiltWords * q + kBuiltN]);
            if (status == kBuiltSpillCap) SH_FAIL_LIMIT("align_families: too many spill rows for one query");
        }
        if (!need_n) break;
        if (attempt >= 3 || need_n > 65535u) SH_FAIL_LIMIT("align_families: family DAG exceeds device limits");
        ncap = std::min<uint32_t>(65535, need_n + need_n / 8 + 16);
    }
    bg->ncap = ncap;
    return 0;
}

// the DAG builder behind sina_hip_align_families
int build_graphs_for_launch(sina_hip_ctx *c, const uint32_t *fam_ids, const uint64_t *fam_off, uint32_t q0, uint32_t n,
                            const sina_hip_align_params *p, int W, const PrunePlan &pp, BuiltGraphs *bg) {
    return build_family_graphs(c, fam_ids, fam_off, q0, n, p->fs_weight, W, bg, p->insertion == SINA_INSERTION_FORBID,
                               pp.on ? pp.kappa64 : 0.f, true);
}

}  // namespace

extern "C" {

int sina_hip_align_families(sina_hip_ctx *c, const uint32_t *fam_ids, const uint64_t *fam_off, uint32_t nq,
                            const uint8_t *qmask, const uint64_t *qoff, const sina_hip_align_params *p,
                            sina_hip_align_out *out, uint32_t *out_pos) {
    return align_family_batches(c, FamilyCall{"align_families", build_graphs_for_launch, false, fam_ids, fam_off, nq, qmask, qoff, p, out, out_pos});
}

int sina_hip_align_families_wsets(sina_hip_ctx *c, const uint32_t *fam_ids, const uint64_t *fam_off, uint32_t nq,
                                  const uint8_t *qmask, const uint64_t *qoff, const sina_hip_align_params *p,
                                  const uint32_t *weight_set, uint32_t n_sets, sina_hip_align_out *out, uint32_t *out_pos) {
    if (p && !weighted_scheme(p)) SH_FAIL("align_families_wsets: weight sets need positional weights (p->weights, p->n_weights)");
    return align_family_batches(c, FamilyCall{"align_families_wsets", build_graphs_for_launch, false, fam_ids, fam_off, nq, qmask, qoff, p,
                                             out, out_pos, weight_set, n_sets});
}

#ifdef SINA_DP_PROFILE
int sina_hip_debug_graph_profile(unsigned long long *out16, int reset) {
    SH_CHECK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_graph_prof), sizeof(unsigned long long) * 16));
    if (reset) {
        unsigned long long z[16] = {};
        SH_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_graph_prof), z, sizeof z));
    }
    return 0;
}
#endif

int sina_hip_debug_family_graph(sina_hip_ctx *c, const uint32_t *fam_ids, uint32_t F, float fs_weight,
                                uint32_t ring_depth, uint32_t *n_nodes, uint32_t *n_edges, uint32_t *pos,
                                uint8_t *mask, float *weight, uint32_t *pred_off, uint32_t *pred,
                                uint32_t *succ_minpos, uint8_t *sink, uint32_t *spill_idx, uint32_t cap_nodes,
                                uint32_t cap_edges) {
    if (!c || !fam_ids || !n_nodes || !n_edges) SH_FAIL("debug_family_graph: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->st->have_refs) SH_FAIL("debug_family_graph: upload references first");
    if (F == 0 || F > (uint32_t)kMaxFam) SH_FAIL("debug_family_graph: family size must be in 1..128");
    SH_CHECK(hipSetDevice(c->device));
    const uint64_t foff[2] = {0, F};
    BuiltGraphs bg;
    // (with the row-skip bound for the default scoring: sina_hip_debug_rgain reads it back)
    if (build_family_graphs(c, fam_ids, foff, 0, 1, fs_weight, (int)ring_depth, &bg, true, fs_weight >= 0.f ? 64.0f * 1.0001f * 2.0f : 0.f, false)) return 1;
    const uint32_t N = bg.sizes[kBuiltN];
    std::vector<uint4> rec(N);
    std::vector<uint32_t> pr(bg.sizes[kBuiltEdges] + 8);
    SH_CHECK(hipMemcpy(rec.data(), c->rec.p, sizeof(uint4) * N, hipMemcpyDeviceToHost));
    SH_CHECK(hipMemcpy(pr.data(), c->pred.p, 4 * pr.size(), hipMemcpyDeviceToHost));
    uint32_t E = 0;
    for (uint32_t m = 0; m < N; m++) E += rec[m].z & 0xffu;
    *n_nodes = N;
    *n_edges = E;
    if (N > cap_nodes || E > cap_edges) SH_FAIL("debug_family_graph: output buffers too small");
    SH_CHECK(hipMemcpy(pos, c->node_pos.p, 4 * N, hipMemcpyDeviceToHost));
    SH_CHECK(hipMemcpy(succ_minpos, c->succ_minpos.p, 4 * N, hipMemcpyDeviceToHost));
    uint32_t e = 0;
    for (uint32_t m = 0; m < N; m++) {
        mask[m] = (uint8_t)((rec[m].z >> 8) & 0xffu);
        memcpy(&weight[m], &rec[m].y, 4);
        sink[m] = (rec[m].z & kRecSink) ? 1 : 0;
        spill_idx[m] = rec[m].w;
        pred_off[m] = e;
        for (uint32_t x = 0; x < (rec[m].z & 0xffu); x++) pred[e++] = pr[rec[m].x + x] & 0xffffu;
    }
    pred_off[N] = e;
    return 0;
}

int sina_hip_debug_family_graph_words(sina_hip_ctx *c, const uint32_t *fam_ids, uint32_t F, float fs_weight,
                                      uint32_t ring_depth, uint32_t *n_nodes, uint32_t *n_edges, uint32_t *rec_z,
                                      uint32_t *rec_w, uint32_t *pred_entries, uint32_t *size_words, uint32_t cap_nodes,
                                      uint32_t cap_edges) {
    if (!c || !fam_ids || !n_nodes || !n_edges || !rec_z || !rec_w || !pred_entries || !size_words)
        SH_FAIL("debug_family_graph_words: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->st->have_refs) SH_FAIL("debug_family_graph_words: upload references first");
    if (F == 0 || F > (uint32_t)kMaxFam) SH_FAIL("debug_family_graph_words: family size must be in 1..128");
    SH_CHECK(hipSetDevice(c->device));
    const uint64_t foff[2] = {0, F};
    BuiltGraphs bg;
    // (the same build as sina_hip_debug_family_graph's: successor minima and the row-skip bound of the default scoring)
    if (build_family_graphs(c, fam_ids, foff, 0, 1, fs_weight, (int)ring_depth, &bg, true, fs_weight >= 0.f ? 64.0f * 1.0001f * 2.0f : 0.f, false)) return 1;
    const uint32_t N = bg.sizes[kBuiltN];
    std::vector<uint4> rec(N);
    std::vector<uint32_t> pr(bg.sizes[kBuiltEdges] + 8);
    if (N) SH_CHECK(hipMemcpy(rec.data(), c->rec.p, sizeof(uint4) * N, hipMemcpyDeviceToHost));
    SH_CHECK(hipMemcpy(pr.data(), c->pred.p, 4 * pr.size(), hipMemcpyDeviceToHost));
    uint32_t E = 0;
    for (uint32_t m = 0; m < N; m++) E += rec[m].z & 0xffu;
    *n_nodes = N;
    *n_edges = E;
    if (N > cap_nodes || E > cap_edges) SH_FAIL("debug_family_graph_words: output buffers too small");
    uint32_t e = 0;
    for (uint32_t m = 0; m < N; m++) {
        rec_z[m] = rec[m].z;
        rec_w[m] = rec[m].w;
        for (uint32_t x = 0; x < (rec[m].z & 0xffu); x++) pred_entries[e++] = pr[rec[m].x + x];
    }
    memcpy(size_words, bg.sizes.data(), 4 * kBuiltWords);
    return 0;
}

}  // extern "C"
