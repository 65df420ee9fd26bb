// Family profile build on the GPU + sina_hip_align_profiles (--fs-no-graph).
//
// What it computes: pseq::pseq + scoring_scheme_profile's match term for every query's family (reference
// src/pseq.cpp, src/pseq.h:65-113, src/align.cpp:428-433) -- exactly what build_family_profile() / profile_comp()
// (host/family_graph.cpp) tabulate on the host:
//   * one node for alignment column 0, occupied or not, then one per occupied column, ascending; every node's one
//     predecessor is the node before it;
//   * per node the column's base_profile: twelve points per member that has a base there, split evenly over the
//     bases of its IUPAC code (A, G, C, T/U), twelve per member whose gap OPENS there (absent, and present -- or
//     never absent since its last real base -- at the node before), twelve per member whose gap EXTENDS there (absent
//     before as well; a member's leading gap counts as extended); a base without any of the four bits is consumed
//     and changes nothing.  Shares = points / sum of points;
//   * score16[16 * node + m] = base_profile::comp(node's shares, shares of a base with mask m), m = 1..15; entry 0
//     (a mask no query base has) is +inf.
//
// How it maps to the hardware: one workgroup per distinct ordered family, like the DAG build (graph_build.hip).
//   1. occupied-column bitmap in LDS (atomicOr per base; bit 0 is set whatever the family says), prefix popcount ->
//      the node of every alignment column -- the DAG build's steps 1 and 2;
//   2. columns, row records, predecessor entries of the chain: what prep_range() (dp_plan.h) makes of the host-built
//      chain -- every finished row is handed to the next one in registers, no spill rows;
//   3. per tile of nodes (all of them for a 16S family): one thread per BASE of the family.  Its points go to its
//      node's counters; the absent stretch behind it -- the nodes up to its member's next base -- opens at the first
//      node and extends on the rest, which is one +1 / -1 pair in a difference array however long the stretch is.
//      LDS atomics on 16-bit counters packed in pairs (128 members * 12 points < 2^16); integers, so the result
//      does not depend on the order of arrival.  A prefix sum turns the differences into the extended counts;
//   4. one lane per (node, mask): six shares, sixteen products in base_profile::comp's order, two gap terms; a wave
//      stores 256 contiguous bytes.
// A family with more nodes than the LDS tile holds is swept tile by tile; every member keeps a cursor (the last
// base in front of the next tile), and a stretch that began in an earlier tile is clamped to the tile's first node.
// Floating point: conversion of the integer points, IEEE division, products and sums in the host's order; the
// library is compiled with -ffp-contract=off.
#include <algorithm>
#include <cstring>
#include <limits>

#include "common.h"
#include "ctx.h"

namespace sina_hip {
namespace {

constexpr int kPT = 512;             // threads per workgroup
constexpr uint32_t kTileMax = 6144;  // nodes whose counters are in LDS at a time, at most (12 bytes each)
constexpr uint32_t kLdsSlack = 256;  // the kernel's static LDS, rounded up

// base_profile(const base_iupac&), pseq.h:65-86
struct Shares {
    float v[6];  // A, G, C, T/U, opened gaps, extended gaps
};
__host__ __device__ inline Shares shares_of_mask(uint32_t mask) {
    Shares b;
    for (int i = 0; i < 6; i++) b.v[i] = 0.f;
    const int order = ((mask >> 0) & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1);
    if (order > 0) {
        const float val = 1.f / (float)order;
        for (int i = 0; i < 4; i++)
            if (mask & (1u << i)) b.v[i] = val;
    }
    return b;
}
// base_profile::comp, pseq.h:100-113: sixteen products in i-outer, j-inner order, then the gap terms
__host__ __device__ inline float profile_comp(const Shares &a, const Shares &b, float match, float mismatch, float gap, float gap_ext) {
    float res = 0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            if (i == j) res += match * a.v[i] * b.v[j];
            else res += mismatch * a.v[i] * b.v[j];
        }
    return res + gap * a.v[4] + gap_ext * a.v[5];
}

struct ProfileArgs {
    const uint32_t *ref_ab;
    const uint64_t *ref_off;
    const uint32_t *fam_ids;  // concatenated
    const uint64_t *fam_off;  // [n + 1]
    uint4 *rec;               // [n][ncap]
    uint32_t *node_pos;       // [n][ncap]
    uint32_t *succ_min;       // [n][ncap]
    uint32_t *pred;           // [n][pred_stride]
    uint2 *pred4;             // [n][ncap] the first four predecessor ids of every node (common.h, pred4_pack): the one before it
    float *prof16;           // [n][ncap][16]
    uint32_t *sizes;          // [n][kBuiltWords]: N, edges, 0, status (0 or kBuiltNodeCap: more than ncap or 65535 nodes), first sink row, 0
    uint32_t width, ncap, pred_stride;
    uint32_t tile_nodes;      // nodes per LDS tile
    uint32_t bitmap_off;      // LDS offset of the occupied-column bitmap (behind the three counter arrays)
    uint32_t member_off;      // LDS offset of the per-member records (behind the bitmap and its ranks)
    float match, mismatch, gap, gap_ext;  // the scheme's: -match_score, -mismatch_score, pen_gap, pen_gapext
};

// per family member, in LDS
struct PMember {
    uint64_t beg;        // offset of its bases in the store
    uint32_t len;
    uint32_t cur, curn;  // the first base this tile looks at, ... the next tile will
    uint32_t pad_;
};
static_assert(sizeof(PMember) == 24, "LDS layout");

__global__ void __launch_bounds__(kPT) family_profile_kernel(ProfileArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_tmp[kPT / 64 + 2];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const uint32_t nwords = (a.width + 31) / 32;
    const uint64_t f0 = a.fam_off[q];
    const uint32_t F = (uint32_t)(a.fam_off[q + 1] - f0);
    const uint32_t T = a.tile_nodes;
    // per node of the tile, 16-bit counters in pairs: points of A | G << 16; of C | T << 16; members whose gap opens |
    // difference of the members whose gap extends << 16 (step 3: after the prefix sum, their number)
    uint32_t *cAG = reinterpret_cast<uint32_t *>(smem);
    uint32_t *cCT = cAG + T;
    uint32_t *cGap = cCT + T;
    uint32_t *bitmap = reinterpret_cast<uint32_t *>(smem + a.bitmap_off);  // [nwords]
    uint16_t *wrank = reinterpret_cast<uint16_t *>(bitmap + nwords);      // [nwords]
    PMember *mb = reinterpret_cast<PMember *>(smem + a.member_off);       // [F]

    uint32_t *sz = a.sizes + kBuiltWords * (size_t)q;
    for (uint32_t j = tid; j < F; j += kPT) {
        const uint32_t id = a.fam_ids[f0 + j];
        mb[j].beg = a.ref_off[id];
        mb[j].len = (uint32_t)(a.ref_off[id + 1] - a.ref_off[id]);
        mb[j].cur = mb[j].curn = 0;
    }
    for (uint32_t i = tid; i < nwords; i += kPT) bitmap[i] = (i == 0) ? 1u : 0u;  // (column 0 has a node whatever happens)
    __syncthreads();

    // 1. occupied columns (the DAG build's step 1: eight members' loads in flight per thread)
    for (uint32_t j0 = 0; j0 < F; j0 += 8) {
        uint32_t maxlen = 0;
#pragma unroll
        for (int u = 0; u < 8; u++) maxlen = max(maxlen, j0 + u < F ? mb[j0 + u].len : 0u);
        for (uint32_t i = tid; i < maxlen; i += kPT) {
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
    // ... and the node of every column: rank(pos) = wrank[pos >> 5] + popc(bits below)
    {
        const uint32_t chunk = (nwords + kPT - 1) / kPT;
        const uint32_t b = min(nwords, tid * chunk), e = min(nwords, b + chunk);
        uint32_t s = 0;
        for (uint32_t i = b; i < e; i++) s += __popc(bitmap[i]);
        uint32_t x = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(x, off);
            if ((int)lane >= off) x += y;
        }
        if (lane == 63) s_tmp[wave] = x;
        __syncthreads();
        uint32_t base = 0, total = 0;
        for (uint32_t w = 0; w < (uint32_t)kPT / 64; w++) {
            if (w < wave) base += s_tmp[w];
            total += s_tmp[w];
        }
        uint32_t run = base + x - s;
        for (uint32_t i = b; i < e; i++) {
            wrank[i] = (uint16_t)run;
            run += __popc(bitmap[i]);
        }
        if (tid == 0) s_tmp[kPT / 64] = total;
    }
    __syncthreads();
    const uint32_t N = s_tmp[kPT / 64];
    if (N > a.ncap || N > 65535u) {  // (nothing has been written: the host grows the arrays and comes again, or gives up)
        if (tid == 0) {
            sz[kBuiltN] = N;
            sz[kBuiltEdges] = sz[kBuiltSpill] = 0;
            sz[kBuiltStatus] = kBuiltNodeCap;
            sz[kBuiltFirstSink] = sz[kBuiltGmin] = 0;
        }
        return;
    }
    auto rank = [&](uint32_t pos) -> uint32_t {
        return (uint32_t)wrank[pos >> 5] + __popc(bitmap[pos >> 5] & ((1u << (pos & 31)) - 1u));
    };

    // 2. the chain as the DP kernel reads it
    {
        uint4 *rec = a.rec + (size_t)q * a.ncap;
        uint32_t *node_pos = a.node_pos + (size_t)q * a.ncap;
        uint32_t *smin = a.succ_min + (size_t)q * a.ncap;
        uint32_t *pred = a.pred + (size_t)q * a.pred_stride;
        uint2 *pred4 = a.pred4 + (size_t)q * a.ncap;
        for (uint32_t w = tid; w < nwords; w += kPT) {
            uint32_t bits = bitmap[w], n = wrank[w];
            while (bits) {
                const uint32_t pos = w * 32u + (uint32_t)(__ffs(bits) - 1);
                bits &= bits - 1u;
                node_pos[n] = pos;
                if (n > 0) smin[n - 1] = pos;  // the successor's column (for --insertion=forbid)
                n++;
            }
        }
        for (uint32_t n = tid; n < N; n += kPT) {
            uint4 r;
            r.x = n > 0 ? n - 1u : 0u;  // its predecessor entry
            r.y = 0u;                   // (node weight 0.f, mask 0: a profile's match term comes from prof16)
            r.z = (n > 0 ? 1u : 0u) | (n + 1 == N ? kRecSink : 0u) | ((n > 0 ? 1u : kRecDistFar) << kRecDistShift);
            r.w = kRowNone;             // (only the next row reads it: handed over in registers)
            rec[n] = r;
            pred4[n] = pred4_pack(n > 0 ? n - 1u : 0u, 0u, 0u, 0u);
            if (n + 1 < N) pred[n] = n;  // entry n: node n + 1's predecessor
        }
        if (tid == 0) {
            smin[N - 1] = 1000000u;  // "no successor" sentinel of mesh.h:480
            sz[kBuiltN] = N;
            sz[kBuiltEdges] = N - 1u;
            sz[kBuiltSpill] = 0;
            sz[kBuiltStatus] = 0;
            sz[kBuiltFirstSink] = N - 1u;
            sz[kBuiltGmin] = 0;
        }
    }

    float *prof = a.prof16 + 16 * ((size_t)q * a.ncap);
    for (uint32_t n0 = 0; n0 < N; n0 += T) {
        const uint32_t n1 = min(N, n0 + T), tn = n1 - n0;
        for (uint32_t i = tid; i < tn; i += kPT) cAG[i] = cCT[i] = cGap[i] = 0;
        __syncthreads();
        // members absent on nodes [x, y): their gap extends there
        auto extends_on = [&](uint32_t x, uint32_t y) {
            const uint32_t lo = max(x, n0), hi = min(y, n1);
            if (lo >= hi) return;
            atomicAdd(&cGap[lo - n0], 0x00010000u);
            if (hi < n1) atomicAdd(&cGap[hi - n0], 0xFFFF0000u);  // (-1 in the upper half)
        };
        // 3. a wave per member, a lane per base; four loads in flight per lane
        for (uint32_t j = wave; j < F; j += (uint32_t)kPT / 64) {
            const uint32_t cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)mb[j].cur);
            const uint32_t len = (uint32_t)__builtin_amdgcn_readfirstlane((int)mb[j].len);
            const uint32_t *bases = a.ref_ab + mb[j].beg;
            if (len == 0) {  // (absent everywhere: one long leading gap)
                if (lane == 0) extends_on(0, N);
                continue;
            }
            bool beyond = false;  // the whole wave is past the tile: so is the rest of the member
            for (uint32_t i0 = cur; i0 < len && !beyond; i0 += 256) {
                uint32_t abv[4], nxv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t i = i0 + 64u * (uint32_t)u + lane;
                    abv[u] = i < len ? bases[i] : 0xFFFFFFFFu;
                    nxv[u] = i + 1 < len ? bases[i + 1] : 0xFFFFFFFFu;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t i = i0 + 64u * (uint32_t)u + lane;
                    if (abv[u] == 0xFFFFFFFFu) continue;
                    const uint32_t m = (abv[u] >> 24) & 0xFu;
                    const uint32_t r = rank(abv[u] & 0xFFFFFFu);
                    const uint32_t r1 = nxv[u] != 0xFFFFFFFFu ? rank(nxv[u] & 0xFFFFFFu) : N;  // the member is absent on (r, r1)
                    const uint32_t order = (uint32_t)__popc(m);
                    if (order && r >= n0 && r < n1) {
                        const uint32_t pts = (0x346Cu >> (4u * (order - 1u))) & 0xFu;  // 12 / order
                        const uint32_t v0 = ((m & 1u) ? pts : 0u) | ((m & 2u) ? pts << 16 : 0u);
                        const uint32_t v1 = ((m & 4u) ? pts : 0u) | ((m & 8u) ? pts << 16 : 0u);
                        if (v0) atomicAdd(&cAG[r - n0], v0);
                        if (v1) atomicAdd(&cCT[r - n0], v1);
                    }
                    if (i == 0) extends_on(0, r);  // (a member's leading gap counts as extended)
                    if (r + 1 < r1 && r + 1 < n1 && r1 > n0) {
                        // In a gap already?  Never behind a real base.  A base without any of the four bits leaves the
                        // state as it found it: what the bases before it say (rare: a walk back through them).
                        bool in_gap = false;
                        if (!order) {
                            in_gap = true;  // (nothing but such bases since the start: the leading gap)
                            uint32_t k = i, rk1 = r;
                            while (k > 0) {
                                k--;
                                const uint32_t abk = bases[k];
                                const uint32_t rk = rank(abk & 0xFFFFFFu);
                                if (rk + 1 < rk1) break;  // absent in between: in a gap
                                if ((abk >> 24) & 0xFu) {
                                    in_gap = false;
                                    break;
                                }
                                rk1 = rk;
                            }
                        }
                        uint32_t x = r + 1;
                        if (!in_gap) {
                            if (x >= n0) atomicAdd(&cGap[x - n0], 1u);  // (x < n1: checked above)
                            x++;
                        }
                        extends_on(x, r1);
                    }
                    if (r < n1 && r1 >= n1) mb[j].curn = i;  // (one base per member: the last one in front of the next tile)
                }
                const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)abv[0]);  // (lane 0 of chunk 0: i0 < len)
                beyond = rank(first & 0xFFFFFFu) >= n1;
            }
        }
        __syncthreads();
        // the extended counts: inclusive prefix sum of the differences
        {
            const uint32_t chunk = (tn + kPT - 1) / kPT;
            const uint32_t b = min(tn, tid * chunk), e = min(tn, b + chunk);
            int s = 0;
            for (uint32_t i = b; i < e; i++) s += (int)(int16_t)(uint16_t)(cGap[i] >> 16);
            int x = s;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int y = __shfl_up(x, off);
                if ((int)lane >= off) x += y;
            }
            if (lane == 63) s_tmp[wave] = (uint32_t)x;
            __syncthreads();
            int run = x - s;
            for (uint32_t w = 0; w < wave; w++) run += (int)s_tmp[w];
            for (uint32_t i = b; i < e; i++) {
                const uint32_t v = cGap[i];
                run += (int)(int16_t)(uint16_t)(v >> 16);
                cGap[i] = (v & 0xFFFFu) | ((uint32_t)run << 16);
            }
        }
        __syncthreads();
        // 4. the match terms: a lane per (node, mask)
        for (uint32_t t = tid; t < 16u * tn; t += kPT) {
            const uint32_t ln = t >> 4, m = t & 15u;
            float v = std::numeric_limits<float>::infinity();  // (mask 0: no query base has it)
            if (m) {
                const uint32_t w0 = cAG[ln], w1 = cCT[ln], w2 = cGap[ln];
                const int c0 = (int)(w0 & 0xFFFFu), c1 = (int)(w0 >> 16), c2 = (int)(w1 & 0xFFFFu), c3 = (int)(w1 >> 16);
                const int open = (int)(w2 & 0xFFFFu) * 12, ext = (int)(w2 >> 16) * 12;
                const float sum = (float)(c0 + c1 + c2 + c3 + open + ext);
                Shares col;
                col.v[0] = (float)c0 / sum;
                col.v[1] = (float)c1 / sum;
                col.v[2] = (float)c2 / sum;
                col.v[3] = (float)c3 / sum;
                col.v[4] = (float)open / sum;
                col.v[5] = (float)ext / sum;
                v = profile_comp(col, shares_of_mask(m), a.match, a.mismatch, a.gap, a.gap_ext);
            }
            prof[16 * (size_t)n0 + t] = v;
        }
        for (uint32_t j = tid; j < F; j += kPT) mb[j].cur = mb[j].curn;
        __syncthreads();
    }
}

// LDS of one workgroup: the counters of a tile, the bitmap + ranks, the member records
struct ProfileLds {
    uint32_t tile_nodes, bitmap_off, member_off;
    size_t total;
};
// forced != 0: at most that many nodes per tile (SINA_HIP_TEST=profile_tile=N), never more than the LDS allows
bool profile_lds(uint32_t width, uint32_t max_family, uint32_t ncap, uint32_t forced, ProfileLds *l) {
    const size_t nwords = (width + 31) / 32;
    const size_t bm = (6 * nwords + 15) & ~(size_t)15, members = sizeof(PMember) * (size_t)max_family;
    const size_t budget = 160 * 1024 - kLdsSlack;
    if (bm + members + 12 * 64 + 16 > budget) return false;
    const size_t room = (budget - bm - members - 16) / 12;
    size_t tile = std::min<size_t>(std::min<size_t>(ncap, kTileMax), room);
    if (forced) tile = std::min<size_t>(tile, forced);
    l->tile_nodes = (uint32_t)std::max<size_t>(1, tile);
    l->bitmap_off = (uint32_t)((12 * (size_t)l->tile_nodes + 15) & ~(size_t)15);
    l->member_off = (uint32_t)(l->bitmap_off + bm);
    l->total = l->member_off + members;
    return true;
}

void self_scores(const sina_hip_align_params *p, float *out16) {  // profile_self_scores (host/family_graph.cpp)
    out16[0] = 0.f;
    for (unsigned m = 1; m < 16; m++) {
        const Shares b = shares_of_mask(m);
        out16[m] = profile_comp(b, b, -p->match_score, -p->mismatch_score, p->gap_penalty, p->gap_ext_penalty);
    }
}

// Builds the profiles of n families (fam_off is absolute, first family = q0) into the context's rec / node_pos /
// succ_minpos / pred / prof16 buffers, and uploads the scheme's self16.  The arrays are sized by the node count of the
// context's last profile build (64 bytes of prof16 per node: not by a cap that suits every family); a family with
// more nodes reports its count before anything is written, and the launch is repeated with room for it.
int build_family_profiles(sina_hip_ctx *c, const uint32_t *fam_ids, const uint64_t *fam_off, uint32_t q0, uint32_t n,
                          const sina_hip_align_params *p, int /*W: no row is kept for later*/, const PrunePlan & /*off*/, BuiltGraphs *bg) {
    hipStream_t s = c->stream;
    if (ensure_ref_off_host(c)) return 1;
    std::vector<uint64_t> foff(n + 1);
    uint64_t bases = 0;
    uint32_t max_f = 1;
    for (uint32_t q = 0; q <= n; q++) foff[q] = fam_off[q0 + q] - fam_off[q0];
    for (uint32_t q = 0; q < n; q++) {
        max_f = std::max<uint32_t>(max_f, (uint32_t)(foff[q + 1] - foff[q]));
        for (uint64_t x = fam_off[q0 + q]; x < fam_off[q0 + q + 1]; x++) {
            const uint32_t id = fam_ids[x];
            if (id >= c->st->n_refs) SH_FAIL("align_profiles: reference id out of range");
            bases += c->st->ref_off_host[id + 1] - c->st->ref_off_host[id];
        }
        // (a family without a single base still has the node of column 0: unlike the DAG build, graph_build.hip, nothing
        // to refuse here)
    }
    float self16[16];
    self_scores(p, self16);
    if (c->self16.reserve(64) || upload(c, 8, c->self16.p, self16, 64, s)) return 1;
    if (c->g_fam_ids.reserve(4 * std::max<uint64_t>(foff[n], 1)) || c->g_fam_off.reserve(8 * ((uint64_t)n + 1)) ||
        c->g_sizes.reserve(4 * kBuiltWords * (uint64_t)n))
        return 1;
    if (upload(c, 1, c->g_fam_ids.p, fam_ids + fam_off[q0], 4 * foff[n], s) ||
        upload(c, 2, c->g_fam_off.p, foff.data(), 8 * ((uint64_t)n + 1), s))
        return 1;
    if (allow_full_lds(reinterpret_cast<const void *>(family_profile_kernel))) return 1;
    uint32_t ncap = c->prof_ncap ? c->prof_ncap : 4096u;
    uint32_t max_n = 1;
    // (SINA_HIP_TEST=profile_tile=N: tiles of N nodes, so that a family of a few hundred nodes is swept in several)
    const uint32_t forced_tile = (uint32_t)strtoul(test_knob("profile_tile").c_str(), nullptr, 10);
    for (int attempt = 0;; attempt++) {
        ProfileLds lds;
        if (!profile_lds(c->st->width, max_f, ncap, forced_tile, &lds)) SH_FAIL_LIMIT("align_profiles: family too wide for the device profile build");
        const uint32_t pred_stride = ncap + 8;  // (slack behind every list, like the DAG build's)
        if (c->rec.reserve(sizeof(uint4) * (uint64_t)n * ncap) || c->node_pos.reserve(4 * (uint64_t)n * ncap) ||
            c->succ_minpos.reserve(4 * (uint64_t)n * ncap) || c->pred.reserve(4 * (uint64_t)n * pred_stride) ||
            c->pred4.reserve(sizeof(uint2) * (uint64_t)n * ncap) ||
            c->prof16.reserve(64 * (uint64_t)n * ncap))
            return 1;
        ProfileArgs pa;
        pa.ref_ab = c->st->ref_ab.as<uint32_t>();
        pa.ref_off = c->st->ref_off.as<uint64_t>();
        pa.fam_ids = c->g_fam_ids.as<uint32_t>();
        pa.fam_off = c->g_fam_off.as<uint64_t>();
        pa.rec = c->rec.as<uint4>();
        pa.node_pos = c->node_pos.as<uint32_t>();
        pa.succ_min = c->succ_minpos.as<uint32_t>();
        pa.pred = c->pred.as<uint32_t>();
        pa.pred4 = c->pred4.as<uint2>();
        pa.prof16 = c->prof16.as<float>();
        pa.sizes = c->g_sizes.as<uint32_t>();
        pa.width = c->st->width;
        pa.ncap = ncap;
        pa.pred_stride = pred_stride;
        pa.tile_nodes = lds.tile_nodes;
        pa.bitmap_off = lds.bitmap_off;
        pa.member_off = lds.member_off;
        pa.match = -p->match_score;  // scoring_scheme_profile(-match, -mismatch, gap, gapext), align.cpp:428-433
        pa.mismatch = -p->mismatch_score;
        pa.gap = p->gap_penalty;
        pa.gap_ext = p->gap_ext_penalty;
        {
            heavy_launch hl(c, s, kHeavyGraph);  // (a device-filling kernel: ctx.h)
            SH_CHECK(hipEventRecord(c->ev[6], hl.stream()));
            hipLaunchKernelGGL(family_profile_kernel, dim3(n), dim3(kPT), lds.total, hl.stream(), pa);
            SH_CHECK(hipGetLastError());
            SH_CHECK(hipEventRecord(c->ev[7], hl.stream()));
            if (hl.done()) return 1;
        }
        if (download(c, 4, c->g_sizes.p, 4 * kBuiltWords * (uint64_t)n, s)) return 1;
        SH_CHECK(wait_stream(c, s));
        bg->sizes.resize(kBuiltWords * (size_t)n);
        memcpy(bg->sizes.data(), c->h_stage[4].p, 4 * kBuiltWords * (uint64_t)n);
        float gms = 0;
        SH_CHECK(hipEventElapsedTime(&gms, c->ev[6], c->ev[7]));
        uint32_t need_n = 0;
        uint64_t nodes = 0;
        max_n = 1;
        for (uint32_t q = 0; q < n; q++) {
            const uint32_t N = bg->sizes[kBuiltWords * q + kBuiltN];
            if (bg->sizes[kBuiltWords * q + kBuiltStatus] == kBuiltNodeCap) need_n = std::max(need_n, N);
            else nodes += N;
            max_n = std::max(max_n, N);
        }
        {
            // One build = one launch in the counters, however often the kernel had to come again (its time is all
            // there).  Algorithmic bytes, counted once, for the attempt that built everything: the families' bases in,
            // the profiles out -- row record, column, successor column, predecessor entry, sixteen match terms per node
            std::lock_guard<std::mutex> slk(c->st->stats_mu);
            c->st->stats.graph_ms += gms;
            if (!need_n) {
                c->st->stats.graph_bytes += 4 * bases + nodes * (16 + 4 + 4 + 4 + 8 + 64);
                c->st->stats.graph_launches++;
            }
        }
        if (!need_n) break;
        if (attempt >= 3 || need_n > 65535u) SH_FAIL_LIMIT("align_profiles: family profile exceeds device limits (more than 65535 nodes)");
        ncap = std::min<uint32_t>(65535, need_n + need_n / 8 + 16);
    }
    // what the next launch starts with: never less than before -- a workload that alternates short and long families
    // would otherwise build every long chunk twice (the buffers never shrink either)
    c->prof_ncap = std::max(c->prof_ncap, std::min<uint32_t>(65535, max_n + max_n / 8 + 16));
    bg->ncap = ncap;
    bg->pred_off.resize(n);
    for (uint32_t q = 0; q < n; q++) bg->pred_off[q] = (uint64_t)q * (ncap + 8);
    return 0;
}

}  // namespace
}  // namespace sina_hip

using namespace sina_hip;

extern "C" {

int sina_hip_align_profiles(sina_hip_ctx *c, const uint32_t *fam_ids, const uint64_t *fam_off, uint32_t nq,
                            const uint8_t *qmask, const uint64_t *qoff, const sina_hip_align_params *p,
                            sina_hip_align_out *out, uint32_t *out_pos) {
    return align_family_batches(c, FamilyCall{"align_profiles", build_family_profiles, true, fam_ids, fam_off, nq, qmask, qoff, p, out, out_pos});
}

int sina_hip_debug_family_profile(sina_hip_ctx *c, const uint32_t *fam_ids, uint32_t F, float match, float mismatch,
                                  float gap, float gap_ext, uint32_t *n_nodes, uint32_t *pos, float *score16,
                                  float *self16, uint32_t cap_nodes) {
    if (!c || !fam_ids || !n_nodes || !pos || !score16 || !self16) SH_FAIL("debug_family_profile: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->st->have_refs) SH_FAIL("debug_family_profile: upload references first");
    if (F == 0 || F > (uint32_t)kFamilyMax) SH_FAIL("debug_family_profile: family size must be in 1..128");
    if (c->st->width > 524288u) SH_FAIL("debug_family_profile: alignment wider than 524288 columns");
    SH_CHECK(hipSetDevice(c->device));
    sina_hip_align_params p;
    memset(&p, 0, sizeof p);
    p.match_score = -match;  // (the arguments are the scheme's: the builder negates the options back)
    p.mismatch_score = -mismatch;
    p.gap_penalty = gap;
    p.gap_ext_penalty = gap_ext;
    const uint64_t foff[2] = {0, F};
    BuiltGraphs bg;
    if (build_family_profiles(c, fam_ids, foff, 0, 1, &p, 0, PrunePlan(), &bg)) return 1;
    const uint32_t N = bg.sizes[kBuiltN];
    *n_nodes = N;
    if (N > cap_nodes) SH_FAIL("debug_family_profile: output buffers too small");
    SH_CHECK(hipMemcpy(pos, c->node_pos.p, 4 * (size_t)N, hipMemcpyDeviceToHost));
    SH_CHECK(hipMemcpy(score16, c->prof16.p, 64 * (size_t)N, hipMemcpyDeviceToHost));
    self_scores(&p, self16);
    return 0;
}

int sina_hip_debug_family_profile_words(sina_hip_ctx *c, const uint32_t *fam_ids, uint32_t F, uint32_t *n_nodes,
                                        uint32_t *rec_words, uint32_t *succ_min, uint32_t *pred_entries,
                                        uint32_t *size_words, uint32_t cap_nodes) {
    if (!c || !fam_ids || !n_nodes || !rec_words || !succ_min || !pred_entries || !size_words)
        SH_FAIL("debug_family_profile_words: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->st->have_refs) SH_FAIL("debug_family_profile_words: upload references first");
    if (F == 0 || F > (uint32_t)kFamilyMax) SH_FAIL("debug_family_profile_words: family size must be in 1..128");
    if (c->st->width > 524288u) SH_FAIL("debug_family_profile_words: alignment wider than 524288 columns");
    SH_CHECK(hipSetDevice(c->device));
    sina_hip_align_params p;
    sina_hip_align_params_default(&p);  // (the chain does not depend on the scheme)
    const uint64_t foff[2] = {0, F};
    BuiltGraphs bg;
    if (build_family_profiles(c, fam_ids, foff, 0, 1, &p, 0, PrunePlan(), &bg)) return 1;
    const uint32_t N = bg.sizes[kBuiltN];
    *n_nodes = N;
    if (N > cap_nodes) SH_FAIL("debug_family_profile_words: output buffers too small");
    static_assert(sizeof(uint4) == 16, "four words per row record");
    SH_CHECK(hipMemcpy(rec_words, c->rec.p, sizeof(uint4) * (size_t)N, hipMemcpyDeviceToHost));
    SH_CHECK(hipMemcpy(succ_min, c->succ_minpos.p, 4 * (size_t)N, hipMemcpyDeviceToHost));
    if (N > 1) SH_CHECK(hipMemcpy(pred_entries, c->pred.p, 4 * (size_t)(N - 1), hipMemcpyDeviceToHost));
    memcpy(size_words, bg.sizes.data(), 4 * kBuiltWords);
    return 0;
}

}  // extern "C"
