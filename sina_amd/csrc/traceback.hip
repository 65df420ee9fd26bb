// Trace-back walk + alignment assembly for gfx950 (CDNA4): what follows the DP fill (mesh_dp.hip) on the same stream.
//
// What it computes: the cell walk of backtrack() (reference src/mesh.h:594-721) from a query's DP result to its emitted
// columns, sum_weight and overhangs (walk_query; it resolves gapm_idx for the cells of the final path: common.h, kTbExt /
// kTbOpLast), and, where they are plain, the cseq container steps and the NAST fix-up (assemble_kernel).
// How it maps to the hardware: the walk is one logical thread per query, a chain of dependent look-ups -- one WAVE per
// query with a window of the plane in LDS (backtrack_kernel), or one LANE per query with plain global loads
// (backtrack_lanes_kernel) for large launches of short queries; which: bt_by_lanes (dp_plan.h).  Either way a step
// fetches its cell, the row's record and the row's first four predecessor ids (pred4) together.  assemble_kernel is one
// wave per query.  Built with the fill kernels' extra flags (Makefile): its code stays what it was inside mesh_dp.hip.
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "dp_plan.h"

namespace sina_hip {

namespace {

// The cell walk of backtrack() (mesh.h:594-721) reads three things of the trace-back plane: cells, row records
// and predecessor ids.  Two memory policies fetch them; walk_query() below is the walk itself.  A policy
// offers at(row, col) -- everything the walk needs of a cell, see BtAt --, cell(row, col) alone (the insertion
// scan), pred_far(pb, e) (predecessor entry e >= 4 of a row whose first is pb = rec.x) and `writes`: whether
// this thread stores the query's output.  LAZY: 16-bit cells (type code + predecessor ordinal) instead of 32-bit ones.
//
// What a step knows once it knows (row, col): the cell, the row's record (.w replaced by the node's column) and
// the ids of its first four predecessors (pred4, common.h).  None of the three depends on another, so a policy
// issues their loads together: one round trip per step where looking the predecessor entry up through the
// record's .x, then the cell, then the next record took three.
struct BtAt {
    uint32_t c;
    uint4 r;
    uint2 p4;
    __device__ uint32_t npred() const { return r.z & 0xffu; }
    __device__ uint32_t pred_near(uint32_t e) const {  // e < 4
        const uint32_t w = (e & 2u) ? p4.y : p4.x;
        return (e & 1u) ? w >> 16 : w & 0xffffu;
    }
};

// BtDirect: plain global loads, one lane per query (backtrack_lanes_kernel).
template <bool LAZY>
struct BtDirect {
    using cell_t = typename std::conditional<LAZY, uint16_t, uint32_t>::type;
    static constexpr bool writes = true;
    const cell_t *tb;
    const uint4 *recs;
    const uint2 *pred4;
    const uint32_t *node_pos, *preds;
    uint32_t Lp;
    __device__ BtDirect(const BtArgs &a, const QDesc &d)
        : tb(reinterpret_cast<const cell_t *>(a.tb) + d.tb_off), recs(a.rec + d.node_off), pred4(a.pred4 + d.node_off),
          node_pos(a.node_pos + d.node_off), preds(a.pred + d.edge_off), Lp(a.Lp) {}
    __device__ uint32_t cell(uint32_t row, uint32_t col) const { return (uint32_t)tb[(size_t)row * Lp + col]; }
    __device__ uint4 rec(uint32_t row) const {
        uint4 rx = recs[row];
        rx.w = node_pos[row];
        return rx;
    }
    __device__ BtAt at(uint32_t row, uint32_t col) const {  // four loads, none waiting for another
        BtAt x;
        x.c = cell(row, col);
        x.r = recs[row];
        x.r.w = node_pos[row];
        x.p4 = pred4[row];
        // All of it in registers HERE: left alone the compiler moves each word's load down to its first use, behind
        // the branches of the walk -- a round trip each again.
        asm volatile("" : "+v"(x.c), "+v"(x.r.x), "+v"(x.r.y), "+v"(x.r.z), "+v"(x.r.w), "+v"(x.p4.x), "+v"(x.p4.y));
        return x;
    }
    __device__ uint32_t pred_far(uint32_t pb, uint32_t e) const { return preds[pb + e] & 0xffffu; }
};

// BtWindow: one wave per query (backtrack_kernel).  There the walk is one logical thread (every lane computes the
// same thing) -- a chain of dependent look-ups, two per step when they go to HBM.  It only ever moves to smaller
// rows and smaller columns, so the wave keeps a WINDOW of the trace-back plane in LDS: the 64 rows x 32 columns
// whose upper right corner is the cell that missed, one row per lane, together with those rows' records, columns
// and first four predecessors.  A step inside the window costs LDS latency; a refill (one round trip, every ~30
// steps) is paid by 64 lanes at once.  Lane 0 writes.
constexpr int kBtRows = 64, kBtCols = 32;
template <bool LAZY>
struct BtWindow {
    using cell_t = typename BtDirect<LAZY>::cell_t;
    static constexpr uint32_t kAlign = 16 / sizeof(cell_t);  // cells per 16-byte load
    struct Lds {
        cell_t cell[kBtRows][kBtCols];
        uint4 rec[kBtRows];   // row records, .w replaced by the node's column
        uint2 pred[kBtRows];  // ids of the row's first four predecessors (pred4)
    };
    BtDirect<LAZY> g;  // (refills and the look-ups outside the window)
    Lds &w;
    uint32_t N, lane;
    bool writes;
    // rows [wr0, wr0 + 64), columns [wc0, wc0 + 32); empty until the first miss
    uint32_t wr0 = 0x80000000u, wc0 = 0;  // (no row is within 64 of that)
    __device__ BtWindow(const BtArgs &a, const QDesc &d, Lds &lds, uint32_t lane_)
        : g(a, d), w(lds), N(d.N), lane(lane_), writes(lane_ == 0) {}
    __device__ void refill(uint32_t row, uint32_t col) {
        __syncthreads();  // (one wave: orders the LDS reads before against the writes below)
        wr0 = row + 1 >= (uint32_t)kBtRows ? row + 1 - kBtRows : 0u;
        const uint32_t ctop = (col & ~(kAlign - 1)) + kAlign;  // first column right of the window
        wc0 = ctop >= (uint32_t)kBtCols ? ctop - kBtCols : 0u;
        const uint32_t x = wr0 + lane;
        if (x < N) {
            const uint4 *src = reinterpret_cast<const uint4 *>(g.tb + (size_t)x * g.Lp + wc0);
            uint4 *dst = reinterpret_cast<uint4 *>(&w.cell[lane][0]);
#pragma unroll
            for (uint32_t i = 0; i < kBtCols / kAlign; i++) dst[i] = src[i];
            w.rec[lane] = g.rec(x);
            w.pred[lane] = g.pred4[x];
        }
        __syncthreads();
    }
    __device__ bool in_rows(uint32_t row) const { return row - wr0 < (uint32_t)kBtRows; }
    __device__ uint32_t cell(uint32_t row, uint32_t col) {
        if (!(in_rows(row) && col - wc0 < (uint32_t)kBtCols)) refill(row, col);
        return (uint32_t)w.cell[row - wr0][col - wc0];
    }
    __device__ BtAt at(uint32_t row, uint32_t col) {
        BtAt x;
        x.c = cell(row, col);  // (first: a refill brings the row's record and predecessors along)
        x.r = w.rec[row - wr0];
        x.p4 = w.pred[row - wr0];
        return x;
    }
    __device__ uint32_t pred_far(uint32_t pb, uint32_t e) const { return g.pred_far(pb, e); }
};

// The walk of query q, from its DP result to its emitted columns (out_pos) and its sina_hip_align_out.
template <bool LAZY, class Mem>
__device__ __forceinline__ void walk_query(const BtArgs &a, uint32_t q, const QDesc &d, Mem &mem) {
    const DpResult r = a.res[q];
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
    if (r.status != 0) {
        if (mem.writes) a.out[q] = o;
        return;
    }
    uint32_t *out = a.out_pos + d.q_off;
    const uint32_t width = a.width;
    uint32_t m = r.end_m, s = r.end_s;
    uint32_t n = 0;
    const uint32_t send = d.L - 1;
    auto emit = [&](uint32_t p) {
        if (mem.writes) out[n] = p;
        n++;
    };

    // right hand overhang (:594-615)
    const int tail = (int)(send - s);
    o.cutoff_tail = tail;
    BtAt cur = mem.at(m, s);  // the cell the walk stands on, its row's record and predecessors
    uint4 rm = cur.r;
    if (tail && a.overhang != SINA_OVERHANG_REMOVE) {
        int pos = (a.overhang == SINA_OVERHANG_ATTACH) ? (int)(width - 1 - rm.w - (uint32_t)tail) : 0;
        for (int i = 0; i < tail; i++) {
            const int p = pos++;
            emit((uint32_t)(p > 0 ? p : 0));
        }
    }
    const uint8_t *qmb = a.qmask + d.q_off;
    // (the query's own positional weights, as in mesh_dp_kernel)
    const float *wts = a.weights;
    if (wts != nullptr && a.wset != nullptr) wts += (size_t)a.wset[q] * a.n_weights;
    auto mscore_at = [&](const uint4 &rx, uint32_t si) -> float {  // tr.s.match(sum, ab2, ab1) with comp()==true
        // (--fs-no-graph: the master copy takes the slave's base, its profile is compared with itself)
        if (a.self16 != nullptr) return a.self16[qmb[si] & 0xfu];
        const float wgt = __uint_as_float(rx.y);
        if (wts != nullptr) {
            const uint32_t nw1 = a.n_weights - 1;
            return a.ms * wts[rx.w < nw1 ? rx.w : nw1] * wgt;
        }
        return a.ms * wgt;
    };
    unsigned int pos = width - 1 - rm.w;
    float sum_weight = 0.f;
    int aligned = 0;
    emit(pos);
    aligned++;
    sum_weight = sum_weight + mscore_at(rm, s);

    // value_midx of a cell whose deletion extends the gap of predecessor x: gapm_idx[x][col]
    // (common.h, Ext / OpLast) -- follow last predecessors to the row that opened the gap
    constexpr uint32_t ext_bit = LAZY ? kTb16Ext : kTbExt;
    // predecessor e of the row of x: one of the four that came with it, or its entry in the list
    auto pred_of = [&](const BtAt &x, uint32_t e) -> uint32_t { return e < 4u ? x.pred_near(e) : mem.pred_far(x.r.x, e); };
    // (one round trip per hop: the hop's cell, record and last predecessor arrive together)
    auto gapm_idx = [&](uint32_t x, uint32_t col) -> uint32_t {
        for (uint32_t guard = 0; guard < 65536u; ++guard) {
            const BtAt ax = mem.at(x, col);
            const uint32_t np = ax.npred();
            if (np == 0) return 0u;  // an edge row keeps its initial gapm_idx
            const uint32_t lastp = pred_of(ax, np - 1);
            if (LAZY ? !(ax.c & kTb16XLast) : (ax.c & kTbOpLast) != 0) return lastp;
            x = lastp;
        }
        return 0u;
    };
    // the row the cell x of row `row` points at, before Ext is resolved: stored (32-bit cells), or the
    // row itself / 0 / the predecessor with the stored ordinal (16-bit cells)
    auto midx_raw = [&](const BtAt &x, uint32_t row) -> uint32_t {
        if (!LAZY) return x.c >> 16;
        const uint32_t t = x.c & kTbTypeMask;
        if (t == kTbIns) return row;
        if (t == kTbNone) return 0u;
        return pred_of(x, x.c >> kTb16OrdShift);
    };
    // value_sidx of cell cc = (row, col): stored, or (type-code cells, common.h) what the type implies
    auto sidx_of = [&](uint32_t cc, uint32_t row, uint32_t col) -> uint32_t {
        if (!LAZY) return cc & kTbSMask;
        const uint32_t t = cc & kTbTypeMask;
        if (t == kTbNone) return 0u;
        if (t == kTbMatch) return col - 1;
        if (t == kTbDel) return col;
        uint32_t k = col - 1;  // insertion: the gap began where the run of insertion cells to the left ends
        while (k > 0 && (mem.cell(row, k) & kTbTypeMask) == kTbIns) --k;
        return k;
    };
    auto is_deletion_at = [&](uint32_t cc, uint32_t col) -> bool {  // value_sidx == own column
        return LAZY ? (cc & kTbTypeMask) == kTbDel : (cc & kTbSMask) == col;
    };
    // :642-685 (a source node has no predecessors)
    uint32_t npred_m = rm.z & 0xffu;
    while (s != 0 && npred_m != 0) {
        const uint32_t snew = sidx_of(cur.c, m, s);
        const uint32_t vm = midx_raw(cur, m);
        m = (cur.c & ext_bit) ? gapm_idx(vm, s) : vm;
        // (the record comes with the cell, before the test below decides whether the walk stays on this row: a
        // skipped row's record is dropped unread but for its predecessors)
        cur = mem.at(m, snew);
        if (snew != 0 && is_deletion_at(cur.c, snew)) {  // the one-step deletion skip (:653-655)
            const uint32_t vm2 = midx_raw(cur, m);
            m = (cur.c & ext_bit) ? gapm_idx(vm2, snew) : vm2;
            cur = mem.at(m, snew);
        }
        rm = cur.r;
        npred_m = rm.z & 0xffu;
        pos = width - 1 - rm.w;
        while (s != snew) {
            --s;
            emit(pos);
            aligned++;
            sum_weight = sum_weight + mscore_at(rm, s);
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
    if (mem.writes) a.out[q] = o;
}

template <bool LAZY>
__global__ void __launch_bounds__(64) backtrack_kernel(BtArgs a) {
    __shared__ typename BtWindow<LAZY>::Lds lds;
    const uint32_t q = blockIdx.x;
    if (q >= a.nq) return;
    const QDesc d = a.qd[q];
    BtWindow<LAZY> mem(a, d, lds, threadIdx.x);
    walk_query<LAZY>(a, q, d, mem);
}

// One LANE per query (launches of kBtLanesMin queries and more).  The wave-per-query kernel above spends a whole
// wave's issue slots on one logical thread -- 60 instructions per step, 3000 steps, 9216 waves: 3 ms of a device
// whose other kernels (the next batch's DAG build, k-mer search and DP, running beside it) are bound by instruction
// issue as well.  Here a wave walks 64 queries: 64 times fewer instructions, every look-up a global load of its own
// (cells 2 bytes, a 64-byte sector each: a quarter of the window refills' traffic), and the walk's latency -- one
// round trip per step, the cell's (BtDirect::at), the rare branches of any lane paid by the whole wave -- is hidden
// behind the kernels it runs beside instead of competing with them.
template <bool LAZY>
__global__ void __launch_bounds__(64) backtrack_lanes_kernel(BtArgs a) {
    const uint32_t q = blockIdx.x * 64u + threadIdx.x;
    if (q >= a.nq) return;
    const QDesc d = a.qd[q];
    BtDirect<LAZY> mem(a, d);
    walk_query<LAZY>(a, q, d, mem);
}


// The cseq container steps that follow the cell walk in backtrack() (src/mesh.h:603-726), for the
// queries where they are plain -- one wave per query, behind backtrack_kernel on the same stream:
//   * every emitted base is appended under the container rule (a column left of the sequence's
//     current width is moved up to it, src/cseq.cpp:79-95): a running maximum over the emitted columns;
//   * setWidth(width) + reverse() (:283-289): written back to front, column c -> width - 1 - c;
//   * fix_duplicate_positions (src/cseq.cpp:456-594): bases sharing a column are an
//     insertion; where the free columns up to the next base suffice they are placed right-aligned
//     there (and lower-cased with --lowercase=unaligned).
// SHIFT = false (sina_hip_align_params::assemble == 1) handles that case only.  An insertion
//     that does not fit and makes its neighbours move, a column at or beyond the alignment's width,
//     or more than kAsmMax bases leave out_pos as backtrack_kernel wrote it (assembled = 0): the host
//     finishes those with the container's own code.
// SHIFT = true (assemble == 2, SINA_ASSEMBLE_SHIFT) also places the insertions that do not fit: the
//     reference's widening loop (src/cseq.cpp:503-570; assemble_shift below).  Left to the host there:
//     more than kShiftLog shifted runs, no free column on either side (the reference throws), a
//     column at or beyond the width -- in the input or reached by a widening --, more than kAsmMax bases.
// out_pos is rewritten in place: columns in, packed aligned bases (column | mask << 24) out.
// LDS: 4 bytes per base of the launch's longest query + 1 KB (16S: 7 KB -- what a resident DP kernel
// leaves free on a CU, so the wave runs beside it like backtrack_kernel does).  The same for both: SHIFT
// needs no bitmap of the duplicates and keeps its event row (97 words, 388 bytes) in that bitmap's 512.
constexpr int kAsmMax = 4096;
constexpr uint32_t kShiftLog = SINA_HIP_SHIFT_LOG, kShiftRow = 1 + 3 * kShiftLog;  // events, words of a query's log row

__device__ __forceinline__ uint32_t first_lane_of(unsigned long long m) { return (uint32_t)__ffsll((long long)m) - 1u; }

// The fix-up with widening, over col[0 .. n): the bases' columns in SEQUENCE order, after the append rule and the
// mirror.  The runs are taken left to right as the reference takes them (so_cseq_fix_duplicate_positions,
// oracle/sina_oracle.c, is the same loop with indices): a widening reads the columns earlier runs have left on its
// left and the raw ones, later insertions included, on its right.  Every variable is the wave's (the same in all
// lanes); the lanes share the searches -- 64 positions per ballot -- and the placing.  moved: one bit per base the
// fix-up placed; ev: the event row (word 0 is written by the caller); facts: total, longest, last run.
// Returns the number of events, or 0xFFFFFFFF: the host finishes the query.
__device__ __forceinline__ uint32_t assemble_shift(uint32_t *col, unsigned long long *moved, uint32_t *ev, uint32_t n,
                                                   uint32_t width, uint32_t lane, uint32_t *facts) {
    auto uni = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };
    // the base from which everything up to `from` sits column to column: the largest l <= from with l == 0 or a
    // free column between l - 1 and l
    auto gap_left_of = [&](uint32_t from) -> uint32_t {
        for (uint32_t l = from;; l -= 64) {  // (position 0 stops: l never passes it)
            const int p = (int)l - (int)lane;
            const bool stop = p >= 0 && (p == 0 || col[p - 1] + 1 < col[p]);
            const unsigned long long m = __builtin_amdgcn_ballot_w64(stop);
            if (m != 0ull) return l - first_lane_of(m);
        }
    };
    // ... and to the right: the smallest r >= from with r == n - 1 or a free column between r and r + 1
    auto gap_right_of = [&](uint32_t from) -> uint32_t {
        for (uint32_t r = from;; r += 64) {  // (position n - 1 stops)
            const uint32_t p = r + lane;
            const bool stop = p < n && (p + 1 == n || col[p] + 1 < col[p + 1]);
            const unsigned long long m = __builtin_amdgcn_ballot_w64(stop);
            if (m != 0ull) return r + first_lane_of(m);
        }
    };
    uint32_t total = 0, longest = 0, last_run = 0, nev = 0;
    for (uint32_t anchor = 0;;) {
        // the next insertion: the first j >= anchor that shares its column with j + 1
        uint32_t j = n;
        for (uint32_t b = anchor; b + 1 < n; b += 64) {
            const uint32_t p = b + lane;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(p + 1 < n && col[p] == col[p + 1]);
            if (m != 0ull) {
                j = b + first_lane_of(m);
                break;
            }
        }
        if (j >= n) break;
        const uint32_t c0 = uni(col[j]);
        uint32_t k = n;  // the first base behind the run, or the sequence's end
        for (uint32_t b = j + 2; b < n; b += 64) {
            const uint32_t p = b + lane;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(p < n && col[p] != c0);
            if (m != 0ull) {
                k = b + first_lane_of(m);
                break;
            }
        }
        // bases first .. last go into the free columns [range_begin, range_end)
        uint32_t first = j + 1, last = k - 1, num = k - j - 1;
        uint32_t range_begin = c0 + 1, range_end = k == n ? width : uni(col[k]);
        last_run = num;
        if (range_end - range_begin < num) {
            if (nev == kShiftLog) return 0xFFFFFFFFu;
            if (lane == 0) {
                ev[1 + 3 * nev] = num;
                ev[2 + 3 * nev] = range_begin;
                ev[3 + 3 * nev] = range_end;
            }
            nev++;
            while (range_end - range_begin < num) {  // (each turn gains one free column or gives up)
                int next_left_gap, next_right_gap;
                uint32_t left = first, right = last;
                if (left == 0) {
                    next_left_gap = range_begin > 0 ? (int)(range_begin - 1) : -1;
                } else if (uni(col[left - 1]) + 1 < range_begin) {
                    next_left_gap = (int)(range_begin - 1);
                } else {
                    left = gap_left_of(left - 1);
                    next_left_gap = (int)(uni(col[left]) - 1u);
                }
                if (right + 1 == n) {
                    next_right_gap = range_end < width ? (int)range_end : -1;
                } else if (uni(col[right + 1]) > range_end) {
                    next_right_gap = (int)range_end;
                } else {
                    right = gap_right_of(right + 1);
                    next_right_gap = (int)(uni(col[right]) + 1);
                }
                if (next_right_gap == -1 ||
                    (next_left_gap != -1 && range_begin - (uint32_t)next_left_gap <= (uint32_t)next_right_gap - (range_end - 1))) {
                    if (next_left_gap == -1) return 0xFFFFFFFFu;  // (no space to left and right: the reference throws)
                    num += first - left;
                    range_begin = (uint32_t)next_left_gap;
                    first = left;
                } else {
                    num += right - last;
                    range_end = (uint32_t)next_right_gap + 1;
                    last = right;
                }
            }
            // (a right scan that ends on a last base in column width - 1 takes `width` for a free column, as the
            // reference does: a column the alignment does not have)
            if (range_begin + num > width) return 0xFFFFFFFFu;
        } else {
            range_begin = range_end - num;  // enough room: right-aligned in the free range
        }
        for (uint32_t t = lane; t < num; t += 64) col[first + t] = range_begin + t;
        for (uint32_t w = (first >> 6) + lane; w <= (last >> 6); w += 64) {
            const uint32_t lo = w == (first >> 6) ? (first & 63u) : 0u, hi = w == (last >> 6) ? (last & 63u) : 63u;
            moved[w] |= (~0ull << lo) & (~0ull >> (63u - hi));
        }
        __syncthreads();  // (one wave: the next run's searches read what this one placed)
        total += num;
        longest = max(longest, num);
        anchor = last + 1;
    }
    facts[0] = total;
    facts[1] = longest;
    facts[2] = last_run;
    return nev;
}

template <bool SHIFT>
__global__ void __launch_bounds__(64) assemble_kernel(BtArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char asm_lds[];
    unsigned long long *dupm = reinterpret_cast<unsigned long long *>(asm_lds);  // [kAsmMax / 64]
    unsigned long long *movedm = dupm + kAsmMax / 64;                              // [kAsmMax / 64]
    uint32_t *colm = reinterpret_cast<uint32_t *>(movedm + kAsmMax / 64);          // [a.asm_cap] column of emission i after the append rule
    __shared__ uint32_t facts[4];                                // ok, total, longest, last run
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    if (q >= a.nq) return;
    const QDesc d = a.qd[q];
    const sina_hip_align_out o = a.out[q];
    const uint32_t n = o.n_out, width = a.width;
    if constexpr (SHIFT) {  // (every query's log row is defined: no events unless the fix-up below says otherwise)
        for (uint32_t t = lane; t < kShiftRow; t += 64) a.shift_log[(size_t)q * kShiftRow + t] = 0u;
    }
    if (o.status != 0 || n == 0 || n > a.asm_cap) return;
    uint32_t *pos = a.out_pos + d.q_off;
    const uint8_t *qm = a.qmask + d.q_off;
    const bool keep_over = a.overhang != SINA_OVERHANG_REMOVE;
    const uint32_t tail = keep_over ? (uint32_t)o.cutoff_tail : 0u;
    const uint32_t n_aligned = (uint32_t)o.aligned_bases;
    if constexpr (SHIFT) {
        // ---- append rule as below, stored mirrored and in sequence order: col[n-1-i] = width - 1 - (column of emission i)
        uint32_t *col = colm, *ev = reinterpret_cast<uint32_t *>(dupm);
        uint32_t carry = 0;
        bool beyond = false;
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t i = base + lane;
            uint32_t v = i < n ? pos[i] : 0u;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t y = __shfl_up(v, off);
                if ((int)lane >= off) v = max(v, y);
            }
            v = max(v, carry);
            if (lane == 0) movedm[base >> 6] = 0ull;
            if (i < n) {
                col[n - 1 - i] = width - 1 - v;
                beyond = beyond || v >= width;
            }
            carry = __shfl(v, 63);
        }
        if (__builtin_amdgcn_ballot_w64(beyond) != 0ull) return;
        __syncthreads();
        // ---- the fix-up, widening included
        uint32_t nast[3];  // total, longest, last run
        const uint32_t nev = assemble_shift(col, movedm, ev, n, width, lane, nast);
        if (nev == 0xFFFFFFFFu) return;
        __syncthreads();
        // ---- bases: sequence position j is emission n-1-j
        const uint32_t keep_case = a.lowercase == SINA_LOWERCASE_ORIGINAL ? 0xFFu : 0xEFu;
        const uint32_t lower = a.lowercase == SINA_LOWERCASE_UNALIGNED ? 0x10u : 0u;
        const uint32_t first_q = (uint32_t)o.end_s + tail;  // query index of emission 0
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t j = base + lane;
            if (j >= n) break;
            const uint32_t i = n - 1 - j;
            const bool overhang_base = i < tail || i >= tail + n_aligned;
            const bool moved = (movedm[j >> 6] >> (j & 63)) & 1ull;
            const uint32_t bits = ((uint32_t)qm[first_q - i] & keep_case) | ((overhang_base || moved) ? lower : 0u);
            pos[j] = (col[j] & 0xFFFFFFu) | (bits << 24);
        }
        uint32_t *row = a.shift_log + (size_t)q * kShiftRow;
        for (uint32_t t = lane; t < 1 + 3 * nev; t += 64) row[t] = t == 0 ? nev : ev[t];
        if (lane == 0) {
            sina_hip_align_out *out = a.out + q;
            out->assembled = 1;
            out->nast_total = nast[0];
            out->nast_longest = nast[1];
            out->nast_last_run = nast[2];
        }
        return;
    }
    // ---- append rule: prefix maximum of the emitted columns; equal neighbours are insertions
    uint32_t carry = 0;
    bool beyond = false;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane;
        uint32_t v = i < n ? pos[i] : 0u;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(v, off);
            if ((int)lane >= off) v = max(v, y);
        }
        v = max(v, carry);
        uint32_t prev = __shfl_up(v, 1);
        if (lane == 0) prev = carry;
        const bool dup = i < n && i > 0 && v == prev;
        const unsigned long long dm = __builtin_amdgcn_ballot_w64(dup);
        if (lane == 0) {
            dupm[base >> 6] = dm;
            movedm[base >> 6] = 0ull;
        }
        if (i < n) {
            colm[i] = v;
            beyond = beyond || v >= width;
        }
        carry = __shfl(v, 63);
    }
    const bool any_beyond = __builtin_amdgcn_ballot_w64(beyond) != 0ull;
    __syncthreads();
    // ---- insertions that fit their gap (one lane: a handful of runs per query)
    if (lane == 0) {
        uint32_t total = 0, longest = 0, last_run = 0, ok = any_beyond ? 0u : 1u;
        bool first = true;
        uint32_t i = 1;
        while (ok && i < n) {
            const unsigned long long word = dupm[i >> 6] >> (i & 63);
            if (word == 0ull) {
                i = ((i >> 6) + 1) << 6;
                continue;
            }
            i += (uint32_t)__ffsll((long long)word) - 1u;  // emission i shares its column with i-1
            const uint32_t i0 = i - 1;                      // first emission of the run = its LAST base in sequence order
            uint32_t r = 0;                                 // bases to place: emissions i0 .. i0+r-1 (i0+r stays: the anchor)
            while (i < n && ((dupm[i >> 6] >> (i & 63)) & 1ull)) {
                r++;
                i++;
            }
            const uint32_t anchor_col = width - 1 - colm[i0];
            const uint32_t next_col = i0 > 0 ? width - 1 - colm[i0 - 1] : width;  // the next base in sequence order, or the end
            if (next_col - (anchor_col + 1) < r) {  // does not fit: neighbours would have to move
                ok = 0;
                break;
            }
            for (uint32_t t = 0; t < r; t++) {  // right-aligned in the gap: emission i0 next to next_col
                colm[i0 + t] = width - next_col + t;
                movedm[(i0 + t) >> 6] |= 1ull << ((i0 + t) & 63);
            }
            total += r;
            longest = max(longest, r);
            if (first) last_run = r;  // (the host walks the sequence left to right: its last run is the first one here)
            first = false;
        }
        facts[0] = ok;
        facts[1] = total;
        facts[2] = longest;
        facts[3] = last_run;
    }
    __syncthreads();
    if (!facts[0]) return;
    // ---- reverse + bases: sequence position n-1-i <- emission i
    const uint32_t keep_case = a.lowercase == SINA_LOWERCASE_ORIGINAL ? 0xFFu : 0xEFu;
    const uint32_t lower = a.lowercase == SINA_LOWERCASE_UNALIGNED ? 0x10u : 0u;
    const uint32_t first_q = (uint32_t)o.end_s + tail;  // query index of emission 0
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane;
        if (i >= n) break;
        const bool overhang_base = i < tail || i >= tail + n_aligned;
        const bool moved = (movedm[i >> 6] >> (i & 63)) & 1ull;
        const uint32_t bits = ((uint32_t)qm[first_q - i] & keep_case) | ((overhang_base || moved) ? lower : 0u);
        pos[n - 1 - i] = ((width - 1 - colm[i]) & 0xFFFFFFu) | (bits << 24);
    }
    if (lane == 0) {
        sina_hip_align_out *out = a.out + q;
        out->assembled = 1;
        out->nast_total = facts[1];
        out->nast_longest = facts[2];
        out->nast_last_run = facts[3];
    }
}

}  // namespace

int launch_assemble(const BtArgs &a0, hipStream_t s) {
    BtArgs a = a0;
    a.asm_cap = std::min<uint32_t>((a.asm_cap + 63u) & ~63u, (uint32_t)kAsmMax);  // (longer queries: the host finishes them)
    const size_t lds = 2 * (size_t)(kAsmMax / 64) * 8 + 4 * (size_t)a.asm_cap;
    static_assert(kShiftRow * 4 <= (kAsmMax / 64) * 8, "the event row lives in the duplicates' bitmap");
    // (shift_log: the launch's [nq][kShiftRow] log rows -- assemble = 2 --, or nullptr)
    if (a.shift_log != nullptr) hipLaunchKernelGGL(assemble_kernel<true>, dim3(a.nq), dim3(64), lds, s, a);
    else hipLaunchKernelGGL(assemble_kernel<false>, dim3(a.nq), dim3(64), lds, s, a);
    SH_CHECK(hipGetLastError());
    return 0;
}

// Lanes or waves: bt_by_lanes (dp_plan.h); SINA_HIP_TEST=bt_lanes=0/1 forces one.
int launch_backtrack(const BtArgs &a, hipStream_t s) {
    const std::string e = test_knob("bt_lanes");
    if (bt_by_lanes(a.nq, a.asm_cap, e.empty() ? -1 : (atoi(e.c_str()) != 0 ? 1 : 0))) {
        if (a.lazy_sidx) hipLaunchKernelGGL(backtrack_lanes_kernel<true>, dim3((a.nq + 63u) / 64u), dim3(64), 0, s, a);
        else hipLaunchKernelGGL(backtrack_lanes_kernel<false>, dim3((a.nq + 63u) / 64u), dim3(64), 0, s, a);
    } else if (a.lazy_sidx) hipLaunchKernelGGL(backtrack_kernel<true>, dim3(a.nq), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(backtrack_kernel<false>, dim3(a.nq), dim3(64), 0, s, a);
    SH_CHECK(hipGetLastError());
    return 0;
}

}  // namespace sina_hip
