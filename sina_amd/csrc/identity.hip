// --calc-idty where the device assembles the alignment: family_identity_kernel +
// sina_hip_align_count_identity, sina_hip_staged_identity, sina_hip_identity_inplace_stats.  Launched by dp_launch.hip
// (launch_inplace_counts) behind assemble_kernel; its switch, rows and event are the context's
// inplace[kInplaceIdentity], its counters use[kUseIdentityInplace] (ctx.h).  The tables and the classification are
// compare_dev.h's, shared with search.hip and rank.hip.
//
// What it computes: for every query of a DP launch range that the device assembled, the best overlap identity of its
// finished sequence with a member of its family (align_ident_slv, src/align.cpp:443-453: cseq_comparator(
// CMP_IUPAC_OPTIMISTIC, CMP_DIST_NONE, CMP_COVER_OVERLAP, false) over every member, the maximum kept), and the number
// of members that had a score at all.  The factor 100 stays with the host: two words per query cross back.
//
// How it maps to the hardware: one workgroup of kCT threads per query.  It builds the query's column bitmap, running
// counts and mask bytes in LDS (build_query_tables: up to 106 KB at 524 288 columns), then its four waves stride over
// the family's members in list order, each streaming one member's packed bases from the store against the tables
// (classify_candidate).  A wave keeps the maximum of its members' score bits and their number in registers -- scores
// are never negative, so the order of the bit patterns is the order of the floats --, the four waves meet in LDS and
// thread 0 stores the row.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "ctx.h"
#include "compare_dev.h"
#include "identity_plan.h"

namespace sina_hip {
namespace {

static_assert(kIdentityThreads == (uint32_t)kCT, "identity_plan.h and compare_dev.h disagree on the workgroup");
static_assert(kIdentityMaxLds == kCompareMaxLds, "identity_plan.h and compare_dev.h disagree on the LDS ceiling");
static_assert(identity_lds_bytes(1, 1) == compare_table_bytes(1, 1) && identity_lds_bytes(33, 17) == compare_table_bytes(33, 17) &&
                  identity_lds_bytes(524288, 10240) == compare_table_bytes(524288, 10240),
              "identity_plan.h and compare_dev.h disagree on the tables' size");

struct IdentityArgs {
    const QDesc *qd;
    const sina_hip_align_out *out;
    const uint32_t *out_pos;
    const uint32_t *ref_ab;    // the store's packed references
    const uint64_t *ref_off;
    const uint32_t *fam_ids;   // the build chunk's distinct families, concatenated ...
    const uint64_t *fam_off;   // ... and their offsets, relative to the chunk
    uint32_t *rows;            // [n][2]: best score (float bits), members that scored
    uint32_t n, width, n_refs;
    uint32_t ncap;             // node entries per DAG of the chunk's build
    uint32_t max_l;            // longest query of the range: the tables' mask bytes
};

// Which list is the query's: the chunk's lists are those of its DISTINCT families (dp_plan.h, distinct_families), so
// the query's own index does not find it.  Its DAG's number does, and that is derived as the scout preamble of the DP
// wave derives it (mesh_dp.hip): the builders lay DAG u's node arrays at u * ncap, and the query's descriptor holds
// that offset -- no side array, nothing more to upload.
__global__ void __launch_bounds__(kCT) family_identity_kernel(IdentityArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_tmp[8];
    __shared__ uint32_t s_scal[3];
    __shared__ uint32_t s_best[kCT / 64], s_scored[kCT / 64];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    if (q >= a.n) return;
    const int lane = tid & 63, wave = tid >> 6;
    const sina_hip_align_out *o = a.out + q;
    uint32_t *row = a.rows + (size_t)q * 2;
    const uint32_t la = o->n_out;
    // (the same for every thread of the workgroup; la > max_l cannot happen for an assembled query -- assemble_kernel
    // leaves a longer one alone -- and would overrun the mask bytes.  An assembled query's columns ascend strictly and
    // lie below the width, shifted insertions included: assemble_kernel<true> places them into free columns only)
    if (o->status != 0 || o->assembled == 0 || la > a.max_l) {
        if (tid < 2) row[tid] = 0;
        return;
    }
    const QDesc d = a.qd[q];
    // calc-idty does not filter lower case: lc_bit = 0
    const QueryTables t = build_query_tables(smem, s_tmp, s_scal, a.out_pos + d.q_off, la, a.width, 0u);

    const uint32_t dag = (uint32_t)(d.node_off / a.ncap);
    const uint64_t m0 = a.fam_off[dag], m1 = a.fam_off[dag + 1];
    uint32_t best = 0, scored = 0;
    for (uint64_t x = m0 + wave; x < m1; x += kCT / 64) {
        const uint32_t id = a.fam_ids[x];
        const bool valid = id < a.n_refs;  // (the build checked the ids)
        const uint32_t *Bp = valid ? a.ref_ab + a.ref_off[id] : nullptr;
        const uint32_t lb = valid ? (uint32_t)(a.ref_off[id + 1] - a.ref_off[id]) : 0u;
        const sina_hip_match_counts m = classify_candidate(t, Bp, lb, valid, 0u, SINA_CMP_IUPAC_OPTIMISTIC, lane);
        const int32_t denom = cover_denominator(m, SINA_CMP_COVER_OVERLAP);
        if (denom == 0) continue;  // the host's NaN: std::max(idty, NaN) keeps idty
        best = max(best, __float_as_uint(__fdiv_rn((float)m.match, (float)denom)));
        scored++;
    }
    // (every lane of a wave holds the wave's values: classify_candidate reduces across lanes)
    if (lane == 0) {
        s_best[wave] = best;
        s_scored[wave] = scored;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kCT / 64; w++) {
            best = max(best, s_best[w]);
            scored += s_scored[w];
        }
        row[0] = best;
        row[1] = scored;
    }
}

}  // namespace

int launch_family_identity(sina_hip_ctx *c, const BtArgs &b, uint32_t ncap, uint32_t max_l, uint32_t *rows, hipStream_t s) {
    if (b.nq == 0) return 0;
    if (ncap == 0) SH_FAIL("family identity: the launch has no device-built families");
    const size_t lds = identity_lds_bytes(b.width, max_l);
    if (lds > kIdentityMaxLds) SH_FAIL_LIMIT("family identity: alignment too wide for the device comparison");
    IdentityArgs a;
    a.qd = b.qd;
    a.out = b.out;
    a.out_pos = b.out_pos;
    a.ref_ab = c->st->ref_ab.as<uint32_t>();
    a.ref_off = c->st->ref_off.as<uint64_t>();
    a.fam_ids = c->g_fam_ids.as<uint32_t>();
    a.fam_off = c->g_fam_off.as<uint64_t>();
    a.rows = rows;
    a.n = b.nq;
    a.width = b.width;
    a.n_refs = c->st->n_refs;
    a.ncap = ncap;
    a.max_l = max_l;
    if (allow_full_lds(reinterpret_cast<const void *>(family_identity_kernel))) return 1;
    hipLaunchKernelGGL(family_identity_kernel, dim3(identity_grid(b.nq)), dim3(kCT), lds, s, a);
    SH_CHECK(hipGetLastError());
    return 0;
}

}  // namespace sina_hip

using namespace sina_hip;

extern "C" int sina_hip_align_count_identity(sina_hip_ctx *c, int on) {
    if (!c) SH_FAIL("align_count_identity: null ctx");
    std::lock_guard<std::mutex> lk(c->mu);
    c->inplace[kInplaceIdentity].on = on != 0;
    return 0;
}

extern "C" const uint32_t *sina_hip_staged_identity(sina_hip_ctx *c) {
    if (!c) {
        set_error("staged_identity: null ctx");
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    return c->inplace[kInplaceIdentity].staged();
}

extern "C" int sina_hip_identity_inplace_stats(sina_hip_ctx *c, double *kernel_ms, uint64_t *sequences, uint64_t *pairs, uint64_t *launches) {
    if (!c || !kernel_ms || !sequences || !pairs || !launches) SH_FAIL("identity_inplace_stats: null argument");
    return read_use(c, kUseIdentityInplace, kernel_ms, sequences, pairs, launches);
}
