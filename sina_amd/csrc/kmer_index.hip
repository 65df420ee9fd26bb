// What the reference store holds for the k-mer search: the CSR index -- built on the device (sina_hip_build_index) or
// brought by the caller (sina_hip_upload_index / sina_hip_download_index) -- and the dense posting lists' bitmaps the
// count kernels read (ensure_dense).  What a k-mer is and what the index holds: kmer.hip's header comment.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.h"
#include "ctx.h"

namespace sina_hip {
namespace {

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

// The build's scratch: released when the build ends, however it ends.  (DevBuf has no destructor -- the context's and
// the store's are long-lived and freed by free_all.)
struct BuildScratch {
    DevBuf keys_in, keys_out, flag, pos, counts, tmp;
    ~BuildScratch() {
        for (DevBuf *b : {&keys_in, &keys_out, &flag, &pos, &counts, &tmp}) b->release();
    }
};
// rocPRIM's calls come in pairs: the size of the temporary storage, then -- if there is anything to do -- the run
// (only the bits a key can have: k-mer << 32 | reference id)
bool sort_keys(DevBuf &tmp, uint64_t *in, uint64_t *out, size_t n, unsigned end_bit, hipStream_t s) {
    size_t tb = 0;
    return rocprim::radix_sort_keys(nullptr, tb, in, out, n, 0u, end_bit, s) == hipSuccess && tmp.reserve(tb + 16) == 0 &&
           (n == 0 || rocprim::radix_sort_keys(tmp.p, tb, in, out, n, 0u, end_bit, s) == hipSuccess);
}
bool exclusive_sum(DevBuf &tmp, uint32_t *in, uint32_t *out, size_t n, hipStream_t s) {
    size_t tb = 0;
    return rocprim::exclusive_scan(nullptr, tb, in, out, 0u, n, rocprim::plus<uint32_t>(), s) == hipSuccess && tmp.reserve(tb + 16) == 0 &&
           (n == 0 || rocprim::exclusive_scan(tmp.p, tb, in, out, 0u, n, rocprim::plus<uint32_t>(), s) == hipSuccess);
}

// keys of every window -> sorted -> first occurrences flagged and numbered -> ids scattered, lists counted -> offsets
bool build_index(sina_hip_ctx *c, unsigned k, int nofast) {
    sina_hip_store *st = c->st;
    hipStream_t s = c->stream;
    const uint64_t n = st->total_bases, nk = 1ull << (2 * k);
    BuildScratch b;
    if (b.keys_in.reserve(8 * std::max<uint64_t>(n, 1)) || b.keys_out.reserve(8 * std::max<uint64_t>(n, 1)) ||
        b.flag.reserve(4 * std::max<uint64_t>(n, 1)) || b.pos.reserve(4 * std::max<uint64_t>(n, 1)))
        return false;
    if (st->n_refs)
        hipLaunchKernelGGL(ref_kmer_keys, dim3(st->n_refs), dim3(256), 0, s, st->ref_ab.as<uint32_t>(), st->ref_off.as<uint64_t>(),
                           st->n_refs, k, nofast == 0, b.keys_in.as<uint64_t>());
    if (!sort_keys(b.tmp, b.keys_in.as<uint64_t>(), b.keys_out.as<uint64_t>(), (size_t)n, 32u + 2u * k, s)) return false;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (n) hipLaunchKernelGGL(mark_unique, dim3(blocks), dim3(256), 0, s, b.keys_out.as<uint64_t>(), n, b.flag.as<uint32_t>());
    if (!exclusive_sum(b.tmp, b.flag.as<uint32_t>(), b.pos.as<uint32_t>(), (size_t)n, s)) return false;
    uint32_t last_flag = 0, last_pos = 0;
    if (n && (hipMemcpyAsync(&last_flag, b.flag.as<uint32_t>() + (n - 1), 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
              hipMemcpyAsync(&last_pos, b.pos.as<uint32_t>() + (n - 1), 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
              hipStreamSynchronize(s) != hipSuccess))
        return false;
    const uint64_t np = (uint64_t)last_flag + last_pos;
    if (b.counts.reserve(4 * (nk + 1)) || st->idx_off.reserve(4 * (nk + 1)) || st->idx_ids.reserve(4 * std::max<uint64_t>(np, 1)))
        return false;
    if (hipMemsetAsync(b.counts.p, 0, 4 * (nk + 1), s) != hipSuccess) return false;
    if (n)
        hipLaunchKernelGGL(scatter_unique, dim3(blocks), dim3(256), 0, s, b.keys_out.as<uint64_t>(), b.flag.as<uint32_t>(),
                           b.pos.as<uint32_t>(), n, st->idx_ids.as<uint32_t>(), b.counts.as<uint32_t>());
    if (!exclusive_sum(b.tmp, b.counts.as<uint32_t>(), st->idx_off.as<uint32_t>(), (size_t)(nk + 1), s) ||
        hipStreamSynchronize(s) != hipSuccess)
        return false;
    st->k = k;
    st->nofast = nofast ? 1 : 0;
    st->n_postings = np;
    st->have_index = true;
    st->dense_ready = false;
    return true;
}

}  // namespace

int index_ready(sina_hip_ctx *c) {
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
int ensure_dense(sina_hip_ctx *c) {
    sina_hip_store *st = c->st;
    std::lock_guard<std::mutex> lk(st->aux_mu);
    if (st->dense_ready) return 0;
    hipStream_t s = c->stream;
    const uint32_t nk = 1u << (2 * st->k);
    uint32_t div_ = 64;
    if (const std::string e_ = test_knob("dense_div"); !e_.empty()) div_ = (uint32_t)std::max(1, atoi(e_.c_str()));
    const uint32_t thresh = kmer_dense_threshold(st->n_refs, div_);
    st->dense_words = kmer_dense_words(st->n_refs);
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
        // (one row more than lists: row nd stays all zero -- no k-mer's, dense_id never names it, n_dense does not count
        // it; the count kernels pad a query's bitmap numbers to a multiple of eight with it)
        const size_t bytes = 4 * ((size_t)nd + 1) * st->dense_words;
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
    if (c->st->total_bases >= (1ull << 32)) SH_FAIL("build_index: more than 2^32 reference bases");
    if (build_index(c, k, nofast)) return 0;
    set_error(std::string("build_index failed: ") + hipGetErrorString(hipGetLastError()));
    return 1;
}

}  // extern "C"
