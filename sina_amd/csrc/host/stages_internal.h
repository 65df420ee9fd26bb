// What the host stages' translation units share among themselves (profile.cpp, store.cpp, famfinder.cpp,
// family_graph.cpp, aligner.cpp, search_filter.cpp): declarations, and the templates inline.  stages.h stays the one
// public header -- capi.cpp, rw_fasta.cpp and sidx.cpp do not include this one.
#pragma once

#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "stages.h"
#include "distinct.h"

// (hidden: the host library exports none of it)
namespace sina __attribute__((visibility("hidden"))) {

inline void hip_check(int rc, const char *what) {
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + sina_hip_last_error());
}

// ---------------------------------------------------------------- phase profiler (profile.cpp)
// user + kernel CPU seconds, kernel seconds alone and minor page faults of the calling thread so far
struct thread_use {
    double cpu = 0, sys = 0, faults = 0;
};
// a named phase of the calling thread, on its stack (SINA_HOST_PROFILE / SINA_HOST_TRACE; host_phase is its public twin)
struct scoped_phase {
    const char *name;
    const char *outer;
    thread_use use0;
    std::chrono::steady_clock::time_point t0;
    explicit scoped_phase(const char *n);
    ~scoped_phase();
    scoped_phase(const scoped_phase &) = delete;
};

// ---------------------------------------------------------------- options (famfinder.cpp)
bool to_bool(const std::string &v);
std::string lower(std::string s);
const std::string &famfinder_database();  // famfinder's "db" as it stands: what the aligner falls back to without its own

// ---------------------------------------------------------------- packing a batch's sequences for the device
bool dedup_enabled();  // set_batch_dedup (store.cpp)

// Takes n sequences seq_of(x) and where each starts, qoff [n + 1] (offsets_of); writes sequence x's mask bytes to
// dst + qoff[x] (an unaligned query's as its reader left them; case is kept).  then(x, bytes, n_bytes), if given, sees
// every sequence's bytes right after they are written, in the same pass.
template <class SeqOf, class Then = void (*)(size_t, const uint8_t *, size_t)>
static void pack_masks(size_t n, SeqOf &&seq_of, const uint64_t *qoff, uint8_t *dst, Then &&then = [](size_t, const uint8_t *, size_t) {}) {
    static_assert(sizeof(aligned_base) == 4, "packed words");
    parallel_for(n, [&](size_t x) {
        const cseq &c = seq_of(x);
        const size_t nb = c.size();
        if (const uint8_t *dense = c.denseMasks()) memcpy(dst + qoff[x], dense, nb);
        else masks_of_packed(dst + qoff[x], c.packed(), nb);
        then(x, dst + qoff[x], nb);
    });
}
// The same, as packed aligned bases (a dense query's: base i in column i).
template <class SeqOf> static void pack_words(size_t n, SeqOf &&seq_of, const uint64_t *qoff, uint32_t *dst) {
    parallel_for(n, [&](size_t x) {
        const cseq &c = seq_of(x);
        if (const uint8_t *dense = c.denseMasks()) packed_of_masks(dst + qoff[x], dense, c.size());
        else memcpy(dst + qoff[x], c.packed(), 4 * (size_t)c.size());
    });
}
// Takes n sequences; gives qoff [n + 1], qoff[x + 1] - qoff[x] the number of bases of sequence x.
template <class SeqOf> static std::vector<uint64_t> offsets_of(size_t n, SeqOf &&seq_of) {
    std::vector<uint64_t> qoff(n + 1, 0);
    for (size_t x = 0; x < n; x++) qoff[x + 1] = qoff[x] + seq_of(x).size();
    return qoff;
}

// true if the sequence's columns ascend strictly (what the device's match count asks of a query)
inline bool columns_ascend(const cseq &c) {
    if (c.denseMasks()) return true;  // (base i in column i)
    const uint32_t *ab = c.packed();
    for (size_t i = 1, n = c.size(); i < n; i++)
        if ((ab[i] & 0xFFFFFFu) <= (ab[i - 1] & 0xFFFFFFu)) return false;
    return true;
}

// ---------------------------------------------------------------- one comparison launch (aligner: calc-idty; search_filter)
// Takes n aligned sequences seq_of(x) and for each the n_ids_of(x) reference ids that put_ids(x, dst) writes, packs both and
// compares them in ONE launch; gives the counters of sequence x against its candidate r at counts[coff[x] + r].
struct pair_counts {
    std::vector<uint64_t> coff;
    std::vector<sina_hip_match_counts> counts;
};
template <class SeqOf, class NIdsOf, class PutIds>
static pair_counts compare_packed(sina_hip_ctx *ctx, size_t n, SeqOf &&seq_of, NIdsOf &&n_ids_of, PutIds &&put_ids, int iupac_rule,
                                  int filter_lowercase) {
    pair_counts pc;
    const std::vector<uint64_t> qoff = offsets_of(n, seq_of);
    pc.coff.assign(n + 1, 0);
    for (size_t x = 0; x < n; x++) pc.coff[x + 1] = pc.coff[x] + n_ids_of(x);
    std::vector<uint32_t> qab(qoff.back() ? qoff.back() : 1), cids(pc.coff.back() ? pc.coff.back() : 1);
    for (size_t x = 0; x < n; x++) {
        const cseq &c = seq_of(x);
        memcpy(qab.data() + qoff[x], c.packed(), 4 * (size_t)c.size());
        put_ids(x, cids.data() + pc.coff[x]);
    }
    pc.counts.resize(pc.coff.back() ? pc.coff.back() : 1);
    hip_check(sina_hip_compare(ctx, qab.data(), qoff.data(), (uint32_t)n, cids.data(), pc.coff.data(), iupac_rule, filter_lowercase,
                               pc.counts.data()),
              "sina_hip_compare");
    return pc;
}

}  // namespace sina
