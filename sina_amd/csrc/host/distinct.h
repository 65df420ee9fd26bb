// Batch-level memoisation of repeated items: which items of a batch are equal, the distinct ones' offsets, and their
// bytes gathered for the device.  Header-only; no HIP, no stages.h, no globals: a stand-alone program can include it
// (tests/distinct_check.cpp).  Whether grouping is on and the parallel loop to use are the caller's to pass.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

// (hidden: a shared library that includes this exports none of it)
namespace sina __attribute__((visibility("hidden"))) {

// The big per-batch arrays of a stage call (packed queries, aligned columns coming back: tens of MB): a
// std::vector of that size is a fresh mmap every batch -- zero-filled by the kernel page by page, then
// zero-filled again by the constructor -- 46 MB and 11 000 page faults per 6144-query batch.  One grow-only,
// uninitialised block per calling thread and use instead.  (Not hidden with the rest: the host library's exported
// names have its destructors among them.)
template <typename T> struct __attribute__((visibility("default"))) batch_scratch {
    T *p = nullptr;
    size_t cap = 0;
    T *get(size_t n) {
        if (n > cap) {
            free(p);
            cap = n + n / 4 + 1024;
            p = static_cast<T *>(malloc(cap * sizeof(T)));
            if (!p) {
                cap = 0;
                throw std::bad_alloc();
            }
        }
        return p;
    }
    ~batch_scratch() { free(p); }
    batch_scratch() = default;
    batch_scratch(const batch_scratch &) = delete;
    batch_scratch &operator=(const batch_scratch &) = delete;
};

inline uint64_t hash_bytes(const void *p, size_t n, uint64_t seed) {  // (FNV-1a over 8-byte words + tail)
    const unsigned char *b = static_cast<const unsigned char *>(p);
    uint64_t h = 0xcbf29ce484222325ull ^ seed;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t w;
        memcpy(&w, b + i, 8);
        h = (h ^ w) * 0x100000001b3ull;
        h ^= h >> 29;
    }
    for (; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h ^ (h >> 32);
}
// hash of a query's mask bytes for the grouping of repeats: its two ends (64 bytes each) and its length.  Equal
// queries hash equal; unequal ones that agree there are told apart by the byte comparison that follows a hash match
// -- hashing all 1500 bytes, in famfinder and again in the aligner, was 0.4 us per query.
inline uint64_t hash_ends(const void *p, size_t n, uint64_t seed) {
    if (n <= 160) return hash_bytes(p, n, seed);
    const unsigned char *b = static_cast<const unsigned char *>(p);
    return hash_bytes(b + n - 64, 64, hash_bytes(b, 64, seed ^ n));
}

// The reference's kmer_search::find keeps the scored list of the base strings it has just seen
// (src/kmer_search.cpp:105,377-378,419: a cache of 32 keyed by getBases()) -- real amplicon runs are dominated by
// repeats.  A GPU batch is thousands of queries wide, so the analogue is inside the batch: items with the same key
// bytes (and, for the aligner, the same family) go to the device ONCE, and every item reads the slot of its first
// occurrence.  rep[i] = index of the first item equal to item i; returns the number of distinct items.  `on` false:
// every item is its own (tests compare both ways).  The hashes are computed through par_for(n, fn).
template <class ParFor, class Hash, class Equal>
size_t group_equal_items(bool on, ParFor &&par_for, size_t n, Hash &&hash_of, Equal &&equal, std::vector<uint32_t> &rep) {
    rep.resize(n);
    if (!on || n < 2) {
        for (size_t i = 0; i < n; i++) rep[i] = (uint32_t)i;
        return n;
    }
    std::vector<uint64_t> h(n);
    par_for(n, [&](size_t i) { h[i] = hash_of(i); });
    // open addressing over the first occurrences (a batch is a few thousand items)
    size_t cap = 16;
    while (cap < 2 * n) cap <<= 1;
    std::vector<uint32_t> slot(cap, 0xFFFFFFFFu);
    size_t distinct = 0;
    for (size_t i = 0; i < n; i++) {
        size_t at = (size_t)(h[i] * 0x9E3779B97F4A7C15ull >> 20) & (cap - 1);
        for (;;) {
            const uint32_t j = slot[at];
            if (j == 0xFFFFFFFFu) {
                slot[at] = (uint32_t)i;
                rep[i] = (uint32_t)i;
                distinct++;
                break;
            }
            if (h[j] == h[i] && equal(j, i)) {
                rep[i] = j;
                break;
            }
            at = (at + 1) & (cap - 1);
        }
    }
    return distinct;
}

// What the device is given of a batch with repeats: one slot per distinct item, in order of first occurrence.
struct distinct_items {
    size_t n = 0;                   // number of distinct items
    std::vector<uint32_t> slot_of;  // [items] slot of item i
    std::vector<uint32_t> first;    // [n] first item of slot u; empty if nothing repeats (slot u is item u)
    std::vector<uint64_t> off;      // [n + 1] slot u's elements start at off[u]
};

// Takes rep and the number of distinct items (group_equal_items) and the items' offsets [items + 1]; gives the slots.
inline distinct_items slots_of_rep(const std::vector<uint32_t> &rep, size_t n_distinct, const uint64_t *item_off) {
    const size_t n = rep.size();
    distinct_items d;
    d.n = n_distinct;
    d.slot_of.resize(n);
    if (n_distinct == n) {
        for (size_t i = 0; i < n; i++) d.slot_of[i] = (uint32_t)i;
        d.off.assign(item_off, item_off + n + 1);
        return d;
    }
    d.first.reserve(n_distinct);
    d.off.assign(n_distinct + 1, 0);
    for (size_t i = 0; i < n; i++) {
        if (rep[i] == i) {
            d.slot_of[i] = (uint32_t)d.first.size();
            d.off[d.first.size() + 1] = d.off[d.first.size()] + (item_off[i + 1] - item_off[i]);
            d.first.push_back((uint32_t)i);
        } else {
            d.slot_of[i] = d.slot_of[rep[i]];
        }
    }
    return d;
}

// (no extra key: every item has the same one)
struct same_key {
    uint64_t operator()(size_t) const { return 0; }
    bool operator()(size_t, size_t) const { return true; }
};

// Takes n items, item i the item_off[i + 1] - item_off[i] elements of T at base + item_off[i]; gives the slots of the
// distinct ones: equal length and equal bytes -- and, where the caller has more to an item than its bytes, an equal
// extra key: key_seed(i) goes into item i's hash, same_key(a, b) says whether two items' keys are equal.
template <typename T, class ParFor, class Seed = same_key, class Same = same_key>
distinct_items distinct_spans(bool on, ParFor &&par_for, const T *base, const uint64_t *item_off, size_t n, Seed &&key_seed = Seed(),
                              Same &&same_key_of = Same()) {
    auto len = [&](size_t i) { return item_off[i + 1] - item_off[i]; };
    std::vector<uint32_t> rep;
    const size_t n_distinct = group_equal_items(
        on, par_for, n, [&](size_t i) { return hash_ends(base + item_off[i], sizeof(T) * len(i), key_seed(i) ^ len(i)); },
        [&](size_t a, size_t b) {
            return len(a) == len(b) && same_key_of(a, b) && memcmp(base + item_off[a], base + item_off[b], sizeof(T) * len(a)) == 0;
        },
        rep);
    return slots_of_rep(rep, n_distinct, item_off);
}

// Takes the slots, the items' elements and offsets and a scratch block; gives the distinct items' elements, slot u at
// d.off[u], to hand to the device.  Nothing repeats: that is src itself -- nothing is copied, dst is not touched.
template <typename T, class ParFor>
const T *gather_distinct(const distinct_items &d, ParFor &&par_for, const T *src, const uint64_t *item_off, batch_scratch<T> &dst) {
    if (d.first.empty()) return src;
    T *const out = dst.get(d.off.back() + 1);
    par_for(d.n, [&](size_t u) { memcpy(out + d.off[u], src + item_off[d.first[u]], sizeof(T) * (d.off[u + 1] - d.off[u])); });
    return out;
}

}  // namespace sina
