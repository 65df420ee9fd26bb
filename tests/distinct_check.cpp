// csrc/host/distinct.h -- which items of a batch are equal, the distinct ones' offsets and their gathered bytes --
// against an O(n^2) first-occurrence grouping, as a stand-alone program: tests/test_distinct_cpu.py builds it with the
// address and undefined-behaviour sanitizers and runs it once.  The "parallel for" is a plain serial loop.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "host/distinct.h"

using namespace sina;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            fails++;                                                  \
        }                                                             \
    } while (0)

static void serial_for(size_t n, const std::function<void(size_t)> &fn) {
    for (size_t i = 0; i < n; i++) fn(i);
}

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t rnd(uint32_t below) {  // (xorshift64*)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % below;
}

// a batch: item i is the off[i + 1] - off[i] elements at data + off[i] (one spare element: data is never null)
template <typename T> struct batch {
    std::vector<T> data{T(0)};
    std::vector<uint64_t> off{0};
    size_t n() const { return off.size() - 1; }
    void add(const std::vector<T> &item) {
        data.insert(data.end() - 1, item.begin(), item.end());
        off.push_back(off.back() + item.size());
    }
    bool equal(size_t a, size_t b) const {
        if (off[a + 1] - off[a] != off[b + 1] - off[b]) return false;
        for (uint64_t k = 0; k < off[a + 1] - off[a]; k++)
            if (data[off[a] + k] != data[off[b] + k]) return false;
        return true;
    }
};

// The plain grouping: item i belongs to the first earlier item that is equal to it (`same` adds the extra key), and
// the distinct items are numbered in order of first occurrence.  Checks d, and the gathered elements, against it.
template <typename T, class Same> static void check(const batch<T> &b, const distinct_items &d, const T *dev, const batch_scratch<T> &dst, Same &&same) {
    const size_t n = b.n();
    std::vector<uint32_t> slot_of(n), first;
    std::vector<uint64_t> off{0};
    for (size_t i = 0; i < n; i++) {
        size_t j = 0;
        while (j < i && !(b.equal(j, i) && same(j, i))) j++;
        if (j < i) {
            slot_of[i] = slot_of[j];
        } else {
            slot_of[i] = (uint32_t)first.size();
            first.push_back((uint32_t)i);
            off.push_back(off.back() + (b.off[i + 1] - b.off[i]));
        }
    }
    EXPECT(d.n == first.size());
    EXPECT(d.slot_of == slot_of);
    EXPECT(d.off == off);
    if (first.size() == n) {  // nothing repeats: the input is handed on, nothing is allocated or written
        EXPECT(d.first.empty());
        EXPECT(dev == b.data.data());
        EXPECT(dst.p == nullptr && dst.cap == 0);
    } else {
        EXPECT(d.first == first);
        EXPECT(dev == dst.p && dev != b.data.data());
        for (size_t u = 0; u < first.size() && dev == dst.p; u++)
            EXPECT(memcmp(dev + off[u], b.data.data() + b.off[first[u]], sizeof(T) * (off[u + 1] - off[u])) == 0);
    }
}

static bool always(size_t, size_t) { return true; }

// distinct_spans + gather_distinct on a batch without an extra key, checked; returns the number of distinct items
template <typename T> static size_t run(const batch<T> &b, bool on = true) {
    const distinct_items d = distinct_spans(on, serial_for, b.data.data(), b.off.data(), b.n());
    batch_scratch<T> dst;
    const T *dev = gather_distinct(d, serial_for, b.data.data(), b.off.data(), dst);
    if (on) {
        check(b, d, dev, dst, always);
    } else {  // grouping switched off: the identity
        EXPECT(d.n == b.n() && d.first.empty() && d.off == b.off && dev == b.data.data() && dst.cap == 0);
        for (size_t i = 0; i < b.n(); i++) EXPECT(d.slot_of[i] == i);
    }
    return d.n;
}

template <typename T> static std::vector<T> random_item(uint32_t max_len, uint32_t alphabet) {
    std::vector<T> item(rnd(max_len + 1));
    for (T &x : item) x = (T)(rnd(alphabet) * (sizeof(T) == 4 ? 0x01010101u : 1u));  // (4-byte elements: every byte differs)
    return item;
}

template <typename T> static void directed() {
    batch<T> b;
    EXPECT(run(b) == 0);  // n = 0
    b.add({1, 2, 3});
    EXPECT(run(b) == 1);  // n = 1
    b.add({1, 2});
    b.add({3, 2, 1});
    b.add({1, 2, 3, 4});
    EXPECT(run(b) == 4);  // nothing repeats
    b.add({});            // zero-length items among others
    b.add({1, 2});
    b.add({});
    b.add({1, 2, 3});
    b.add({});
    EXPECT(run(b) == 5);
    EXPECT(run(b, false) == 9);  // grouping switched off
    batch<T> same;
    for (int i = 0; i < 7; i++) same.add({4, 8, 1, 2, 2});
    EXPECT(run(same) == 1);  // everything equal
    EXPECT(run(same, false) == 7);
    batch<T> empties;
    for (int i = 0; i < 3; i++) empties.add({});
    EXPECT(run(empties) == 1);

    // items that agree in their first and last 64 bytes -- all that hash_ends reads of more than 160 bytes -- and
    // differ in the middle: equal hashes, told apart by the comparison
    const size_t len = 400 / sizeof(T) + 3;
    std::vector<T> long_item(len);
    for (size_t k = 0; k < len; k++) long_item[k] = (T)(1 + k % 7);
    batch<T> mid;
    for (int v = 0; v < 3; v++) {
        std::vector<T> item = long_item;
        item[len / 2] = (T)(100 + v);
        mid.add(item);
    }
    mid.add(long_item);
    std::vector<T> again = long_item;  // (= item 0)
    again[len / 2] = (T)100;
    mid.add(again);
    EXPECT(sizeof(T) * len > 160);
    EXPECT(hash_ends(mid.data.data(), sizeof(T) * len, 5) == hash_ends(mid.data.data() + mid.off[1], sizeof(T) * len, 5));
    EXPECT(hash_ends(mid.data.data(), sizeof(T) * len, 5) != hash_ends(mid.data.data(), sizeof(T) * len, 6));
    EXPECT(run(mid) == 4);

    // a hash that returns a constant: every item collides, equality alone decides
    {
        std::vector<uint32_t> rep;
        const size_t nd = group_equal_items(
            true, serial_for, b.n(), [](size_t) { return (uint64_t)42; }, [&](size_t x, size_t y) { return b.equal(x, y); }, rep);
        const distinct_items d = slots_of_rep(rep, nd, b.off.data());
        batch_scratch<T> dst;
        check(b, d, gather_distinct(d, serial_for, b.data.data(), b.off.data(), dst), dst, always);
        EXPECT(nd == 5);
    }

    // an extra key that separates byte-equal items: items 0..6 of `same` with keys 0 1 0 2 1 0 2
    {
        const int key[7] = {0, 1, 0, 2, 1, 0, 2};
        auto same_key_of = [&](size_t x, size_t y) { return key[x] == key[y]; };
        const distinct_items d = distinct_spans(
            true, serial_for, same.data.data(), same.off.data(), same.n(), [&](size_t i) { return (uint64_t)key[i] * 0x9E37u; }, same_key_of);
        batch_scratch<T> dst;
        check(same, d, gather_distinct(d, serial_for, same.data.data(), same.off.data(), dst), dst, same_key_of);
        EXPECT(d.n == 3 && d.slot_of == (std::vector<uint32_t>{0, 1, 0, 2, 1, 0, 2}));
        // ... and with a seed that does not tell the keys apart, the predicate alone does
        const distinct_items e = distinct_spans(
            true, serial_for, same.data.data(), same.off.data(), same.n(), [](size_t) { return (uint64_t)7; }, same_key_of);
        EXPECT(e.n == 3 && e.slot_of == d.slot_of && e.first == d.first && e.off == d.off);
    }
}

// a few hundred batches of short items over a small alphabet: repeats are common
template <typename T> static void random_batches() {
    size_t with_repeats = 0, without = 0;
    for (int round = 0; round < 300; round++) {
        batch<T> b;
        const uint32_t n = rnd(round % 3 == 0 ? 6 : 40), max_len = 1 + rnd(5), alphabet = 2 + rnd(2);
        for (uint32_t i = 0; i < n; i++) b.add(random_item<T>(max_len, alphabet));
        (run(b) < b.n() ? with_repeats : without)++;
        run(b, false);
    }
    EXPECT(with_repeats >= 100 && without >= 20);
}

int main() {
    directed<uint8_t>();
    directed<uint32_t>();
    random_batches<uint8_t>();
    random_batches<uint32_t>();
    if (fails) {
        printf("distinct_check: %d FAILED\n", fails);
        return 1;
    }
    printf("distinct_check: ok\n");
    return 0;
}
