// The staged runner and its hand-over queue (sina_amd/csrc/host/flow.h) on the CPU, under the thread sanitizer:
// delivery, order, the bound on items alive, and what happens when bodies throw -- with full queues and with
// empty ones.  Stand-alone; tests/test_flow_cpu.py builds and runs it.  Ends with "flow_check: ok" and status 0.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "flow.h"

using namespace sina;

namespace {
int failures = 0;
std::string current;  // the case being run, for the messages (and, printed as it starts, for a run that hangs)
void begin(const std::string &name) {
    current = name;
    printf("%s\n", name.c_str());
}
#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            failures++;                                              \
            printf("FAILED [%s] %s: ", current.c_str(), #cond);      \
            printf(__VA_ARGS__);                                     \
            printf("\n");                                            \
        }                                                            \
    } while (0)

// What travels: a number, once the source has made it.  Every item counts itself as made, then as exactly one
// of sunk, discarded or held (by a body that threw with it in its hands).
struct tally {
    std::atomic<int> made{0}, sunk{0}, discarded{0}, held{0}, alive{0}, high{0}, exits{0}, sink_calls{0};
    std::vector<std::atomic<int>> times_sunk;
    std::mutex order_mu;
    std::vector<int> order;  // ids as the sink saw them
    explicit tally(int n) : times_sunk((size_t)n) {}
    void born() {
        made++;
        const int a = ++alive;
        int h = high.load();
        while (a > h && !high.compare_exchange_weak(h, a)) {}
    }
};
struct item {
    int id = -1;
};

enum speed { seeded, slow_consumer, fast_consumer };
struct scenario {
    std::vector<unsigned> threads;  // per stage: source, middle stages, sink
    std::vector<size_t> caps;       // per queue
    int n_items = 0;
    bool inline_mode = false;
    speed sp = seeded;
    // up to two throwers: (stage, item id); two of them meet before they throw
    int throw_stage[2] = {-1, -1}, throw_at[2] = {-1, -1};
};
struct outcome {
    bool threw = false;
    std::string what;
};

// 0 to 200 us, a function of (stage, id) alone: the same in every run, whichever thread gets the item
void nap(const scenario &sc, size_t stage, int id) {
    uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(id + 1) + 0xD1B54A32D192ED03ull * (stage + 1);
    x ^= x >> 29, x *= 0xBF58476D1CE4E5B9ull, x ^= x >> 32;
    unsigned us = (unsigned)(x % 201);
    const bool sink = stage + 1 == sc.threads.size();
    if (sc.sp == slow_consumer) us = sink ? 300 + us : 0;  // the queues fill up
    if (sc.sp == fast_consumer) us = sink ? 0 : us;        // the queues run dry
    if (us) std::this_thread::sleep_for(std::chrono::microseconds(us));
}

outcome run(const scenario &sc, tally &t) {
    const size_t n_stages = sc.threads.size();
    const int n_throwers = (sc.throw_stage[0] >= 0) + (sc.throw_stage[1] >= 0);
    std::atomic<int> next{0}, met{0};
    auto maybe_throw = [&](size_t stage, item &it) {
        for (int k = 0; k < 2; k++)
            if (sc.throw_stage[k] == (int)stage && sc.throw_at[k] == it.id) {
                // two throwers go together (or the second alone, should the first never come: no hang here)
                met++;
                const auto give_up = std::chrono::steady_clock::now() + std::chrono::seconds(20);
                while (met.load() < n_throwers && std::chrono::steady_clock::now() < give_up) std::this_thread::yield();
                t.held++;
                t.alive--;
                throw std::runtime_error("boom " + std::to_string(it.id));
            }
    };
    flow::runner<item> r([&](item &it) {
        if (it.id < 0) return;  // (never made)
        t.discarded++;
        t.alive--;
    });
    r.source("source", sc.threads[0], [&](item &it) {
        const int id = next.fetch_add(1);
        if (id >= sc.n_items) return false;
        it.id = id;
        t.born();
        nap(sc, 0, id);
        maybe_throw(0, it);
        return true;
    }, [&] { t.exits++; });
    for (size_t s = 1; s + 1 < n_stages; s++)
        r.then(sc.caps[s - 1], "middle", sc.threads[s], [&, s](item &it) {
            nap(sc, s, it.id);
            maybe_throw(s, it);
        }, [&] { t.exits++; });
    r.then(sc.caps[n_stages - 2], "sink", sc.threads[n_stages - 1], [&](item &it) {
        t.sink_calls++;
        nap(sc, n_stages - 1, it.id);
        maybe_throw(n_stages - 1, it);
        t.times_sunk[(size_t)it.id]++;
        t.sunk++;
        t.alive--;
        std::lock_guard<std::mutex> lk(t.order_mu);
        t.order.push_back(it.id);
    }, [&] { t.exits++; });
    outcome o;
    try {
        if (sc.inline_mode) r.inline_();
        else r.staged();
    } catch (const std::exception &e) {
        o.threw = true;
        o.what = e.what();
    }
    return o;
}

unsigned sum(const std::vector<unsigned> &v) {
    unsigned s = 0;
    for (unsigned x : v) s += x;
    return s;
}
std::string shape(const scenario &sc) {
    std::string s = "(";
    for (size_t i = 0; i < sc.threads.size(); i++) s += (i ? "," : "") + std::to_string(sc.threads[i]);
    return s + ") " + std::to_string(sc.n_items) + " items" + (sc.inline_mode ? " inline" : "") +
           (sc.sp == slow_consumer ? " slow sink" : sc.sp == fast_consumer ? " fast sink" : "");
}
// what holds after every run, with or without an error
void check_accounts(const scenario &sc, const tally &t) {
    CHECK(t.made == t.sunk + t.discarded + t.held, "made %d sunk %d discarded %d held %d", t.made.load(), t.sunk.load(),
          t.discarded.load(), t.held.load());
    CHECK(t.alive == 0, "alive %d", t.alive.load());
    for (size_t i = 0; i < t.times_sunk.size(); i++) CHECK(t.times_sunk[i] <= 1, "item %zu sunk %d times", i, t.times_sunk[i].load());
    CHECK(t.exits == (int)(sc.inline_mode ? 0 : sum(sc.threads)), "%d exit hooks ran", t.exits.load());
    if (!sc.inline_mode) {
        size_t bound = sum(sc.threads);
        for (size_t c : sc.caps) bound += c;
        CHECK((size_t)t.high <= bound, "%d items alive at once, bound %zu", t.high.load(), bound);
    } else CHECK(t.high <= 1, "%d items alive at once in inline mode", t.high.load());
}

// the shapes the drivers use: pipeline_run with inflight = 2, 4, 3 (queue behind the finders: n_find items, behind
// the aligners: 2) and run_fasta's four nodes with queues of 2
const scenario shapes[] = {
    {{1, 1, 1}, {1, 2}}, {{3, 4, 1}, {3, 2}}, {{2, 3, 1}, {2, 2}}, {{1, 1, 1, 1}, {2, 2, 2}},
};

void delivery_and_order() {
    for (const scenario &base : shapes)
        for (int n : {0, 1, (int)base.caps[0] + 1, 50}) {
            scenario sc = base;
            sc.n_items = n;
            begin("delivery " + shape(sc));
            tally t(n);
            const outcome o = run(sc, t);
            CHECK(!o.threw, "%s", o.what.c_str());
            check_accounts(sc, t);
            CHECK(t.made == n && t.sunk == n && t.discarded == 0, "made %d sunk %d discarded %d", t.made.load(), t.sunk.load(),
                  t.discarded.load());
            if (n == 0) CHECK(t.sink_calls == 0, "the sink ran %d times without an item", t.sink_calls.load());
            if (sum(sc.threads) == sc.threads.size()) {  // one thread per stage: the source's order, and inline the same
                std::vector<int> want((size_t)n);
                for (int i = 0; i < n; i++) want[(size_t)i] = i;
                CHECK(t.order == want, "staged order differs from the source's");
                sc.inline_mode = true;
                begin("order " + shape(sc));
                tally ti(n);
                const outcome oi = run(sc, ti);
                CHECK(!oi.threw, "%s", oi.what.c_str());
                check_accounts(sc, ti);
                CHECK(ti.order == want && ti.order == t.order, "inline order differs from the staged one");
            }
        }
}

void errors() {
    const int n = 20;
    for (const scenario &base : {shapes[0], shapes[1], shapes[3]})
        for (int stage : {0, 1, (int)base.threads.size() - 1})
            for (int at : {0, n / 2, n - 1})
                for (speed sp : {slow_consumer, fast_consumer}) {
                    scenario sc = base;
                    sc.n_items = n, sc.sp = sp, sc.throw_stage[0] = stage, sc.throw_at[0] = at;
                    begin("error in stage " + std::to_string(stage) + " at item " + std::to_string(at) + " " + shape(sc));
                    tally t(n);
                    const outcome o = run(sc, t);
                    CHECK(o.threw && o.what == "boom " + std::to_string(at), "threw %d '%s'", o.threw, o.what.c_str());
                    CHECK(t.held == 1, "held %d", t.held.load());
                    check_accounts(sc, t);
                }
    // inline: the same contract on the calling thread
    for (int stage : {0, 1, 2}) {
        scenario sc = shapes[0];
        sc.n_items = n, sc.inline_mode = true, sc.throw_stage[0] = stage, sc.throw_at[0] = 7;
        begin("error in stage " + std::to_string(stage) + " " + shape(sc));
        tally t(n);
        const outcome o = run(sc, t);
        CHECK(o.threw && o.what == "boom 7", "threw %d '%s'", o.threw, o.what.c_str());
        CHECK(t.sunk == 7 && t.held == 1 && t.made == 8, "made %d sunk %d held %d", t.made.load(), t.sunk.load(), t.held.load());
        check_accounts(sc, t);
    }
}

void two_throwers() {
    // {stage, item, stage, item, items in all}: two aligner threads at once; an aligner thread and the sink at once;
    // a finder thread and the sink at once.  The first thrower to arrive waits for the second with its item in its
    // hands, so the second must be able to arrive whatever order the threads run in:
    //  - an aligner that waits blocks one of four aligner threads and nothing else: every other item flows on.
    //  - the sink that waits blocks everything behind it once the queue in front of it (2) and the aligner threads
    //    are full.  Item 6 still gets an aligner thread if the items that can be ahead of it -- all but the two
    //    throwers' -- fit into that queue and three aligner threads: 7 items in all, not more.
    //  - the finder that makes item 9 needs items 0 and 2 .. 8 out of the finders' hands: they fit behind them
    //    (3 + 4 aligner threads + 2), and no later item exists before 9 does.
    const int pairs[3][5] = {{1, 5, 1, 6, 30}, {1, 6, 2, 1, 7}, {0, 9, 2, 1, 30}};
    for (const auto &pr : pairs)
        for (speed sp : {slow_consumer, fast_consumer}) {
            scenario sc = shapes[1];
            sc.n_items = pr[4], sc.sp = sp;
            sc.throw_stage[0] = pr[0], sc.throw_at[0] = pr[1], sc.throw_stage[1] = pr[2], sc.throw_at[1] = pr[3];
            begin("two throwers (stage " + std::to_string(pr[0]) + " and stage " + std::to_string(pr[2]) + ") " + shape(sc));
            tally t(sc.n_items);
            const outcome o = run(sc, t);
            CHECK(o.threw && (o.what == "boom " + std::to_string(pr[1]) || o.what == "boom " + std::to_string(pr[3])), "threw %d '%s'",
                  o.threw, o.what.c_str());
            CHECK(t.held == 2, "held %d", t.held.load());
            check_accounts(sc, t);
        }
}

void sink_error_stops_the_source() {
    scenario sc = shapes[0];
    sc.n_items = 10000, sc.throw_stage[0] = 2, sc.throw_at[0] = 3;
    begin("a sink error stops the source " + shape(sc));
    tally t(sc.n_items);
    const outcome o = run(sc, t);
    CHECK(o.threw && o.what == "boom 3", "threw %d '%s'", o.threw, o.what.c_str());
    CHECK(t.made < sc.n_items, "the source made all %d items", t.made.load());
    check_accounts(sc, t);
}

void queue_alone() {
    int discarded = 0;
    auto discard = [&](item &) { discarded++; };
    item it;
    {
        begin("queue: drained and no producer left");
        flow::handover<item> q(2, 2, discard);
        q.push(item{1});
        q.producer_done();
        q.push(item{2});
        CHECK(q.pop(it) && it.id == 1, "first pop gave %d", it.id);
        std::atomic<int> late{-2};
        std::thread consumer([&] {  // takes the second, then waits: a producer is live and the queue empty
            item a, b;
            const bool got = q.pop(a);
            late = got && !q.pop(b) ? a.id : -1;
        });
        std::this_thread::sleep_for(std::chrono::milliseconds(5));
        CHECK(late == -2, "pop returned %d with a producer live", late.load());
        q.producer_done();
        consumer.join();
        CHECK(late == 2, "second pop, then the end: %d", late.load());
        CHECK(!q.pop(it), "pop after the end");
        CHECK(discarded == 0, "%d discarded", discarded);
    }
    {
        begin("queue: stop discards what is queued, push after stop discards");
        flow::handover<item> q(2, 1, discard);
        q.push(item{1});
        q.push(item{2});
        std::thread blocked([&] { q.push(item{3}); });  // the queue is full: waits until stop() lets it discard
        std::this_thread::sleep_for(std::chrono::milliseconds(5));
        q.stop();
        blocked.join();
        CHECK(discarded == 3, "%d discarded after stop", discarded);
        q.push(item{4});
        CHECK(discarded == 4, "%d discarded after a push behind stop", discarded);
        CHECK(!q.pop(it), "pop after stop");
    }
}
}  // namespace

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const auto t0 = std::chrono::steady_clock::now();
    queue_alone();
    delivery_and_order();
    errors();
    two_throwers();
    sink_error_stops_the_source();
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (failures) {
        printf("flow_check: %d checks FAILED (%.2f s)\n", failures, s);
        return 1;
    }
    printf("flow_check: ok (%.2f s)\n", s);
    return 0;
}
