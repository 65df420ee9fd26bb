// A run of items through an ordered list of stages, as the host drivers need it (capi.cpp): a source makes
// items, every further stage works on them, the last one keeps what it wants of them.  Knows nothing of trays,
// stores or the device -- tests/flow_check.cpp runs it on the CPU under the thread sanitizer.
//
//   flow::runner<item> run(discard);
//   run.source("finder", 3, make)             bool make(item &): false = no more items
//      .then(3, "aligner", 4, align)          void align(item &), behind a queue of 3 items
//      .then(2, "sink", 1, keep);
//   run.staged();   or   run.inline_();      (once: a runner is not run again)
//
// Errors.  The first exception of any body is kept, every queue is stopped, the sources make nothing more, every
// thread is joined, and only then is that exception rethrown on the caller; later exceptions are dropped.  The
// item in the hands of a body that throws is dropped as it is and NOT given to `discard`: the stage that threw
// owns whatever state it left the item in.  Every other item that does not reach the last stage is discarded.
#pragma once
#include <atomic>
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace sina::flow {

// Bounded FIFO hand-over from `producers` threads to any number of consumers.
template <class Item>
class handover {
public:
    using discard_fn = std::function<void(Item &)>;
    handover(size_t capacity, unsigned n_producers, discard_fn on_discard)
        : cap(capacity), producers(n_producers), discard(std::move(on_discard)) {}
    // waits while the queue is full; after stop() the item is discarded instead
    void push(Item &&it) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return q.size() < cap || stopped; });
        if (stopped) return discard(it);
        q.push_back(std::move(it));
        cv.notify_all();
    }
    // waits while the queue is empty and a producer is live; false: drained with no producer left, or stopped
    bool pop(Item &it) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !q.empty() || producers == 0 || stopped; });
        if (stopped || q.empty()) return false;
        it = std::move(q.front());
        q.pop_front();
        cv.notify_all();
        return true;
    }
    void producer_done() {
        std::lock_guard<std::mutex> lk(mu);
        if (--producers == 0) cv.notify_all();
    }
    // discards what is queued and wakes every waiter
    void stop() {
        std::lock_guard<std::mutex> lk(mu);
        stopped = true;
        for (Item &it : q) discard(it);
        q.clear();
        cv.notify_all();
    }

private:
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Item> q;
    const size_t cap;
    unsigned producers;
    bool stopped = false;
    const discard_fn discard;
};

template <class Item>
class runner {
public:
    using source_fn = std::function<bool(Item &)>;
    using body_fn = std::function<void(Item &)>;
    using exit_fn = std::function<void()>;  // runs on each thread of its stage as the thread leaves (staged only)

    explicit runner(typename handover<Item>::discard_fn on_discard) : discard(std::move(on_discard)) {}
    runner &source(const char *name, unsigned threads, source_fn make, exit_fn at_exit = nullptr) {
        stages.push_back({name, threads, 0, nullptr, std::move(at_exit)});
        make_item = std::move(make);
        return *this;
    }
    // the next stage, behind a queue of `capacity` items
    runner &then(size_t capacity, const char *name, unsigned threads, body_fn body, exit_fn at_exit = nullptr) {
        stages.push_back({name, threads, capacity, std::move(body), std::move(at_exit)});
        return *this;
    }

    // one item at a time through every body on the calling thread
    void inline_() {
        Item it;
        while (make_item(it)) {
            for (size_t s = 1; s < stages.size(); s++) stages[s].body(it);
            it = Item();
        }
    }

    // every stage on its own threads, queues between them
    void staged() {
        for (size_t s = 1; s < stages.size(); s++) queues.emplace_back(stages[s].capacity, stages[s - 1].threads, discard);
        std::vector<std::thread> th;
        try {
            for (size_t s = 0; s < stages.size(); s++)
                for (unsigned i = 0; i < stages[s].threads; i++) th.emplace_back([this, s] { work(s); });
        } catch (...) {  // (a thread that could not be started: the ones that were must not wait for it)
            fail();
        }
        for (std::thread &t : th) t.join();
        if (err) std::rethrow_exception(err);
    }

private:
    struct stage {
        const char *name;
        unsigned threads;
        size_t capacity;  // of the queue in front of it
        body_fn body;
        exit_fn at_exit;
    };
    void work(size_t s) {
        handover<Item> *in = s ? &queues[s - 1] : nullptr, *out = s + 1 < stages.size() ? &queues[s] : nullptr;
        try {
            Item it;
            while (in ? in->pop(it) : (!halted.load() && make_item(it))) {
                if (in) stages[s].body(it);
                if (out) out->push(std::move(it));
                it = Item();
            }
        } catch (...) {
            fail();
        }
        if (out) out->producer_done();
        if (stages[s].at_exit) stages[s].at_exit();
    }
    void fail() {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!err) err = std::current_exception();
        }
        halted.store(true);
        for (handover<Item> &q : queues) q.stop();
    }

    const typename handover<Item>::discard_fn discard;
    source_fn make_item;
    std::vector<stage> stages;
    std::deque<handover<Item>> queues;  // queues[s]: behind stage s
    std::mutex mu;                      // guards err
    std::exception_ptr err;
    std::atomic<bool> halted{false};
};

}  // namespace sina::flow
