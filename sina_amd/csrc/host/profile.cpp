// The host stages' phase profiler (SINA_HOST_PROFILE, SINA_HOST_TRACE) and the thread pool behind parallel_for.
#include "stages_internal.h"

#include <sys/resource.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <map>

namespace sina {

// ================================================================ phase profiler (SINA_HOST_PROFILE=1)

namespace {
struct prof_state {
    std::mutex mu;
    std::map<std::string, std::pair<double, uint64_t>> acc;
    bool on = getenv("SINA_HOST_PROFILE") != nullptr;
    // SINA_HOST_TRACE=<file>: every phase as "thread name t0 t1" (seconds), to see what the batches
    // in flight are doing while the GPU idles
    const char *trace_path = getenv("SINA_HOST_TRACE");
    struct ev {
        size_t tid;
        const char *name;
        double t0, t1;
    };
    std::vector<ev> events;
    std::chrono::steady_clock::time_point origin = std::chrono::steady_clock::now();
};
prof_state &prof() {
    static prof_state p;
    return p;
}
thread_local const char *tl_phase = "(no phase)";  // innermost phase of this thread: names its pool jobs
double thread_cpu_s() {
    if (!prof().on) return 0.0;  // (a system call: only worth it when somebody reads the numbers)
    timespec ts;
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
thread_use thread_use_now() {
    thread_use u;
    if (!prof().on) return u;
    rusage ru;
    if (getrusage(RUSAGE_THREAD, &ru) != 0) return u;
    u.sys = (double)ru.ru_stime.tv_sec + 1e-6 * (double)ru.ru_stime.tv_usec;
    u.cpu = thread_cpu_s();
    u.faults = (double)ru.ru_minflt;
    return u;
}
void add_cpu(const char *phase, double s);
void add_use(const char *phase, const thread_use &since) {
    const thread_use now = thread_use_now();
    add_cpu(phase, now.cpu - since.cpu);
    const std::string ph(phase);
    add_cpu((ph + " (kernel mode)").c_str(), now.sys - since.sys);
    add_cpu((ph + " (k page faults)").c_str(), 1e-3 * (now.faults - since.faults));
}
void add_cpu(const char *phase, double s) {  // CPU seconds spent under a phase, by whichever thread
    prof_state &p = prof();
    if (!p.on) return;
    std::lock_guard<std::mutex> lk(p.mu);
    auto &e = p.acc[std::string(phase) + " [cpu]"];
    e.first += s;
    e.second++;
}
}  // namespace

scoped_phase::scoped_phase(const char *n) : name(n), outer(tl_phase), use0(thread_use_now()), t0(std::chrono::steady_clock::now()) {
    tl_phase = n;
}
scoped_phase::~scoped_phase() {
    tl_phase = outer;
    prof_state &p = prof();
    if (p.on) add_use(name, use0);
    if (!p.on && !p.trace_path) return;
    const auto t1 = std::chrono::steady_clock::now();
    const double s = std::chrono::duration<double>(t1 - t0).count();
    std::lock_guard<std::mutex> lk(p.mu);
    if (p.trace_path)
        p.events.push_back({std::hash<std::thread::id>()(std::this_thread::get_id()) % 9973, name,
                            std::chrono::duration<double>(t0 - p.origin).count(),
                            std::chrono::duration<double>(t1 - p.origin).count()});
    if (!p.on) return;
    auto &e = p.acc[name];
    e.first += s;
    e.second++;
}

void host_profile_add_cpu(const char *what, double seconds) { add_cpu(what, seconds); }
void host_profile_mark(const char *what) {  // a zero-length event in the SINA_HOST_TRACE file
    prof_state &p = prof();
    if (!p.trace_path) return;
    const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - p.origin).count();
    std::lock_guard<std::mutex> lk(p.mu);
    p.events.push_back({0, what, t, t});
}

namespace {
struct tick_slot {
    std::atomic<const char *> name{nullptr};
    std::atomic<uint64_t> cycles{0}, samples{0};
};
tick_slot g_ticks[64];
}  // namespace
uint64_t host_tsc() { return prof().on ? __builtin_ia32_rdtsc() : 0; }
uint64_t host_tick(const char *what, uint64_t since) {
    if (!prof().on) return 0;
    const uint64_t now = __builtin_ia32_rdtsc();
    // (slots are keyed by the literal's address: a short probe sequence, names are few)
    size_t h = (reinterpret_cast<uintptr_t>(what) >> 3) % 64;
    for (int probe = 0; probe < 64; probe++, h = (h + 1) % 64) {
        const char *cur = g_ticks[h].name.load(std::memory_order_acquire);
        if (cur == nullptr) {
            const char *expect = nullptr;
            if (g_ticks[h].name.compare_exchange_strong(expect, what)) cur = what;
            else cur = expect;
        }
        if (cur == what) {
            g_ticks[h].cycles.fetch_add(now - since, std::memory_order_relaxed);
            g_ticks[h].samples.fetch_add(1, std::memory_order_relaxed);
            break;
        }
    }
    return now;
}
double host_thread_cpu_seconds() { return thread_cpu_s(); }
void host_profile_thread_exit(const char *who) {
    if (!prof().on) return;
    rusage ru;
    if (getrusage(RUSAGE_THREAD, &ru) != 0) return;
    const std::string w(who);
    add_cpu(w.c_str(), thread_cpu_s());
    add_cpu((w + " kernel-mode").c_str(), (double)ru.ru_stime.tv_sec + 1e-6 * (double)ru.ru_stime.tv_usec);
    add_cpu((w + " k-minor-faults").c_str(), 1e-3 * (double)ru.ru_minflt);
    add_cpu((w + " k-voluntary-switches").c_str(), 1e-3 * (double)ru.ru_nvcsw);
    add_cpu((w + " k-involuntary-switches").c_str(), 1e-3 * (double)ru.ru_nivcsw);
}
host_phase::host_phase(const char *n) : impl(new scoped_phase(n)) {}
host_phase::~host_phase() { delete static_cast<scoped_phase *>(impl); }

std::string host_profile_dump(bool reset) {
    prof_state &p = prof();
    std::lock_guard<std::mutex> lk(p.mu);
    std::string out;
    char buf[160];
    for (auto &kv : p.acc) {
        snprintf(buf, sizeof(buf), "%-28s %9.3f s  %6llu calls\n", kv.first.c_str(), kv.second.first,
                 (unsigned long long)kv.second.second);
        out += buf;
    }
    {   // time-stamp-counter slots: cycles -> seconds by a one-off calibration against the steady clock
        static const double tsc_hz = [] {
            const auto t0 = std::chrono::steady_clock::now();
            const uint64_t c0 = __builtin_ia32_rdtsc();
            while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < 0.02) {
            }
            return (double)(__builtin_ia32_rdtsc() - c0) / std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }();
        std::vector<std::pair<std::string, std::pair<double, unsigned long long>>> rows;
        for (auto &t : g_ticks) {
            const char *n = t.name.load();
            if (!n) continue;
            rows.push_back({n, {(double)t.cycles.load() / tsc_hz, (unsigned long long)t.samples.load()}});
            if (reset) {
                t.cycles.store(0);
                t.samples.store(0);
            }
        }
        std::sort(rows.begin(), rows.end());
        for (auto &r : rows) {
            snprintf(buf, sizeof(buf), "%-36s %9.3f s  %8llu samples  %7.2f us each [tsc]\n", r.first.c_str(), r.second.first,
                     r.second.second, r.second.second ? 1e6 * r.second.first / (double)r.second.second : 0.0);
            out += buf;
        }
    }
    if (reset) p.acc.clear();
    if (p.trace_path && !p.events.empty()) {
        if (FILE *f = fopen(p.trace_path, "w")) {
            for (auto &e : p.events) fprintf(f, "%zu %s %.6f %.6f\n", e.tid, e.name, e.t0, e.t1);
            fclose(f);
        }
    }
    if (reset) p.events.clear();
    return out;
}

// ================================================================ thread pool

namespace {
// Worker threads shared by every parallel_for in flight: each call posts a job (index range +
// function), the workers and the caller itself pull indices from the posted jobs until they are
// exhausted.  Several host threads (one per batch in flight) can therefore run their per-query loops
// concurrently on the same pool.
class pool {
    struct job {
        const std::function<void(size_t)> *fn;
        const char *phase;
        size_t n;
        size_t chunk = 1;  // indices taken per grab (one shared counter: a grab per query was a cache-line fight)
        std::atomic<size_t> next{0}, done{0};
        std::mutex err_mu;
        std::exception_ptr error;
    };

public:
    static pool &get() {
        static pool p;
        return p;
    }
    void resize(unsigned n) {
        shutdown();
        start(n);
    }
    unsigned size() const { return (unsigned)workers.size() + 1; }
    void run(size_t n, const std::function<void(size_t)> &fn) {
        if (n == 0) return;
        if (workers.empty() || n == 1) {
            for (size_t i = 0; i < n; i++) fn(i);
            return;
        }
        auto j = std::make_shared<job>();
        j->fn = &fn;
        j->phase = tl_phase;
        j->n = n;
        j->chunk = std::max<size_t>(1, n / ((workers.size() + 1) * 8));
        {
            std::lock_guard<std::mutex> lk(mu);
            jobs.push_back(j);
        }
        cv.notify_all();
        work_on(*j);  // the caller helps with its own job
        {
            std::unique_lock<std::mutex> lk(mu);
            done_cv.wait(lk, [&] { return j->done.load() == j->n; });
            jobs.erase(std::find(jobs.begin(), jobs.end(), j));
        }
        if (j->error) std::rethrow_exception(j->error);
    }
    ~pool() { shutdown(); }

private:
    pool() {
        unsigned hw = std::thread::hardware_concurrency();
        // (measured on a 256-thread host, round 2: 6 threads 104 k seq/s at 8.3 busy cores, 8: 111 k / 8.9,
        // 10: 112 k / 8.7, 16: 113 k / 10.7, 32: 111 k / 15 -- more threads only fight over the allocator;
        // with the rank's threads pinned to 16 neighbouring cores (sina_amd/affinity.py) 16S is the same
        // at 10 and 12 (112.7 k / 7.3 and 7.6 cores) and the host-bound V4 amplicons gain: 273 k -> 292 k)
        start(hw > 1 ? std::min(hw, 12u) : 1);
    }
    void start(unsigned n) {
        stop = false;
        for (unsigned i = 1; i < n; i++) workers.emplace_back([this] { loop(); });
    }
    void shutdown() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv.notify_all();
        for (auto &w : workers) w.join();
        workers.clear();
    }
    void work_on(job &j) {
        const bool helper = tl_phase != j.phase;  // (the posting thread's own time is in its scoped_phase)
        const thread_use c0 = (helper && prof().on) ? thread_use_now() : thread_use();
        struct at_exit {
            bool on;
            const char *ph;
            thread_use c0;
            ~at_exit() {
                if (on) add_use(ph, c0);
            }
        } acc{helper && prof().on, j.phase, c0};
        for (;;) {
            const size_t i0 = j.next.fetch_add(j.chunk);
            if (i0 >= j.n) break;
            const size_t i1 = std::min(j.n, i0 + j.chunk);
            for (size_t i = i0; i < i1; i++) {
                try {
                    (*j.fn)(i);
                } catch (...) {
                    std::lock_guard<std::mutex> lk(j.err_mu);
                    if (!j.error) j.error = std::current_exception();
                }
            }
            if (j.done.fetch_add(i1 - i0) + (i1 - i0) == j.n) {
                std::lock_guard<std::mutex> lk(mu);  // (pairs with the waiter's predicate check)
                done_cv.notify_all();
            }
        }
    }
    void loop() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            std::shared_ptr<job> j;
            cv.wait(lk, [&] {
                if (stop) return true;
                for (auto &x : jobs)
                    if (x->next.load() < x->n) {
                        j = x;
                        return true;
                    }
                return false;
            });
            if (stop) return;
            lk.unlock();
            work_on(*j);
            j.reset();
            lk.lock();
        }
    }
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv, done_cv;
    std::vector<std::shared_ptr<job>> jobs;
    bool stop = false;
};
std::mutex pool_resize_mu;
}  // namespace

void parallel_for(size_t n, const std::function<void(size_t)> &fn) { pool::get().run(n, fn); }
void set_host_threads(unsigned n) {  // (not while loops are running)
    std::lock_guard<std::mutex> lk(pool_resize_mu);
    pool::get().resize(n < 1 ? 1 : n);
}
unsigned host_threads() { return pool::get().size(); }

}  // namespace sina
