"""The aligner's exact-relative test on the device (aligner option device-copy) on the bench's 16S
shape: store and queries from sina_amd/synth.py, built as bench.py --exact-rate builds them.

    python tools/perf_copy.py [--queries 9216] [--steps 2] [--refs 100000] [--rounds 3] [--inflight 6] [--out FILE]

Three workloads, each timed with the option off and on, the two legs alternating after a warm-up run of each:
    exact30          full-length queries, 30 % of them unmutated copies of their reference (bench.py --exact-rate 0.3)
    exact30_window   the same cut to windows of 250 bases (--window 250): several family members hold a window
    all_exact_window every query an unmutated window of 250 bases
Per run: sequences/s, busy host cores (process CPU seconds / wall seconds), trays the device answered, the containment
kernel's pairs, launches and milliseconds per launch, trays copied, resident host memory after the run.  The first run
of a process with the option off builds the store's upper-case cache (a byte per reference base): `rss_mb` of the
option-on warm-up, which comes first, is the figure without it.

Prints JSON lines; --out appends them to FILE (profiles/perf_copy.txt)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LENGTH, WIDTH = 1500, 50000


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def rss_mb():
    with open("/proc/self/status") as f:
        for line in f:
            if line.startswith("VmRSS:"):
                return int(line.split()[1]) / 1024.0
    return 0.0


def exact_mix(rate):
    """bench.py --exact-rate: query i of every hundred is exact if i < 100 x the rate."""
    k = int(round(100 * min(1.0, rate)))
    return dict(sub=[0.0] * k + [0.03] * (100 - k), dele=[0.0] * k + [0.005] * (100 - k), ins=[0.0] * k + [0.003] * (100 - k))


def main(a):
    from sina_amd import pipeline, synth
    refs = synth.make_refs(a.refs, length=LENGTH, width=WIDTH, seed=2)
    n = a.queries * a.steps
    window = (1.0 / 3.0, 250)
    loads = [("exact30", synth.make_queries(refs, n, seed=3, **exact_mix(0.3))),
             ("exact30_window", synth.make_queries(refs, n, seed=3, window=window, **exact_mix(0.3))),
             ("all_exact_window", synth.make_queries(refs, n, seed=3, window=window, **exact_mix(1.0)))]
    store = pipeline.Store(":mem:perf-copy", refs)
    store.build_index(10, False)
    pl = pipeline.Pipeline(store)

    def run(name, qs, on, tag):
        pl._set("aligner", "device-copy", bool(on))
        s0 = store.copy_stats()
        c0, t0 = os.times(), time.perf_counter()
        pl.run(qs.mask, qs.off, batch=a.queries, inflight=a.inflight)
        wall = time.perf_counter() - t0
        c1 = os.times()
        s1 = store.copy_stats()
        d = {k: s1[k] - s0[k] for k in s1}
        cpu = (c1.user - c0.user) + (c1.system - c0.system)
        copied = sum(1 for q in range(qs.n) if pl.result(q)["status"] == 1)
        emit(dict(workload=name, tag=tag, device_copy=bool(on), queries=qs.n, batch=a.queries, inflight=a.inflight, refs=refs.n,
                  wall_s=wall, sequences_per_s=qs.n / wall, busy_host_cores=cpu / wall, copied_trays=copied,
                  device_trays=d["trays"], fallback_trays=d["fallback_trays"], pairs=d["pairs"], launches=d["launches"],
                  kernel_ms=d["kernel_ms"], kernel_ms_per_launch=d["kernel_ms"] / d["launches"] if d["launches"] else 0.0,
                  rss_mb=rss_mb()), a.out)

    for name, qs in loads:       # (the option on first: the upper-case cache does not exist yet)
        run(name, qs, True, "warm-up")
    for name, qs in loads:
        run(name, qs, False, "warm-up")
    for rnd in range(a.rounds):
        for name, qs in loads:
            run(name, qs, False, "round %d" % rnd)
            run(name, qs, True, "round %d" % rnd)
    pl.close()
    store.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=9216)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inflight", type=int, default=6)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
