"""--fs-no-graph end to end, the profile built on the device against the profile built on the host.

Shape: 16S (100 000 references of 1500 bases in 50 000 columns), batches of 9216 full-length queries through
famfinder -> aligner with fs-no-graph on.  One pipeline, its device-profile option switched between runs: 1
(sina_hip_align_profiles) and 0 (build_family_profile + sina_hip_align_graphs); one warm-up run per leg, then --runs
timed runs per leg, alternating.  Per run: sequences/s over the wall time, the aligner stage's seconds, and the profile
build's device time per launch (graph_ms / graph_launches: 0 launches on the host route).  Prints one JSON line;
--out also writes it to a file.  On a tree without the device route both legs take the host route.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from sina_amd import capi, pipeline, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--length", type=int, default=1500)
    ap.add_argument("--width", type=int, default=50000)
    ap.add_argument("--batch", type=int, default=9216)
    ap.add_argument("--steps", type=int, default=2, help="batches per run")
    ap.add_argument("--runs", type=int, default=5, help="timed runs per leg")
    ap.add_argument("--inflight", type=int, default=6)
    ap.add_argument("--host-threads", type=int, default=6)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    refs = synth.make_refs(a.refs, length=a.length, width=a.width, seed=2)
    pool = [synth.make_queries(refs, a.batch, seed=(3, b)) for b in range(a.steps)]
    mask = np.concatenate([q.mask for q in pool])
    off = np.zeros(a.steps * a.batch + 1, np.int64)
    np.cumsum(np.concatenate([np.diff(q.off) for q in pool]), out=off[1:])
    n = a.steps * a.batch

    store = pipeline.Store(":mem:perf-profile", refs)
    store.build_index(10, False)
    has_device_route = hasattr(capi.load(), "sina_hip_align_profiles")
    pl = pipeline.Pipeline(store, aligner={"fs-no-graph": True}, host_threads=a.host_threads)
    legs = {"device": True, "host": False}

    def one(name):
        if has_device_route:
            pl._set("aligner", "device-profile", legs[name])   # (the stages read their options when they run)
        s0 = store.stats()
        t0 = time.time()
        t = pl.run(mask, off, batch=a.batch, inflight=a.inflight)
        wall = time.time() - t0
        s1 = store.stats()
        launches = s1["graph_launches"] - s0["graph_launches"]
        aligned = sum(1 for q in range(0, n, max(1, n // 256)) if pl.result(q)["status"] == 0)
        return dict(seq_per_s=n / wall, wall_s=wall, aligner_s=t["aligner_s"], famfinder_s=t["famfinder_s"],
                    graph_launches=launches, graph_ms_per_launch=(s1["graph_ms"] - s0["graph_ms"]) / launches if launches else 0.0,
                    profiles_built=s1["dags_built"] - s0["dags_built"], dp_ms=s1["dp_ms"] - s0["dp_ms"],
                    sampled_aligned=aligned)

    for name in legs:           # (scratch, trace-back planes, pinned staging: allocated here)
        one(name)
    runs = {name: [] for name in legs}
    for r in range(a.runs):
        for name in (("device", "host") if r % 2 == 0 else ("host", "device")):
            runs[name].append(one(name))
    res = dict(tool="tools/perf_profile.py", label=a.label, device_route_present=has_device_route,
               shape=dict(refs=a.refs, length=a.length, width=a.width, batch=a.batch, steps=a.steps, inflight=a.inflight,
                          host_threads=a.host_threads, runs=a.runs), legs={})
    for name, rs in runs.items():
        res["legs"][name] = dict(
            median_seq_per_s=statistics.median(x["seq_per_s"] for x in rs),
            median_aligner_s=statistics.median(x["aligner_s"] for x in rs),
            median_graph_ms_per_launch=statistics.median(x["graph_ms_per_launch"] for x in rs),
            runs=rs)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    pl.close()
    store.close()


if __name__ == "__main__":
    main()
