"""--calc-idty (align_ident_slv) on the bench's 16S shape: store and queries from sina_amd/synth.py.

    python tools/perf_idty.py [--queries 9216] [--steps 4] [--refs 100000] [--rounds 3] [--inflight 6] [--out FILE]

Pipeline.run three ways, alternating in one process: without calc-idty, with it (every finished alignment packed and
uploaded again for compare_kernel on a second context), and with it plus the aligner's device-idty (scored where the
device assembles the alignment, family_identity_kernel).  Per run: sequences/s, busy host cores, the compare launches
of the second trip, the trays scored in place and the in-place kernel's launches, (query, member) pairs and time by
its own events -- in all and per launch.

Prints JSON lines; --out appends them to FILE (profiles/perf_idty.txt)."""
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


def main(a):
    from sina_amd import pipeline, synth
    refs = synth.make_refs(a.refs, length=LENGTH, width=WIDTH, seed=2)
    qs = synth.make_queries(refs, a.queries * a.steps, seed=3)
    store = pipeline.Store(":mem:perf-idty", refs)
    store.build_index(10, False)
    pl = pipeline.Pipeline(store)

    def run(calc, in_place, tag):
        pl._set("aligner", "calc-idty", bool(calc))
        pl._set("aligner", "device-idty", bool(in_place))
        s0, i0 = store.stats(), store.identity_inplace_stats()
        c0, t0 = os.times(), time.perf_counter()
        pl.run(qs.mask, qs.off, batch=a.queries, inflight=a.inflight)
        wall = time.perf_counter() - t0
        c1 = os.times()
        s1, i1 = store.stats(), store.identity_inplace_stats()
        cpu = (c1.user - c0.user) + (c1.system - c0.system)
        with_idty = sum(1 for q in range(0, qs.n, 97) if pl.result(q)["idty"] > 0)
        launches = i1["launches"] - i0["launches"]
        kernel_ms = i1["kernel_ms"] - i0["kernel_ms"]
        emit(dict(tool="perf_idty", tag=tag, calc_idty=bool(calc), device_idty=bool(in_place), queries=qs.n, batch=a.queries,
                  inflight=a.inflight, refs=refs.n, wall_s=wall, sequences_per_s=qs.n / wall, busy_host_cores=cpu / wall,
                  compare_launches=s1["compare_launches"] - s0["compare_launches"], compare_ms=s1["compare_ms"] - s0["compare_ms"],
                  inplace_trays=i1["trays"] - i0["trays"], inplace_launches=launches, inplace_sequences=i1["sequences"] - i0["sequences"],
                  inplace_pairs=i1["pairs"] - i0["pairs"], inplace_kernel_ms=kernel_ms,
                  inplace_kernel_ms_per_launch=kernel_ms / launches if launches else 0.0, sampled_results_with_idty=with_idty), a.out)

    legs = ((False, False), (True, False), (True, True))
    for calc, in_place in legs:
        run(calc, in_place, "warm-up")
    for rnd in range(a.rounds):
        for calc, in_place in legs:
            run(calc, in_place, "round %d" % rnd)
    pl.close()
    store.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=9216)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inflight", type=int, default=6)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
