"""famfinder's --turn on the device (famfinder option device-turn) on the bench's 16S shape: store and
queries from sina_amd/synth.py as bench.py builds them, every second query handed in reversed and complemented.

    python tools/perf_turn.py [--queries 9216] [--steps 2] [--refs 100000] [--rounds 3] [--inflight 6] [--out FILE]

turn = revcomp and turn = all, each timed with the option off (the host makes the variants, one top-1 search over all
of them, then the first round searches the chosen one again) and on (one sina_hip_kmer_topk_turn call), the two legs
alternating after a warm-up run of each.  Per run: sequences/s, busy host cores (process CPU seconds / wall seconds),
famfinder's seconds summed over the batches, and of these (SINA_HOST_PROFILE, set here) the orientation step, ff.orient
-- with the option on it holds the first round's search -- and ff.find_batch, the searches of the rounds (with the
option on the turn call is one of them; off, the orientation's own top-1 search is outside it); the orient and pick
kernels' milliseconds and launches, the trays by route, and how many inputs came out turned.

Prints JSON lines; --out appends them to FILE (profiles/perf_turn.txt)."""
import argparse
import json
import os
import re
import sys
import time

os.environ.setdefault("SINA_HOST_PROFILE", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LENGTH, WIDTH = 1500, 50000


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def phase_seconds(text, name):
    m = re.search(r"^%s\s+([0-9.]+) s" % re.escape(name), text, re.M)
    return float(m.group(1)) if m else 0.0


def main(a):
    import numpy as np
    from sina_amd import pipeline, synth
    refs = synth.make_refs(a.refs, length=LENGTH, width=WIDTH, seed=2)
    base = synth.make_queries(refs, a.queries * a.steps, seed=3)
    comp = np.array([((m & 2) << 1) | ((m & 4) >> 1) | ((m & 1) << 3) | ((m & 8) >> 3) | (m & 16) for m in range(32)], np.uint8)
    masks = [comp[base.seq(q)[::-1]] if q % 2 else base.seq(q) for q in range(base.n)]       # (lengths, hence offsets, stay)
    qmask = np.concatenate(masks)
    store = pipeline.Store(":mem:perf-turn", refs)
    store.build_index(10, False)
    pl = pipeline.Pipeline(store)

    def run(mode, on, tag):
        pl._set("famfinder", "turn", mode)
        pl._set("famfinder", "device-turn", bool(on))
        pl.profile(reset=True)
        s0 = store.turn_stats()
        c0, t0 = os.times(), time.perf_counter()
        pl.run(qmask, base.off, batch=a.queries, inflight=a.inflight)
        wall = time.perf_counter() - t0
        c1 = os.times()
        s1 = store.turn_stats()
        prof = pl.profile(reset=True)
        d = {k: s1[k] - s0[k] for k in s1}
        cpu = (c1.user - c0.user) + (c1.system - c0.system)
        turned = sum(1 for q in range(base.n) if pl.attr(q, "turn") == "reversed and complemented")
        emit(dict(turn=mode, tag=tag, device_turn=bool(on), queries=base.n, batch=a.queries, inflight=a.inflight, refs=refs.n,
                  wall_s=wall, sequences_per_s=base.n / wall, busy_host_cores=cpu / wall, famfinder_s=pl.timings()["famfinder_s"],
                  orient_s=phase_seconds(prof, "ff.orient"), find_batch_s=phase_seconds(prof, "ff.find_batch"),
                  turned_trays=turned, rows_trays=d["rows_trays"], orient_trays=d["orient_trays"], fallback_trays=d["fallback_trays"],
                  kernel_queries=d["queries"], launches=d["launches"], kernel_ms=d["kernel_ms"]), a.out)

    for mode in ("revcomp", "all"):
        for on in (False, True):
            run(mode, on, "warm-up")
    for rnd in range(a.rounds):
        for mode in ("revcomp", "all"):
            run(mode, False, "round %d" % rnd)
            run(mode, True, "round %d" % rnd)
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
