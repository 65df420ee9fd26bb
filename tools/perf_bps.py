"""The helix base-pair score (align_bp_score_slv) on the bench's 16S shape: store and queries from
sina_amd/synth.py, a nested random helix map of about 450 pairs.

    python tools/perf_bps.py host     [--seqs 2000] [--out FILE]     the host walk per sequence on one core (no GPU)
    python tools/perf_bps.py kernel   [--seqs 9216] [--out FILE]     pair_count_kernel alone, and the call around it
    python tools/perf_bps.py pipeline [--queries 9216] [--steps 4] [--refs 100000] [--rounds 2] [--out FILE]
                                                                     Pipeline.run without a helix map, with one
                                                                     (the finished alignments uploaded again) and with
                                                                     one counted where the device assembles them
                                                                     (aligner device-bps); the three legs alternate

Every mode prints JSON lines; --out appends them to FILE (profiles/perf_bps.txt)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

LENGTH, WIDTH, N_PAIRS = 1500, 50000, 450


def helix_map(width=WIDTH, n_pairs=N_PAIRS, seed=11):
    """A symmetric map of n_pairs nested pairs over random columns."""
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.choice(np.arange(1, width), size=2 * n_pairs, replace=False))
    m = np.zeros(width, np.uint32)
    for k in range(n_pairs):
        a, b = int(cols[k]), int(cols[2 * n_pairs - 1 - k])
        m[a], m[b] = b, a
    return m


def aligned_batch(n, seed=2):
    """n aligned 16S-like sequences as (q_ab, q_off): the synthetic references themselves."""
    from sina_amd import synth
    refs = synth.make_refs(n, length=LENGTH, width=WIDTH, seed=seed)
    return np.ascontiguousarray(refs.ab, np.uint32), np.ascontiguousarray(refs.off, np.uint64)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def host(a):
    from sina_amd import pipeline
    q_ab, q_off = aligned_batch(a.seqs)
    m = helix_map()
    pipeline.host_pair_scores(q_ab, q_off[:65], m)                  # (warm-up)
    best = min(pipeline.host_pair_scores(q_ab, q_off, m)[2] for _ in range(5))
    emit(dict(mode="host", what="cseq_base::calcPairScore, one thread, the sequences already built", sequences=a.seqs,
              bases_per_sequence=float(q_off[-1]) / a.seqs, map_entries=int(np.count_nonzero(m)),
              us_per_sequence=1e6 * best / a.seqs, repeats=5, taken="min"), a.out)


def kernel(a):
    from sina_amd import capi
    q_ab, q_off = aligned_batch(a.seqs)
    m = helix_map()
    ctx = capi.Context(0)
    ctx.upload_pairs(m)
    counts = ctx.pair_counts(q_ab, q_off)                           # (warm-up: buffers)
    reps = 10
    s0 = ctx.pair_stats()
    t = time.perf_counter()
    for _ in range(reps):
        ctx.pair_counts(q_ab, q_off, out=counts)
    wall_ms = 1e3 * (time.perf_counter() - t) / reps
    s1 = ctx.pair_stats()
    ms = (s1["kernel_ms"] - s0["kernel_ms"]) / reps
    emit(dict(mode="kernel", kernel="pair_count_kernel", sequences_per_launch=a.seqs, map_entries=int(np.count_nonzero(m)),
              words_per_launch=int(q_off[-1]), kernel_ms_per_launch=ms, call_wall_ms=wall_ms,
              # the call around the kernel: staging copy, upload of the words and offsets, download of the counters, waits
              call_minus_kernel_ms=wall_ms - ms, kernel_share_of_call=ms / wall_ms, bytes_up=4 * int(q_off[-1]) + 8 * (a.seqs + 1),
              bytes_down=24 * a.seqs, us_per_sequence_kernel=1e3 * ms / a.seqs, us_per_sequence_call=1e3 * wall_ms / a.seqs,
              launches=(s1["launches"] - s0["launches"]) // reps, repeats=reps), a.out)
    ctx.close()


def pipeline_mode(a):
    from sina_amd import pipeline, synth
    refs = synth.make_refs(a.refs, length=LENGTH, width=WIDTH, seed=2)
    qs = synth.make_queries(refs, a.queries * a.steps, seed=3)
    store = pipeline.Store(":mem:perf-bps", refs)
    store.build_index(10, False)
    m = helix_map()
    pl = pipeline.Pipeline(store)

    def run(with_map, tag, in_place=False):
        store.set_pairs(m if with_map else np.zeros(0, np.uint32))
        pl._set("aligner", "device-bps", bool(in_place))
        p0, i0 = store.pair_stats(), store.pair_inplace_stats()
        c0, t0 = os.times(), time.perf_counter()
        pl.run(qs.mask, qs.off, batch=a.queries, inflight=a.inflight)
        wall = time.perf_counter() - t0
        c1 = os.times()
        p1, i1 = store.pair_stats(), store.pair_inplace_stats()
        cpu = (c1.user - c0.user) + (c1.system - c0.system)
        nz = sum(1 for q in range(0, qs.n, 97) if pl.result(q)["bp_score"] != 0)
        emit(dict(mode="pipeline", tag=tag, helix_map=bool(with_map), device_bps=bool(in_place), queries=qs.n, batch=a.queries,
                  inflight=a.inflight, refs=refs.n, wall_s=wall, sequences_per_s=qs.n / wall, busy_host_cores=cpu / wall,
                  pair_launches=p1["launches"] - p0["launches"], pair_kernel_ms=p1["kernel_ms"] - p0["kernel_ms"],
                  pair_sequences=p1["sequences"] - p0["sequences"],
                  inplace_trays=i1["trays"] - i0["trays"], inplace_launches=i1["launches"] - i0["launches"],
                  inplace_kernel_ms=i1["kernel_ms"] - i0["kernel_ms"], inplace_sequences=i1["sequences"] - i0["sequences"],
                  sampled_results_with_a_score=nz), a.out)

    run(False, "warm-up")
    run(True, "warm-up")
    run(True, "warm-up", in_place=True)
    for rnd in range(a.rounds):
        run(False, "round %d" % rnd)
        run(True, "round %d" % rnd)
        run(True, "round %d" % rnd, in_place=True)
    pl.close()
    store.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["host", "kernel", "pipeline"])
    ap.add_argument("--seqs", type=int, default=0)
    ap.add_argument("--queries", type=int, default=9216)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--inflight", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.seqs == 0:
        a.seqs = 2000 if a.mode == "host" else 9216
    {"host": host, "kernel": kernel, "pipeline": pipeline_mode}[a.mode](a)
