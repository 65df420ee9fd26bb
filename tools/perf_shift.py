"""The device assembly with shifted insertions (aligner device-shift, sina_hip_align_params::assemble == 2;
DESIGN.md 3.2) on a store laid out like a curated alignment: 16S-sized references whose bases occupy blocks of B
consecutive columns with G free columns between the blocks, where an insertion rarely finds a free column beside it.

    python tools/perf_shift.py kernel   [--queries 9216] [--reps 10] [--out FILE]
        assemble_kernel alone (sina_hip_debug_assemble, events around the kernel) on the emitted columns of one real
        launch range -- its two instantiations on the same input, launches alternating: median and slowest launch
    python tools/perf_shift.py pipeline [--queries 9216] [--steps 2] [--refs 20000] [--rounds 2] [--out FILE]
        Pipeline.run with device-shift off and on, and the same with device-bps; the four legs alternate:
        sequences per second, busy host cores, the share of trays the device had assembled

Every mode prints JSON lines; --out appends them to FILE (profiles/perf_shift.txt)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

LENGTH, BLOCK, FREE = 1500, 50, 20


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def block_store(n_refs, seed=2):
    """synth.make_refs without insertions, base i of the ancestor moved to column i + FREE * (i // BLOCK)."""
    from sina_amd import synth
    refs = synth.make_refs(n_refs, length=LENGTH, width=2 * LENGTH, seed=seed, ins_rate=0.0)
    i = (refs.ab & 0xFFFFFF) // 2
    ab = ((i + FREE * (i // BLOCK)).astype(np.uint32) | (refs.ab & 0xFF000000)).astype(np.uint32)
    return synth.RefSet(ab=ab, off=refs.off, width=LENGTH + FREE * (LENGTH // BLOCK) + FREE)


def helix_map(width, n_pairs=450, seed=11):
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.choice(np.arange(1, width), size=2 * n_pairs, replace=False))
    m = np.zeros(width, np.uint32)
    for k in range(n_pairs):
        a, b = int(cols[k]), int(cols[2 * n_pairs - 1 - k])
        m[a], m[b] = b, a
    return m


def kernel(a):
    """One launch range's walk output (align_families, assemble = 0) through the assembly alone, both ways."""
    from sina_amd import capi, synth
    refs = block_store(2000)
    qs = synth.make_queries(refs, a.queries, seed=3)
    rng = np.random.default_rng(4)
    fam_off = np.arange(a.queries + 1, dtype=np.uint64) * 40
    fam_ids = np.concatenate([np.concatenate([[qs.src[q]], rng.choice(refs.n, size=39, replace=False)]) for q in range(qs.n)]).astype(np.uint32)
    ctx = capi.Context(0)
    ctx.upload_refs(refs.ab, refs.off, refs.width)
    qmask, qoff = qs.mask & 0x0F, qs.off.astype(np.uint64)
    out, pos = ctx.align_families(fam_ids, fam_off, qmask, qoff, ctx.params(lowercase=2, assemble=0))
    ms = {1: [], 2: []}
    res = {}
    for rep in range(a.reps + 1):                       # (the first pair: warm-up)
        for mode in (1, 2):
            o, p = ctx.debug_assemble(ctx.params(lowercase=2, assemble=mode), refs.width, qmask, qoff, out, pos)
            if rep:
                ms[mode].append(ctx.debug_assemble_ms())
            res[mode] = (o, ctx.staged_shift_log())
    runs = [len(e) for e in res[2][1]]
    for mode in (1, 2):
        o = res[mode][0]
        emit(dict(mode="kernel", kernel="assemble_kernel<%s>" % ("true" if mode == 2 else "false"), assemble=mode, queries=a.queries,
                  bases_per_query=float(qoff[-1]) / a.queries, block=BLOCK, free=FREE, width=refs.width,
                  assembled_share=float((o["assembled"] != 0).mean()), shifted_runs_per_query_mean=float(np.mean(runs)) if mode == 2 else 0.0,
                  shifted_runs_per_query_max=int(max(runs)) if mode == 2 else 0,
                  kernel_ms_median=float(np.median(ms[mode])), kernel_ms_slowest=float(max(ms[mode])), kernel_ms_fastest=float(min(ms[mode])),
                  launches=a.reps), a.out)
    ctx.close()


def pipeline_mode(a):
    from sina_amd import pipeline, synth
    refs = block_store(a.refs)
    qs = synth.make_queries(refs, a.queries * a.steps, seed=3)
    store = pipeline.Store(":mem:perf-shift", refs)
    store.build_index(10, False)
    store.set_pairs(helix_map(refs.width))
    pl = pipeline.Pipeline(store)

    def run(shift, bps, tag):
        pl._set("aligner", "device-shift", bool(shift))
        pl._set("aligner", "device-bps", bool(bps))
        s0, i0 = store.assemble_stats(), store.pair_inplace_stats()
        c0, t0 = os.times(), time.perf_counter()
        pl.run(qs.mask, qs.off, batch=a.queries, inflight=a.inflight)
        wall = time.perf_counter() - t0
        c1 = os.times()
        s1, i1 = store.assemble_stats(), store.pair_inplace_stats()
        d = {k: s1[k] - s0[k] for k in s0}
        trays = d["trays_device"] + d["trays_host"]
        emit(dict(mode="pipeline", tag=tag, device_shift=bool(shift), device_bps=bool(bps), queries=qs.n, batch=a.queries,
                  inflight=a.inflight, refs=refs.n, block=BLOCK, free=FREE, width=refs.width, wall_s=wall, sequences_per_s=qs.n / wall,
                  busy_host_cores=((c1.user - c0.user) + (c1.system - c0.system)) / wall,
                  assembled_share=d["trays_device"] / trays if trays else 0.0, host_finished_trays=d["trays_host"],
                  shifted_queries=d["shifted_queries"], shifted_runs=d["shifted_runs"],
                  inplace_bps_trays=i1["trays"] - i0["trays"]), a.out)

    legs = [(0, 0), (1, 0), (0, 1), (1, 1)]
    for shift, bps in legs:
        run(shift, bps, "warm-up")
    for rnd in range(a.rounds):
        for shift, bps in legs:
            run(shift, bps, "round %d" % rnd)
    pl.close()
    store.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "pipeline"])
    ap.add_argument("--queries", type=int, default=9216)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--refs", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inflight", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"kernel": kernel, "pipeline": pipeline_mode}[a.mode](a)
