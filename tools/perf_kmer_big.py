"""Searches that want more than 4096 candidates per query: what the big select costs.

usage: tools/perf_kmer_big.py stage  [n_refs ...]     Pipeline.run of 512 queries against 20 000 and 100 000 synthetic
                                                       references with fs-full-len above every reference's length:
                                                       every query escalates 41 -> 410 -> 4100 -> 41 000 -> the store
       tools/perf_kmer_big.py kernel [n_refs] [M ...]  kmer_count_ms / kmer_select_ms per query of one kmer_topk of 512
                                                       queries for M = 4096 (the LDS kernel), 4100, 41 000 and n_refs
       tools/perf_kmer_big.py trace  [n_refs] [M]      one warm-up and three searches at one M and nothing else: run it
                                                       under `rocprofv3 --kernel-trace --stats -- python ...` for the
                                                       split between select kernel, segmented sort and unpack kernel

Uses only calls that exist before the big select did, so the same script times a build without it (there `kernel`
prints "refused" above 4096 and `stage` takes the host's per-query path).  One JSON line per measurement."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from sina_amd import capi, pipeline, synth  # noqa: E402

NQ = 512
LENGTH, WIDTH = 400, 4000


def world(n_refs):
    refs = synth.make_refs(n_refs, length=LENGTH, width=WIDTH, seed=31, long_del_prob=0.0)
    return refs, synth.make_queries(refs, NQ, seed=32)


def stage(n_refs, repeats=3):
    refs, qs = world(n_refs)
    st = pipeline.Store(":mem:perf-big-%d" % n_refs, refs)
    st.build_index(10, False)
    ff = {"fs-min-len": 100, "fs-req-full": 1, "fs-full-len": 2 * LENGTH}
    times = []
    for rep in range(repeats + 1):                       # (the first run grows every buffer: not counted)
        pl = pipeline.Pipeline(st, famfinder=ff)
        s0 = st.stats()
        t = time.perf_counter()
        pl.run(qs.mask, qs.off, batch=NQ, inflight=1)
        dt = time.perf_counter() - t
        s1 = st.stats()
        fam = pl.result(0)["family"]
        pl.close()
        if rep:
            times.append(dt)
        print(json.dumps(dict(what="stage", n_refs=n_refs, nq=NQ, rep=rep, run_s=round(dt, 4),
                              kmer_launches=s1["kmer_launches"] - s0["kmer_launches"],
                              kmer_count_ms=round(s1["kmer_count_ms"] - s0["kmer_count_ms"], 3),
                              kmer_select_ms=round(s1["kmer_select_ms"] - s0["kmer_select_ms"], 3),
                              family_members=len(fam.split()))), flush=True)
    print(json.dumps(dict(what="stage_summary", n_refs=n_refs, nq=NQ, best_s=round(min(times), 4),
                          median_s=round(float(np.median(times)), 4))), flush=True)
    st.close()


def _search(ctx, qs, mx):
    s0 = ctx.stats()
    t = time.perf_counter()
    ids, sc, n = ctx.kmer_topk(qs.mask, qs.off.astype(np.uint64), mx)
    dt = time.perf_counter() - t
    s1 = ctx.stats()
    return dict(wall_s=dt, count_ms=s1["kmer_count_ms"] - s0["kmer_count_ms"], select_ms=s1["kmer_select_ms"] - s0["kmer_select_ms"],
                launches=s1["kmer_launches"] - s0["kmer_launches"], checksum=int(ids.astype(np.uint64).sum()) + int(sc.sum()))


def _context(n_refs):
    refs, qs = world(n_refs)
    ctx = capi.Context(0)
    ctx.upload_refs(refs.ab, refs.off, refs.width)
    ctx.build_index(10, False)
    return ctx, qs


def kernel(n_refs, maxes, repeats=5):
    ctx, qs = _context(n_refs)
    for mx in maxes:
        try:
            _search(ctx, qs, mx)                        # warm-up: buffers, the dense bitmaps
        except capi.SinaHipError as e:
            print(json.dumps(dict(what="kernel", n_refs=n_refs, M=mx, refused=str(e))), flush=True)
            continue
        runs = [_search(ctx, qs, mx) for _ in range(repeats)]
        sel = sorted(r["select_ms"] for r in runs)
        cnt = sorted(r["count_ms"] for r in runs)
        print(json.dumps(dict(what="kernel", n_refs=n_refs, nq=NQ, M=mx, launches=runs[0]["launches"],
                              select_us_per_query=round(1e3 * sel[len(sel) // 2] / NQ, 3),
                              select_us_per_query_min=round(1e3 * sel[0] / NQ, 3),
                              count_us_per_query=round(1e3 * cnt[len(cnt) // 2] / NQ, 3),
                              wall_ms=round(1e3 * float(np.median([r["wall_s"] for r in runs])), 2),
                              checksum=runs[0]["checksum"])), flush=True)
    ctx.close()


def trace(n_refs, mx):
    ctx, qs = _context(n_refs)
    for _ in range(4):
        _search(ctx, qs, mx)
    ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    nums = [int(x) for x in sys.argv[2:]]
    if mode == "stage":
        for n in nums or [20000, 100000]:
            stage(n)
    elif mode == "kernel":
        n = nums[0] if nums else 100000
        kernel(n, nums[1:] or [4096, 4100, 41000, n])
    elif mode == "trace":
        trace(nums[0] if nums else 100000, nums[1] if len(nums) > 1 else 41000)
    else:
        sys.exit(__doc__)
