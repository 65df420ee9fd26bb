"""The weighted DP launch alone at bench scale: tools/perf_dp.py's workload (2000 16S references, 9216 queries, one
positional-variability filter) through sina_hip_align_families -- the families are the device k-mer search's top 40,
the DAGs are built on the device.  Prints one JSON line per repetition: DP kernel ms, DAG build ms, Gcell/s.
PERF_LABEL names the build in the output (two builds measured against each other in one session: a copy of this
script beside the other build's package); argv: queries [9216], repetitions [3], weight sets [1] (> 1: the same launch through sina_hip_align_families_wsets
with the queries spread over that many vectors)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sina_amd import synth, capi

nq = int(sys.argv[1]) if len(sys.argv) > 1 else 9216
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
n_sets = int(sys.argv[3]) if len(sys.argv) > 3 else 1
refs = synth.make_refs(2000, length=1500, width=50000, seed=2)
qs = synth.make_queries(refs, nq, seed=3)
ctx = capi.Context(0)
ctx.upload_refs(refs.ab, refs.off, refs.width)
ctx.build_index(10, False)
ids, sc, n = ctx.kmer_topk(qs.mask, qs.off, 40)
fam = np.concatenate([ids[q, :n[q]] for q in range(nq)]).astype(np.uint32)
foff = np.zeros(nq + 1, np.uint64); foff[1:] = np.cumsum(n)
W = np.stack([np.random.default_rng(8 + s).uniform(0.3, 1.4, size=refs.width).astype(np.float32) for s in range(n_sets)])
sets = (np.arange(nq) % n_sets).astype(np.uint32)

def launch():
    if n_sets > 1:
        return ctx.align_families_wsets(fam, foff, qs.mask, qs.off, ctx.params_wsets(W), sets, n_sets)
    return ctx.align_families(fam, foff, qs.mask, qs.off, ctx.params(weights=W[0]))

launch()  # warm-up: buffers, the trace-back planes
for rep in range(reps):
    s0 = ctx.stats()
    t = time.time(); out, pos = launch(); wall = time.time() - t
    s1 = ctx.stats()
    d = {k: s1[k] - s0[k] for k in ("dp_ms", "graph_ms", "backtrack_ms", "dp_cells", "dp_launches")}
    assert (out["status"] == 0).all()
    print(json.dumps({"build": os.environ.get("PERF_LABEL", "this tree"),
                      "kernel": "mesh_dp_kernel<weighted>", "queries": nq, "weight_sets": n_sets, "rep": rep,
                      "dp_ms": round(d["dp_ms"], 3), "graph_ms": round(d["graph_ms"], 3), "backtrack_ms": round(d["backtrack_ms"], 3),
                      "dp_launches": d["dp_launches"], "gcell_per_s": round(d["dp_cells"] / d["dp_ms"] / 1e6, 1),
                      "wall_ms": round(1e3 * wall, 1), "checksum": int(out["end_m"].astype(np.uint64).sum() + pos.astype(np.uint64).sum())}))
