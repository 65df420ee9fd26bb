"""A mixed-filter pipeline run: 16S references in three unrelated groups (80 / 15 / 5 %) with a taxonomy field, one
positional-variability filter per group, famfinder's auto-filter-field on, batches of 9216 queries -- the aligner's
weight-sets on (one DP launch per batch for the weighted trays) against off (one per filter).  Prints one JSON line
per run: sequences/s, DP launches, DAG-build launches.  argv: batches [4], repetitions of each setting [3], batches in flight [1]."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sina_amd import synth, pipeline

n_batches = int(sys.argv[1]) if len(sys.argv) > 1 else 4
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
inflight = int(sys.argv[3]) if len(sys.argv) > 3 else 1   # (two weighted 16S batches in flight hold two trace-back planes of 105-118 GB)
batch = 9216
groups = (("Bacteria;Proteobacteria", "pv:Bacteria", 1600), ("Archaea;Euryarchaeota", "pv:Archaea;Eury", 300),
          ("Archaea;Crenarchaeota", "pv:Archaea;Cren", 100))
parts = [synth.make_refs(n, length=1500, width=50000, seed=40 + x) for x, (_, _, n) in enumerate(groups)]
off = [np.zeros(1, np.int64)]
for p in parts:
    off.append(p.off[1:] + off[-1][-1])
refs = synth.RefSet(ab=np.concatenate([p.ab for p in parts]), off=np.concatenate(off), width=50000)
qs = synth.make_queries(refs, n_batches * batch, seed=44)
st = pipeline.Store(":mem:perf-autofilter", refs)
lo = 0
for x, (tax, name, n) in enumerate(groups):
    for i in range(lo, lo + n):
        st.set_attr(i, "tax_slv", tax)
    st.add_filter(name, np.random.default_rng(50 + x).uniform(0.3, 1.4, size=refs.width).astype(np.float32))
    lo += n
share = [float(((qs.src >= a) & (qs.src < b)).mean()) for a, b in ((0, 1600), (1600, 1900), (1900, 2000))]
ff = {"filter": "pv", "auto-filter-field": "tax_slv"}
sums = {}
for rep in range(reps + 1):          # (the first pass of each setting warms the contexts and is not reported)
    for ws in (True, False):
        pl = pipeline.Pipeline(st, famfinder=ff, aligner={"weight-sets": ws})
        s0 = st.stats()
        t = pl.run(qs.mask, qs.off, batch=batch, inflight=inflight)
        s1 = st.stats()
        chosen = [pl.attr(q, "align_filter_slv") for q in range(0, qs.n, 97)]
        sums[ws] = sum(int(pl.result(q)["packed"].astype(np.uint64).sum()) for q in range(0, qs.n, 97))
        pl.close()
        if rep == 0:
            continue
        print(json.dumps({"run": "mixed-filter pipeline", "weight_sets": ws, "rep": rep - 1, "queries": qs.n, "batch": batch, "inflight": inflight,
                          "query_share_by_group": [round(x, 3) for x in share], "seq_per_s": round(qs.n / t["wall_s"], 1),
                          "wall_s": round(t["wall_s"], 4), "dp_launches": s1["dp_launches"] - s0["dp_launches"],
                          "graph_launches": s1["graph_launches"] - s0["graph_launches"],
                          "dp_ms": round(s1["dp_ms"] - s0["dp_ms"], 2), "graph_ms": round(s1["graph_ms"] - s0["graph_ms"], 2),
                          "filters_seen": sorted(set(chosen)), "checksum": sums[ws]}))
assert sums[True] == sums[False], "weight-sets on and off gave different alignments"
st.close()
