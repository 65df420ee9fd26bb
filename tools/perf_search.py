"""The search stage in a pipeline, without and with `device-rank` and with the aligner's `device-search`
(3.5d), and the comparison kernel alone.

    python tools/perf_search.py stage [--queries 9216] [--refs 100000] [--search-all] [--rounds 3] [--out FILE]

runs famfinder -> aligner -> search_filter (lca-fields set) over the bench's world in ONE process: a warm-up pass with
each setting, then `--rounds` rounds that alternate the three settings: device-rank off, device-rank on, and device-rank
on with the aligner's device-search and device-shift (the rows come back with the alignments; the stage's own path
takes the trays the device did not rank).  Per run one JSON line: the pipeline's sequences per second and busy host
cores, the stage's wall seconds (Pipeline.search_seconds()), its host phases (SINA_HOST_PROFILE), the kernels'
milliseconds by events with their algorithmic bytes (4 B per candidate base) over that time, and the bytes the stage's
device calls copy each way (computed from the entries' contracts: ids, scores and counters per candidate off; rows per
query on; in place nothing up and a 520-byte row per query down, plus the rest's share of the device-rank route).  All
search results of the three settings are compared; a last line says whether they are identical.  --out appends the raw
lines.

    python tools/perf_search.py [nq] [n_refs]

is the comparison kernel alone at bench scale, as before: 1000 k-mer candidates per aligned query; one JSON line with
pairs/s, candidate bases/s, achieved HBM GB/s and the oracle's rate on a few queries."""
import json, os, re, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def kernel_alone(nq, n_refs):
    from sina_amd import synth, capi
    ncand = 1000
    refs = synth.make_refs(n_refs, length=1500, width=50000, seed=2)
    rng = np.random.default_rng(5)
    src = rng.integers(0, refs.n, size=nq)
    qs_ab, masks = [], []
    for i in src:                                  # aligned queries: a reference with 3 % substitutions
        ab = refs.seq(int(i)).copy()
        sub = rng.random(len(ab)) < 0.03
        ab[sub] = (ab[sub] & 0xFFFFFF) | (rng.choice([1, 2, 4, 8], size=int(sub.sum())).astype(np.uint32) << 24)
        qs_ab.append(ab)
        masks.append(((ab >> 24) & 0x0f).astype(np.uint8))
    q_off = np.zeros(nq + 1, np.uint64); q_off[1:] = np.cumsum([len(x) for x in qs_ab])
    ctx = capi.Context(0)
    ctx.upload_refs(refs.ab, refs.off, refs.width)
    ctx.build_index(10, False)
    ids, sc, n = ctx.kmer_topk(np.concatenate(masks), q_off, ncand)
    cand = np.concatenate([ids[q, :n[q]] for q in range(nq)]).astype(np.uint32)
    c_off = np.zeros(nq + 1, np.uint64); c_off[1:] = np.cumsum(n)
    flat = np.concatenate(qs_ab)
    ctx.compare(flat, q_off, cand, c_off, 0, False)          # warm-up (buffers)
    s0 = ctx.stats()
    reps = 5
    t = time.time()
    for _ in range(reps):
        got = ctx.compare(flat, q_off, cand, c_off, 0, False)
    wall = (time.time() - t) / reps
    s1 = ctx.stats()
    ms = (s1["compare_ms"] - s0["compare_ms"]) / reps
    bases = (s1["compare_bases"] - s0["compare_bases"]) / reps
    out = {"kernel": "compare_kernel", "queries_per_launch": nq, "candidates_per_query": ncand, "n_refs": n_refs,
           "ms_per_launch": ms, "wall_ms_per_call": 1e3 * wall, "pairs_per_s": len(cand) / (ms * 1e-3),
           "roofline": {"bound": "hbm", "achieved": 4 * bases / (ms * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
                        "frac": 4 * bases / (ms * 1e-3) / 1e9 / 8000.0, "algorithmic_bytes_per_launch": 4 * bases}}
    try:  # CPU baseline: the oracle's literal traverse on a bounded sample (test infrastructure, not the product)
        from oracle import pyoracle as po
        take = 8
        need = sorted({int(r) for q in range(take) for r in ids[q, :n[q]]})
        cs = {r: po.Cseq.from_packed("ref%d" % r, refs.seq(r), refs.width) for r in need}
        t = time.time(); pairs = 0
        for q in range(take):
            qc = po.Cseq.from_packed("q", qs_ab[q], refs.width)
            for x, r in enumerate(ids[q, :n[q]]):
                want = po.compare_counts(qc, cs[int(r)])
                assert tuple(got[int(c_off[q]) + x]) == want
                pairs += 1
        dt = time.time() - t
        out["cpu_baseline"] = {"value": pairs / dt, "unit": "pairs/s", "cores": 1, "kind": "port",
                               "sample": "%d queries x %d candidates through the oracle's traverse() via ctypes "
                                         "(includes the Python call overhead), all equal to the GPU counters" % (take, ncand)}
    except ImportError:
        pass
    print(json.dumps(out))


def stage(argv):
    import argparse
    ap = argparse.ArgumentParser(prog="perf_search.py stage")
    ap.add_argument("--queries", type=int, default=9216)
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--length", type=int, default=1500)
    ap.add_argument("--width", type=int, default=50000)
    ap.add_argument("--search-all", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    os.environ["SINA_HOST_PROFILE"] = "1"          # (read when the host library is loaded)
    from sina_amd import synth, pipeline

    refs = synth.make_refs(a.refs, length=a.length, width=a.width, seed=2)
    qs = synth.make_queries(refs, a.queries, seed=3)
    store = pipeline.Store(":mem:perf-search", refs)
    for i in range(refs.n):
        store.set_attr(i, "tax_slv", "Bacteria;phylum%d;class%d;order%d;" % (i % 3, i % 11, i % 41))
    store.build_index(10, False)
    sopts = {"lca-fields": "tax_slv"}
    if a.search_all:
        sopts["search-all"] = True
    pl = pipeline.Pipeline(store, search=sopts)
    n_best, kmer_cand = 10, min(1000, refs.n)
    phases = ("sf.find_batch", "sf.compare(C-ABI)", "sf.device_rank(C-ABI)", "sf.rank+lca")
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def results():
        out = []
        for q in range(qs.n):
            r = pl.result(q)
            if r["search_ids"] is None:
                out.append(None)
            else:
                out.append((r["search_ids"].tobytes(), r["search_scores"].tobytes(), pl.attr(q, "nearest_slv"), pl.attr(q, "lca_tax_slv")))
        return out

    def run(on, tag, in_place=False):
        pl._set("search", "device-rank", bool(on))
        pl._set("aligner", "device-search", bool(in_place))
        pl._set("aligner", "device-shift", bool(in_place))
        pl.profile(reset=True)
        s0, r0, i0 = store.stats(), store.rank_stats(), store.search_inplace_stats()
        t, cpu = time.time(), time.process_time()
        pl.run(qs.mask, qs.off, batch=a.batch, inflight=a.inflight)
        wall, cpu = time.time() - t, time.process_time() - cpu
        s1, r1, i1 = store.stats(), store.rank_stats(), store.search_inplace_stats()
        prof = {}
        for ln in pl.profile(reset=True).splitlines():
            m = re.match(r"^(.*?)\s+([0-9.]+) s\s+[0-9]+ calls$", ln)
            if m and m.group(1).split(" ")[0] in phases:
                prof[m.group(1)] = float(m.group(2))
        res = results()
        searched = sum(r is not None for r in res)
        pairs_off = searched * (refs.n if a.search_all else kmer_cand)
        rec = dict(tag=tag, device_rank=bool(on), device_search=bool(in_place), queries=qs.n, searched=searched, refs=refs.n,
                   search_all=bool(a.search_all), wall_s=wall, sequences_per_s=qs.n / wall, busy_host_cores=cpu / wall,
                   search_seconds=pl.search_seconds(), phases=prof)
        trays = i1["trays"] - i0["trays"]
        if in_place:
            # nothing goes up again for a tray ranked in place; its slot's 520-byte row came down with the alignment
            rec.update(in_place_trays=trays, rank_inplace_kernel_ms=i1["kernel_ms"] - i0["kernel_ms"],
                       rank_inplace_launches=i1["launches"] - i0["launches"], rank_inplace_sequences=i1["sequences"] - i0["sequences"],
                       rank_inplace_pairs=i1["pairs"] - i0["pairs"], in_place_bytes_up=0,
                       in_place_bytes_down=520 * (i1["sequences"] - i0["sequences"]))
        if on:
            ms, bases = r1["kernel_ms"] - r0["kernel_ms"], r1["cand_bases"] - r0["cand_bases"]
            rec.update(ranked=r1["ranked"] - r0["ranked"], fallen_back=r1["fallen_back"] - r0["fallen_back"],
                       rank_kernel_ms=ms, rank_launches=r1["launches"] - r0["launches"], pairs=r1["pairs"] - r0["pairs"],
                       # up: the queries' packed bases; down: max_result ids and scores, a count and a flag per query
                       # (in place: only the trays the stage's own path still takes -- their share of the bases)
                       bytes_up=4 * int(qs.off[-1]) * (searched - trays) // max(searched, 1), bytes_down=(searched - trays) * (8 * n_best + 8))
        else:
            ms, bases = s1["compare_ms"] - s0["compare_ms"], s1["compare_bases"] - s0["compare_bases"]
            rec.update(compare_kernel_ms=ms, compare_launches=s1["compare_launches"] - s0["compare_launches"], pairs=pairs_off,
                       # up: the queries' packed bases and the candidates' ids (search-all: n_refs ids per query);
                       # down: the k-mer search's ids and scores (not with search-all) and 24 bytes of counters per pair
                       bytes_up=4 * int(qs.off[-1]) + 4 * pairs_off, bytes_down=(24 + (0 if a.search_all else 8)) * pairs_off)
        rec.update(kernel_ms=ms, algorithmic_bytes=4 * bases, kernel_GBps=(4 * bases / (ms * 1e-3) / 1e9) if ms > 0 else None)
        emit(rec)
        return res

    base = run(False, "warm-up")
    same = run(True, "warm-up") == base
    same = (run(True, "warm-up", in_place=True) == base) and same
    for rnd in range(a.rounds):
        same = (run(False, "round %d" % rnd) == base) and same
        same = (run(True, "round %d" % rnd) == base) and same
        same = (run(True, "round %d" % rnd, in_place=True) == base) and same
    emit(dict(tag="results", identical_between_settings=bool(same), queries_with_results=sum(r is not None for r in base)))
    if a.out:
        with open(a.out, "a") as f:
            f.write("tools/perf_search.py stage " + " ".join(argv) + "\n" + "\n".join(lines) + "\n")
    pl.close()
    store.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "stage":
        stage(sys.argv[2:])
    else:
        kernel_alone(int(sys.argv[1]) if len(sys.argv) > 1 else 2048, int(sys.argv[2]) if len(sys.argv) > 2 else 100000)
