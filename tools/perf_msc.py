"""A leave-out run (fs-leave-query-out, fs-msc-max 0.9): what the identity filter costs on the host and on the device.

usage: tools/perf_msc.py [n_queries [n_refs]]    the bench's world (100 000 references of 1500 bases in 50 000
                                                  columns), about a thousand queries taken from the references
                                                  themselves -- aligned, under their own names --, through
                                                  Pipeline.run_aligned with famfinder's device-msc off and on,
                                                  and with device-cascade on beside them
       tools/perf_msc.py n_queries n_refs stages  the stage legs only: after a warm-up run of each, device-msc on and
                                                  device-cascade on alternate (the lines of profiles/perf_cascade.txt)
       tools/perf_msc.py n_queries n_refs default the default path instead: queries derived from the references as the
                                                  bench derives them, default options, device-cascade off and on alternating

Per setting: the run's wall time, famfinder's share, the host phases ff.find_batch and ff.match_pass
(SINA_HOST_PROFILE is switched on here), and the match-count kernel's time, pairs and GB/s -- 4 B x the candidates'
bases over the kernel's own time -- against the HBM peak.  Then, in the same session, compare_kernel's GB/s on a sample
of the same (query, candidate) pairs and match_count_kernel's on that sample; last the kernel with other chunk floors
and with one load in flight per lane (SINA_HIP_TEST=match_floor=N;match_loads=1).  One JSON line per measurement.
A stage line also has the cascade kernel's time, queries and candidates, and the bytes a run's rounds brought down:
ids, scores and match counts per candidate listed, or one family row per query and round."""
import json
import os
import re
import sys
import time

os.environ.setdefault("SINA_HOST_PROFILE", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from sina_amd import capi, pipeline, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0        # MI355X: 8 TB/s
FF = {"fs-leave-query-out": 1, "fs-msc-max": 0.9}


def _phase_s(text, name):
    """The wall seconds of one phase in the profile dump (0 if it never ran)."""
    for line in text.splitlines():
        if name in line:
            nums = re.findall(r"[-+]?\d+\.\d+|\d+", line.split(name, 1)[1])
            if nums:
                return float(nums[0])
    return 0.0


def stage(st, q_ab, q_off, names, on, repeats=2, cascade=0, first_rep=0):
    best = None
    for rep in range(first_rep, first_rep + repeats + 1):   # (the first run grows every buffer: not counted)
        pl = pipeline.Pipeline(st, famfinder=dict(FF, **{"device-msc": on, "device-cascade": cascade}))
        pl.profile(reset=True)
        m0, f0 = st.match_stats(), st.family_stats()
        t = time.perf_counter()
        tm = pl.run_aligned(q_ab, q_off, names, batch=len(names), inflight=1)
        dt = time.perf_counter() - t
        m1, f1 = st.match_stats(), st.family_stats()
        prof = pl.profile(reset=True)
        fam = [pl.result(q)["family"] for q in range(min(len(names), 64))]
        pl.close()
        d = {k: m1[k] - m0[k] for k in m1}
        f = {k: f1[k] - f0[k] for k in f1}
        row_bytes = 4 * capi.FamilyRule(fs_msc_max=FF["fs-msc-max"]).row_words
        rec = dict(what="stage", device_msc=on, device_cascade=cascade, nq=len(names), rep=rep, run_s=round(dt, 3),
                   famfinder_s=round(tm["famfinder_s"], 3), find_batch_s=_phase_s(prof, "ff.find_batch"),
                   match_pass_s=_phase_s(prof, "ff.match_pass"), match_kernel_ms=round(d["kernel_ms"], 3),
                   match_pairs=d["pairs"], match_launches=d["launches"],
                   match_gbs=round(4e-6 * d["cand_bases"] / d["kernel_ms"], 1) if d["kernel_ms"] else 0.0,
                   hbm_peak_share=round(4e-6 * d["cand_bases"] / d["kernel_ms"] / HBM_PEAK_GBS, 3) if d["kernel_ms"] else 0.0,
                   cascade_kernel_ms=round(f["kernel_ms"], 3), cascade_queries=f["queries"], cascade_listed=f["candidates_listed"],
                   cascade_scanned=f["candidates_scanned"], cascade_launches=f["launches"],
                   bytes_down=f["queries"] * row_bytes if cascade else d["pairs"] * 10,
                   family_checksum=hash(tuple(fam)) & 0xFFFFFFFF)
        print(json.dumps(rec), flush=True)
        if rep and (best is None or rec["famfinder_s"] < best["famfinder_s"]):
            best = rec
    return best


def default_path(st, refs, nq, turns=3):
    """41 candidates per query: the bench's 16S queries with default options, device-cascade off and on."""
    qs = synth.make_queries(refs, nq, seed=4)
    for turn in range(turns + 1):                        # (turn 0: the warm-up runs)
        for cascade in (0, 1):
            pl = pipeline.Pipeline(st, famfinder={"device-cascade": cascade})
            pl.profile(reset=True)
            f0 = st.family_stats()
            t = time.perf_counter()
            tm = pl.run(qs.mask, qs.off, batch=nq, inflight=1)
            dt = time.perf_counter() - t
            f1 = st.family_stats()
            prof = pl.profile(reset=True)
            fam = [pl.result(q)["family"] for q in range(min(nq, 64))]
            pl.close()
            print(json.dumps(dict(what="default", device_cascade=cascade, nq=nq, rep=turn, run_s=round(dt, 3),
                                  famfinder_s=round(tm["famfinder_s"], 4), find_batch_s=_phase_s(prof, "ff.find_batch"),
                                  match_pass_s=_phase_s(prof, "ff.match_pass"), cascade_kernel_ms=round(f1["kernel_ms"] - f0["kernel_ms"], 3),
                                  cascade_queries=f1["queries"] - f0["queries"], family_checksum=hash(tuple(fam)) & 0xFFFFFFFF)), flush=True)


def kernels(refs, q_ab, q_off, n_sample=64, per_query=4100, repeats=3):
    """compare_kernel and match_count_kernel on the same pairs: n_sample queries x their top per_query candidates."""
    ctx = capi.Context(0)
    ctx.upload_refs(refs.ab, refs.off.astype(np.uint64), refs.width)
    ctx.build_index(10, False)
    nq = min(n_sample, len(q_off) - 1)
    ab, off = q_ab[:int(q_off[nq])], q_off[:nq + 1]
    ids, sc, n, mt = ctx.kmer_topk_match(ab, off, per_query)
    cand = np.ascontiguousarray(ids.reshape(-1))
    c_off = (np.arange(nq + 1) * ids.shape[1]).astype(np.uint64)
    bases = int(np.diff(refs.off)[cand].sum())
    for rep in range(repeats + 1):
        s0, m0 = ctx.stats(), ctx.match_stats()
        six = ctx.compare(ab, off, cand, c_off, 0, False)
        s1 = ctx.stats()
        got = ctx.match_counts(ab, off, cand, c_off)
        m1 = ctx.match_stats()
        assert (six[:, 4] == got).all() and (got == mt.reshape(-1)).all()
        if rep:
            cmp_ms, mc_ms = s1["compare_ms"] - s0["compare_ms"], m1["kernel_ms"] - m0["kernel_ms"]
            print(json.dumps(dict(what="kernels", nq=nq, pairs=len(cand), cand_bases=bases, rep=rep,
                                  compare_kernel_ms=round(cmp_ms, 3), compare_gbs=round(4e-6 * bases / cmp_ms, 1),
                                  match_kernel_ms=round(mc_ms, 3), match_gbs=round(4e-6 * bases / mc_ms, 1))), flush=True)
    ctx.close()


def _knobs(**kw):
    cur = dict(x.split("=", 1) for x in os.environ.get("SINA_HIP_TEST", "").split(";") if "=" in x)
    for k, v in kw.items():
        cur.pop(k, None)
        if v is not None:
            cur[k] = str(v)
    os.environ["SINA_HIP_TEST"] = ";".join("%s=%s" % kv for kv in cur.items())


def variants(refs, q_ab, q_off, repeats=3):
    """The chunk floor and the loads in flight the kernel was built with, each beside its alternatives, on the shapes
    where they matter: one tray and four trays of 41 000 candidates (the floor decides the grid), and 64 queries of
    4100 (chunks above any floor: the loads alone)."""
    ctx = capi.Context(0)
    ctx.upload_refs(refs.ab, refs.off.astype(np.uint64), refs.width)
    ctx.build_index(10, False)
    for nq, per_query in ((1, 41000), (4, 41000), (64, 4100)):
        ab, off = q_ab[:int(q_off[nq])], q_off[:nq + 1]
        ids, sc, n, mt = ctx.kmer_topk_match(ab, off, per_query)
        cand = np.ascontiguousarray(ids.reshape(-1))
        c_off = (np.arange(nq + 1) * ids.shape[1]).astype(np.uint64)
        bases = int(np.diff(refs.off)[cand].sum())
        for floor, loads in ((64, 4), (16, 4), (256, 4), (1024, 4), (64, 1)):
            _knobs(match_floor=floor, match_loads=loads)
            ms = []
            for rep in range(repeats + 1):
                m0 = ctx.match_stats()
                got = ctx.match_counts(ab, off, cand, c_off)
                ms.append(ctx.match_stats()["kernel_ms"] - m0["kernel_ms"])
                assert (got == mt.reshape(-1)).all()
            best = min(ms[1:])
            print(json.dumps(dict(what="variant", nq=nq, per_query=per_query, floor=floor, loads=loads,
                                  kernel_ms=round(best, 4), gbs=round(4e-6 * bases / best, 1))), flush=True)
        _knobs(match_floor=None, match_loads=None)
    ctx.close()


if __name__ == "__main__":
    nq = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    n_refs = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    refs = synth.make_refs(n_refs, length=1500, width=50000, seed=2)
    pick = np.random.default_rng(3).choice(n_refs, size=nq, replace=False)
    seqs = [refs.seq(int(i)) for i in pick]
    names = ["ref%d" % int(i) for i in pick]
    q_ab = np.concatenate(seqs).astype(np.uint32)
    q_off = np.zeros(nq + 1, np.uint64)
    q_off[1:] = np.cumsum([len(s) for s in seqs])
    st = pipeline.Store(":mem:perf-msc", refs)
    st.build_index(10, False)
    if len(sys.argv) > 3 and sys.argv[3] == "default":
        default_path(st, refs, nq)
        st.close()
        sys.exit(0)
    if len(sys.argv) > 3 and sys.argv[3] == "stages":
        stage(st, q_ab, q_off, names, 1, repeats=0)                  # the warm-up runs
        stage(st, q_ab, q_off, names, 1, repeats=0, cascade=1)
        for turn in range(1, 4):
            stage(st, q_ab, q_off, names, 1, repeats=0, first_rep=turn)
            stage(st, q_ab, q_off, names, 1, repeats=0, cascade=1, first_rep=turn)
        st.close()
        sys.exit(0)
    off_run = stage(st, q_ab, q_off, names, 0)
    on_run = stage(st, q_ab, q_off, names, 1)
    cascade_run = stage(st, q_ab, q_off, names, 1, cascade=1)
    print(json.dumps(dict(what="summary", nq=nq, n_refs=n_refs, famfinder_off_s=off_run["famfinder_s"],
                          famfinder_on_s=on_run["famfinder_s"],
                          ratio=round(off_run["famfinder_s"] / on_run["famfinder_s"], 2),
                          famfinder_cascade_s=cascade_run["famfinder_s"],
                          same_families=off_run["family_checksum"] == on_run["family_checksum"] == cascade_run["family_checksum"])), flush=True)
    st.close()
    kernels(refs, q_ab, q_off)
    variants(refs, q_ab, q_off)
