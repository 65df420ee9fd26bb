"""The stages with every device option on at once: device-bps, device-idty, device-shift, device-search and
wide-fallback on the aligner, device-msc and device-cascade on famfinder, device-rank on the search stage -- against
the same run with all of them off, on the small world of tests/shift_cases.py (48 references laid out in blocks, 18
queries of which two are beyond the shift log's cap and host-finished whatever the options say), and on the long-query
world of tests/test_gpu_long.py.

No two of these options exclude each other by the host's rules (plan_counting and plan_search_inplace in
host/align_plan.h read each switch on its own), so every device path must have done its work: the counters the
per-option stage tests read say so."""
import numpy as np
import pytest

from sina_amd import pipeline, synth
from tests import bps_ref as br, long_cases as lc, rank_cases as rc, shift_cases as sc, shift_ref as sr, util
from tests.test_gpu_long import _run as _long_run

pytestmark = pytest.mark.gpu

# the options that decide WHAT is computed: the same in both runs
FF = {"fs-min-len": 50, "fs-full-len": 150, "fs-leave-query-out": 1, "fs-msc-max": 0.9}     # (msc_cases.LEAVEOUT_FF's two, this world's lengths)
ORACLE_FF = dict(fs_min_len=50, fs_full_len=150, fs_leave_query_out=1, fs_msc_max=0.9)
AL = {"realign": True, "calc-idty": 1, "lowercase": "unaligned"}
ORACLE_AL = dict(realign=1, lowercase=2)
SEARCH = {"lca-fields": "tax_slv", "search-max-result": 7}
# ... and the options that decide WHERE
FF_DEVICE = ("device-msc", "device-cascade")
AL_DEVICE = ("device-bps", "device-idty", "device-shift", "device-search")
COUNTERS = ("pair_inplace_stats", "identity_inplace_stats", "search_inplace_stats", "assemble_stats", "family_stats",
            "match_stats", "rank_stats", "pair_stats", "slow_path_queries")


def options(on):
    """(famfinder, aligner, search) with every device option on or off; wide-fallback belongs to the all-on run alone."""
    ff = dict(FF, **{k: int(on) for k in FF_DEVICE})
    al = dict(AL, **{k: int(on) for k in AL_DEVICE})
    if on:
        al["wide-fallback"] = True
    return ff, al, dict(SEARCH, **{"device-rank": bool(on)})


def mirror_map(width):
    """tests/test_gpu_shift.py's map: column i pairs with its mirror image."""
    helix = np.zeros(width, np.uint32)
    cols = np.arange(5, width // 2 - 5)
    helix[cols] = width - 1 - cols
    helix[width - 1 - cols] = cols
    return helix


def near_map(width, d=3):
    """Column c paired with column c + d, every 2 d columns: the long world has a base every third column."""
    helix = np.zeros(width, np.uint32)
    for c in range(d, width - 2 * d, 2 * d):
        helix[c], helix[c + d] = c + d, c
    return helix


@pytest.fixture(scope="module")
def world(oracle):
    refs, qs, caps = sc.stage_world()
    st = pipeline.Store(":mem:gpu-all-options", refs)
    for i in range(refs.n):                 # (the taxonomy of tests/test_gpu_rank_stage.py; no version: the family text keeps ".0")
        st.set_attr(i, "tax_slv", rc.stage_taxonomy(i))
    assert [st.name(i) for i in range(refs.n)] == rc._names(refs.n)
    st.set_pairs(mirror_map(refs.width))
    yield st, refs, qs, caps
    st.close()


def _counters(st):
    out = {}
    for name in COUNTERS:
        v = getattr(st, name)()
        out[name] = dict(zip(("wide", "long"), v)) if isinstance(v, tuple) else v
    return out


def _delta(a, b):
    return {n: {k: b[n][k] - a[n][k] for k in b[n]} for n in b}


def _tray(pl, q):
    """Every key result() returns, floats by their bits, and the search stage's attributes."""
    r = pl.result(q)
    d = dict(r)
    d["packed"] = r["packed"].tobytes()
    d["idty"], d["bps"] = int(util.f32_bits(r["idty"])), int(util.f32_bits(r["bps"]))
    searched = r["search_ids"] is not None
    d["search_ids"] = r["search_ids"].tolist() if searched else None
    d["search_scores"] = util.f32_bits(r["search_scores"]).tolist() if searched else None
    d["nearest_slv"] = pl.attr(q, "nearest_slv") if searched else None
    d["lca_tax_slv"] = pl.attr(q, "lca_tax_slv") if searched else None
    return d


def _pipeline_run(st, qs, on, batch, check=None):
    ff, al, search = options(on)
    before = _counters(st)
    pl = pipeline.Pipeline(st, famfinder=ff, aligner=al, search=search)
    try:
        pl.run(qs.mask, qs.off, batch=batch, inflight=2)
        trays = [_tray(pl, q) for q in range(qs.n)]
        if check is not None:
            check(pl)
    finally:
        pl.close()
    return trays, _delta(before, _counters(st))


def _same_trays(off, on, tag):
    assert len(off) == len(on)
    for q, (a, b) in enumerate(zip(off, on)):
        assert sorted(a) == sorted(b), (tag, q)
        for k in a:
            assert a[k] == b[k], (tag, "query %d" % q, k, a[k], b[k])


def _device_paths_worked(d, qs, caps, events, tag):
    """With everything on: what each option's own stage test reads of its counters."""
    n_host = len(caps)
    shifted = sum(0 < e <= sr.SHIFT_LOG for e in events)
    print(tag, {k: v for k, v in d.items()})
    assert d["pair_inplace_stats"]["trays"] == qs.n - n_host and d["pair_inplace_stats"]["sequences"] > 0, tag
    assert d["identity_inplace_stats"]["trays"] == qs.n - n_host and d["identity_inplace_stats"]["sequences"] > 0, tag
    assert d["search_inplace_stats"]["trays"] == qs.n - n_host and d["search_inplace_stats"]["sequences"] > 0, tag
    assert d["search_inplace_stats"]["launches"] >= 1 and d["search_inplace_stats"]["pairs"] >= d["search_inplace_stats"]["sequences"], tag
    # the trays the row ranked made no call of sina_hip_kmer_topk_rank: device-rank saw the host-finished ones alone
    assert d["rank_stats"]["ranked"] + d["rank_stats"]["fallen_back"] == n_host, tag
    assert d["assemble_stats"]["shifted_queries"] == shifted > 0, tag
    assert d["assemble_stats"]["shifted_runs"] == sum(e for e in events if e <= sr.SHIFT_LOG), tag
    assert d["assemble_stats"]["trays_host"] == n_host and d["assemble_stats"]["trays_device"] == qs.n - n_host, tag
    assert d["family_stats"]["queries"] >= qs.n and d["family_stats"]["launches"] > 0, tag         # family-cascade rows
    assert d["match_stats"]["launches"] > 0 and d["match_stats"]["pairs"] > 0, tag
    assert d["slow_path_queries"]["wide"] == 0, tag                                                  # (nothing here needs the wide path)


def _device_paths_idle(d, tag):
    for name in ("pair_inplace_stats", "identity_inplace_stats", "search_inplace_stats", "family_stats", "match_stats"):
        assert all(v == 0 for v in d[name].values()), (tag, name, d[name])
    assert d["rank_stats"]["ranked"] == 0 and d["rank_stats"]["launches"] == 0, tag
    assert d["assemble_stats"]["shifted_queries"] == 0, tag


def _events(trays, caps):
    """Shifted runs per query, from the all-off run's logs (there the host's container code writes them)."""
    events = [len(sc.log_events(t["log"])) for t in trays]
    assert [q for q, e in enumerate(events) if e > sr.SHIFT_LOG] == list(caps)
    return events


@pytest.mark.parametrize("batch", ("all", 5))
def test_pipeline_trays_are_the_same_with_everything_on(oracle, world, batch):
    """Identical trays -- sequence and case bits, head, tail, quality, family, align_bp_score_slv, align_ident_slv, the
    search results, nearest_slv, lca_tax_slv, the whole log -- in one batch and in batches of five; the all-off run's
    are the oracle's (util.check_trays; the oracle's famfinder applies no identity limit below 1 and needs none here:
    the queries arrive unaligned, base i in column i, and no reference comes near 0.9 of that); with everything on
    every device path did its work, the two queries beyond the shift log's cap are the host's."""
    st, refs, qs, caps = world
    n = qs.n if batch == "all" else batch
    cs = util.cseqs_from_refs(refs)
    idx = oracle.Index(cs, k=10)
    n_dp = []
    off, d_off = _pipeline_run(st, qs, False, n, check=lambda pl: n_dp.append(util.check_trays(oracle, qs, pl, cs, idx, ORACLE_FF, ORACLE_AL)))
    assert n_dp == [qs.n]
    on, d_on = _pipeline_run(st, qs, True, n)
    _same_trays(off, on, ("batch", batch))
    print("status", [t["status"] for t in on], "search results", [None if t["search_ids"] is None else len(t["search_ids"]) for t in on],
          "bp_score", [t["bp_score"] for t in on])
    assert all(t["status"] == 0 and t["search_ids"] is not None for t in on)
    assert sum(len(t["search_ids"]) > 0 for t in on) >= qs.n - len(caps)
    assert sum(t["bp_score"] != 0 for t in on) >= qs.n - len(caps) and all(t["idty"] != int(util.f32_bits(-1.0)) for t in on)
    _device_paths_idle(d_off, ("off", batch))
    _device_paths_worked(d_on, qs, caps, _events(off, caps), ("on", batch))


def test_run_fasta_writes_the_same_file(world, tmp_path):
    st, refs, qs, caps = world
    events = _events(_pipeline_run(st, qs, False, qs.n)[0], caps)
    src = str(tmp_path / "in.fasta")
    with open(src, "w") as f:
        for q in range(qs.n):
            f.write(">q%d\n%s\n" % (q, synth.bases_string(qs.seq(q))))
    runs = {}
    for on in (False, True):
        ff, al, search = options(on)
        dst = str(tmp_path / ("out%d.fasta" % on))
        before = _counters(st)
        got = pipeline.run_fasta(st, src, dst, famfinder=ff, aligner=al, search=search, fasta={"meta-fmt": "comment"}, batch=8)
        lines = open(dst, "rb").read().split(b"\n")
        runs[on] = (got, [l for l in lines if not l.lstrip(b"; ").startswith(b"aligned_slv")],      # (the date)
                    _delta(before, _counters(st)))
    assert runs[False][0] == runs[True][0] and runs[False][1] == runs[True][1]
    text = runs[True][1]
    assert len(text) > 2 * qs.n and any(b"nearest_slv" in l for l in text) and any(b"align_bp_score_slv" in l for l in text)
    _device_paths_idle(runs[False][2], "run_fasta off")
    _device_paths_worked(runs[True][2], qs, caps, events, "run_fasta on")


def test_long_route_with_everything_on(oracle):
    """The pipeline world of tests/test_gpu_long.py (three queries above 10 240 bases among five windows, long-queries
    and wide-fallback) with every device option on, against that file's own expectations: every tray equals the
    oracle's, the long queries took the long count kernel and the wide DP kernel; their search results are the
    oracle's.  The world has unique names and a search stage, so device-search stays on: the long route's one-slot
    calls rank nothing (plan_search_inplace), the windows are ranked in place."""
    from oracle import pyoracle as po
    refs, _, idx = lc.pipe_world()
    qs = lc.pipe_queries()
    want = lc.pipe_expected(0)
    st = pipeline.Store(":mem:gpu-all-options-long", refs)
    try:
        helix = near_map(refs.width)
        st.set_pairs(helix)
        before = _counters(st)
        pl = _long_run(st, qs, want, ff={k: 1 for k in FF_DEVICE}, al=dict({k: 1 for k in AL_DEVICE}, **{"calc-idty": 1}),
                       search={"device-rank": True})
        try:
            so = oracle.search_opts()
            for qi in range(qs.n):
                aligned = po.Cseq.from_packed("query%d" % qi, want[qi]["packed"], want[qi]["width"])
                want_ids, want_sc, _ = oracle.search(idx, aligned, so)
                got = pl.result(qi)
                assert len(want_ids) > 0 and (got["search_ids"] == want_ids).all(), qi
                assert (util.f32_bits(got["search_scores"]) == util.f32_bits(want_sc)).all(), qi
                assert got["idty"] != -1, qi
                bp = br.attr(br.score(br.counts(want[qi]["packed"], helix)))
                assert got["bp_score"] == bp != 0, (qi, got["bp_score"], bp)
        finally:
            pl.close()
        d = _delta(before, _counters(st))
        print("long route", d)
        n_short = qs.n - len(lc.PIPE_LONG_AT)
        assert d["slow_path_queries"]["wide"] == len(lc.PIPE_LONG_AT)
        assert 0 < d["pair_inplace_stats"]["trays"] <= n_short and 0 < d["identity_inplace_stats"]["trays"] <= n_short
        assert 0 < d["search_inplace_stats"]["trays"] <= n_short
        # every tray the row did not rank went through the stage's own device ranking
        assert d["rank_stats"]["ranked"] + d["rank_stats"]["fallen_back"] == qs.n - d["search_inplace_stats"]["trays"]
        assert d["family_stats"]["queries"] >= qs.n
    finally:
        st.close()
