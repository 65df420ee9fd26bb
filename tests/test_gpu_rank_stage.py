"""The search stage with `device-rank` (score and rank the candidates on the device) against the same stage without
it: result ids, score bits, nearest_slv, the LCA classification and the whole log text of every query are equal, on a
store of tests/test_gpu_search.py's kind; the store's counters say who ranked what.  tests/test_rank_cpu.py runs the
reference (the oracle) over the same worlds and asserts how many queries have a candidate without a score: those, and
only those, go back to the host path."""
import numpy as np
import pytest

from sina_amd import pipeline, synth
from tests import rank_cases as rc
from tests import util

pytestmark = pytest.mark.gpu


def _annotate(st, n):
    for i in range(n):
        st.set_attr(i, "version", str(1 + i % 3))
        st.set_attr(i, "start", str(i % 7))
        st.set_attr(i, "stop", str(1400 + i))
        st.set_attr(i, "tax_slv", rc.stage_taxonomy(i))


def _run(st, qs, sopts, device_rank, batch=10, inflight=2, dedup=True):
    search = dict({"lca-fields": "tax_slv"}, **sopts)
    if device_rank is not None:
        search["device-rank"] = device_rank
    before = st.rank_stats()
    pl = pipeline.Pipeline(st, famfinder=rc.STAGE_FF, aligner={"realign": True}, search=search, dedup=dedup)
    pl.run(qs.mask, qs.off, batch=batch, inflight=inflight)
    out = []
    for q in range(qs.n):
        r = pl.result(q)
        out.append(dict(ids=r["search_ids"], scores=r["search_scores"], log=r["log"],
                        nearest=pl.attr(q, "nearest_slv") if r["search_ids"] is not None else None,
                        lca=pl.attr(q, "lca_tax_slv") if r["search_ids"] is not None else None))
    pl.close()
    after = st.rank_stats()
    return out, {k: after[k] - before[k] for k in after}


def _same(off, on):
    assert len(off) == len(on)
    for q, (a, b) in enumerate(zip(off, on)):
        assert (a["ids"] is None) == (b["ids"] is None), q
        if a["ids"] is not None:
            assert a["ids"].tolist() == b["ids"].tolist(), q
            assert util.f32_bits(a["scores"]).tolist() == util.f32_bits(b["scores"]).tolist(), q
        assert a["nearest"] == b["nearest"] and a["lca"] == b["lca"], q
        assert a["log"] == b["log"], q


@pytest.mark.parametrize("name", rc.STAGE_NAMES)
def test_stage_device_rank_equals_host_path(name):
    sopts, oopts, kind, n_refs = rc.STAGE[name]
    refs = rc.stage_refs(n_refs)
    qs = rc.stage_queries(kind, n_refs)
    ref_run = rc.stage_reference_run(name)
    st = pipeline.Store(":mem:rank-stage-%s" % name, refs)
    try:
        _annotate(st, refs.n)
        off, d_off = _run(st, qs, sopts, None)
        assert d_off["ranked"] == 0 and d_off["fallen_back"] == 0 and d_off["launches"] == 0
        on, d_on = _run(st, qs, sopts, True)
        _same(off, on)
        searched = sum(1 for r in on if r["ids"] is not None)
        flagged = sum(1 for r in ref_run if r is not None and r["nan"])
        assert searched == sum(1 for r in ref_run if r is not None) and searched >= 10
        assert d_on["fallen_back"] == flagged and d_on["ranked"] == searched - flagged
        assert d_on["launches"] > 0 and d_on["pairs"] > 0 and d_on["kernel_ms"] > 0
        if not name.endswith("_fragments"):
            assert flagged == 0
            # ... and what both return is the reference's
            for q, r in enumerate(ref_run):
                if r is not None:
                    assert on[q]["ids"].tolist() == list(r["ids"]) and util.f32_bits(on[q]["scores"]).tolist() == util.f32_bits(r["scores"]).tolist()
        assert sum(len(r["ids"]) for r in on if r["ids"] is not None) > 0
    finally:
        st.close()


@pytest.mark.parametrize("name,sopts", [
    ("jc", {"search-correction": "jc", "search-cover": "target", "search-min-sim": 0.0}),
    ("ignore_super", {"search-ignore-super": True, "search-min-sim": 0.0}),
    ("max_result_65", {"search-max-result": 65, "search-min-sim": 0.0}),
])
def test_stage_keeps_the_host_path(name, sopts):
    """What the device does not rank as the host does stays on the host: nothing is ranked, every query counts as sent
    back, results are equal."""
    kind = "fragments" if name == "jc" else "full"       # (Jukes-Cantor of an identity above 0.75 is NaN)
    refs = rc.stage_refs(300)
    qs = rc.stage_queries(kind, 300)
    st = pipeline.Store(":mem:rank-stage-%s" % name, refs)
    try:
        _annotate(st, refs.n)
        off, _ = _run(st, qs, sopts, False)
        on, d = _run(st, qs, sopts, True)
        _same(off, on)
        searched = sum(1 for r in on if r["ids"] is not None)
        assert d["ranked"] == 0 and d["launches"] == 0 and d["fallen_back"] == searched >= 10
    finally:
        st.close()


def test_stage_repeated_name_keeps_the_host_path(tmp_path):
    """A FASTA store in which two references share a name: the order by name is no total order, the option changes
    nothing."""
    refs = rc.stage_refs(300)
    qs = rc.stage_queries("full", 300)
    db = str(tmp_path / "twice.fasta")
    with open(db, "w") as f:
        for i in range(refs.n):
            f.write(">%s\n%s\n" % ("ref%d" % (7 if i == 211 else i), synth.aligned_string(refs.seq(i), refs.width)))
    st = pipeline.Store.open(db)
    try:
        assert st.name(211) == st.name(7)
        _annotate(st, refs.n)
        off, _ = _run(st, qs, {"search-min-sim": 0.0}, False)
        on, d = _run(st, qs, {"search-min-sim": 0.0}, True)
        _same(off, on)
        assert d["ranked"] == 0 and d["launches"] == 0 and d["fallen_back"] == sum(1 for r in on if r["ids"] is not None) >= 10
    finally:
        st.close()


@pytest.mark.parametrize("kind", sorted(rc.REPEAT_STAGE))
def test_stage_repeated_queries_go_to_the_device_once(kind):
    """30 trays in one batch of which 12 are distinct (rc.stage_repeat_pick): device-rank off and on, each with the
    batch's repeats grouped and not, give the same trays -- for the whole queries the reference's, row for row through
    the pick.  With the repeats grouped the device compares what a run over the twelve alone compares, without them
    more; every searched tray counts as ranked or sent back, and a flag on a slot sends every tray that reads the slot
    back to the host."""
    name = rc.REPEAT_STAGE[kind]
    sopts = rc.STAGE[name][0]
    refs = rc.stage_refs(300)
    base = rc.stage_queries(kind, 300)
    distinct, pick = rc.stage_repeat_pick(kind)
    qs = synth.pick_queries(base, pick)
    ref_run = rc.stage_reference_run(name)
    assert qs.n == 30 and len(distinct) == 12
    st = pipeline.Store(":mem:rank-stage-repeats-%s" % kind, refs)
    try:
        _annotate(st, refs.n)
        runs = {(on, dedup): _run(st, qs, sopts, on, batch=30, inflight=1, dedup=dedup) for on in (False, True) for dedup in (True, False)}
        first = runs[False, True][0]
        for got, _ in runs.values():
            _same(first, got)
        searched = sum(1 for r in first if r["ids"] is not None)
        assert searched == sum(1 for q in pick if ref_run[q] is not None) >= 10
        if kind == "full":
            for t, q in enumerate(pick):
                r = ref_run[q]
                assert (first[t]["ids"] is None) == (r is None), t
                if r is not None:
                    assert first[t]["ids"].tolist() == list(r["ids"]), t
                    assert util.f32_bits(first[t]["scores"]).tolist() == util.f32_bits(r["scores"]).tolist(), t
        _, alone = _run(st, synth.pick_queries(base, distinct), sopts, True, batch=12, inflight=1, dedup=True)
        d_on, d_off = runs[True, True][1], runs[True, False][1]
        assert d_on["pairs"] == alone["pairs"] > 0 and d_off["pairs"] > alone["pairs"]
        flagged = sum(1 for q in pick if ref_run[q] is not None and ref_run[q]["nan"])
        assert (flagged > 0) == (kind == "fragments")
        for d in (d_on, d_off):
            assert d["ranked"] + d["fallen_back"] == searched and d["fallen_back"] == flagged
        for dedup in (True, False):
            d = runs[False, dedup][1]
            assert d["ranked"] == 0 and d["fallen_back"] == 0 and d["pairs"] == 0
    finally:
        st.close()
