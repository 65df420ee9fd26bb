"""CPU side of the auto-filter tests: the options and symbols exist, the exported vote (autofilter_vote behind
sina_host_autofilter_vote) equals its ten-line restatement on directed inputs, and the inputs of
tests/test_gpu_autofilter.py (tests/autofilter_cases.py) reach the edges they are there for.  No GPU."""
import os
import re

import numpy as np

from sina_amd import capi, pipeline, synth
from tests import autofilter_cases as ac, walk_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sina_hip_align_graphs_wsets", "sina_hip_align_families_wsets")


def test_options_and_symbols():
    H = pipeline.load_host()
    H.sina_host_reset_options()
    assert H.sina_host_set_option(b"famfinder", b"auto-filter-field", b"tax_slv") == 0
    assert H.sina_host_set_option(b"famfinder", b"auto-filter-threshold", b"0.5") == 0
    assert H.sina_host_set_option(b"famfinder", b"auto-filter-threshold", b"much") != 0
    assert H.sina_host_set_option(b"aligner", b"weight-sets", b"0") == 0
    H.sina_host_reset_options()
    hdr = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", hdr)
    L = capi.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert s in capi.ABI_SYMBOLS and hasattr(L, s), s


def _store(key, fields, names):
    """A store of len(fields) tiny references, reference i with `fields[i]` in tax_slv (None: without the field)."""
    refs = synth.make_refs(len(fields), length=60, width=240, seed=3)
    st = pipeline.Store(key, refs)
    for i, f in enumerate(fields):
        if f is not None:
            st.set_attr(i, ac.TAX_FIELD, f)
    for n in names:
        st.add_filter(n, np.ones(refs.width, np.float32))
    return st


def _both(st, names, fields, ids, prefix, threshold):
    want = ac.vote(names, ["" if fields[i] is None else fields[i] for i in ids], prefix, threshold)
    got, name = st.autofilter_vote(ids, ac.TAX_FIELD, prefix, threshold)
    assert got == want and name == ("" if want < 0 else names[want]), (ids, prefix, threshold, got, want)
    return got


def test_vote_directed_inputs():
    names = ["pv:Bacteria", "pv:Archaea;Eury", "pv:Archaea", "pv:bacteria;Proteo"]
    fields = ["Bacteria;Proteo", "bacteria;Firmi", "BACTERIA", "Archaea;Eury", "Archaea;Eury;x", "Archaea;Cren", None, "",
              "Bacteria;Proteo;y", "Eukaryota"]
    st = _store(":mem:autofilter-vote", fields, names)
    try:
        v = lambda ids, prefix="pv", thr=0.8: _both(st, names, fields, ids, prefix, thr)   # noqa: E731
        # a tie goes to the first registered filter: two bacteria, two euryarchaea
        assert v([0, 1, 3, 4], thr=0.4) == 0
        assert v([3, 4, 0, 1], thr=0.4) == 0
        # a prefix that differs only in case matches (field in another case, filter name in another case)
        assert v([1, 2]) == 0
        assert v([0, 8], prefix="PV") == 0
        # a general and a specific filter both match: the first registered stays, either way round
        assert v([3, 4]) == 1                       # "pv:Archaea;Eury" before "pv:Archaea"
        assert v([0, 8]) == 0                       # "pv:Bacteria" before "pv:bacteria;Proteo"
        assert v([3, 4, 5], thr=0.6) == 2           # only the general one counts the crenarchaeon: strictly more
        # 4 of 5 at 0.8 is no match (4 > 5 * 0.8f is false), 5 of 6 is one
        assert v([0, 1, 2, 8, 9]) == -1
        assert v([0, 1, 2, 8, 0, 9]) == 0
        assert v([0, 1, 2, 8, 9], thr=0.79) == 0
        # an empty family
        assert v([]) == -1
        assert v([], thr=0.0) == -1
        # relatives without the field, with an empty one: they count for nobody
        assert v([6, 7]) == -1
        assert v([0, 1, 2, 8, 6]) == -1 and v([0, 1, 2, 8, 0, 6]) == 0
        # an empty --filter prefix: the text is ":" + field, which no "pv..." filter heads
        assert v([0, 1, 2], prefix="") == -1
        # the threshold option's default is what a negative threshold stands for
        st.H.sina_host_reset_options()
        assert st.autofilter_vote([0, 1, 2, 8, 9], ac.TAX_FIELD, "pv")[0] == -1          # 0.8: 4 of 5 is not enough
        assert st.autofilter_vote([0, 1, 2, 8, 0, 9], ac.TAX_FIELD, "pv")[0] == 0        # ... 5 of 6 is
        assert st.H.sina_host_set_option(b"famfinder", b"auto-filter-threshold", b"0.79") == 0
        assert st.autofilter_vote([0, 1, 2, 8, 9], ac.TAX_FIELD, "pv")[0] == 0
        st.H.sina_host_reset_options()
    finally:
        st.close()


def test_vote_with_an_empty_prefix_can_match():
    """The reference's text is prefix + ":" + field even without --filter: a filter called ":Bacteria" heads it."""
    names = [":Bacteria"]
    fields = ["Bacteria;x", "bacteria"]
    st = _store(":mem:autofilter-empty-prefix", fields, names)
    try:
        assert _both(st, names, fields, [0, 1], "", 0.8) == 0
    finally:
        st.close()


def test_pipeline_world_chooses_several_filters(oracle):
    """Through the oracle alone: under --filter pv the queries choose at least two different filters and at least one
    finds no match; the general filter wins where only it counts every relative; some relatives lack the field;
    without --filter nothing matches, and under --filter other the default stays for every query."""
    refs, qs, cs, idx, tax, filters = ac.world_pipeline()
    assert (refs.n, refs.width, qs.n) == (400, 3000, 12)
    assert all(len(w) == refs.width for _, w in filters)
    exp = ac.pipeline_expected("pv")
    chosen = [r["chosen"] for r in exp]
    assert len(set(c for c in chosen if c >= 0)) >= 3 and chosen.count(-1) >= 1, chosen
    assert 2 in chosen                                         # "pv:Archaea": behind "pv:Archaea;Eury", yet strictly more
    assert all(r["status"] == 0 for r in exp)                  # every query goes through the DP
    assert any(r["filter"] == "" for r in exp) and any(r["filter"] != "" for r in exp)   # simple and weighted trays
    assert any(int(i) not in tax for r in exp for i in r["ids"])
    assert all(r["log"].startswith("autofilter: ") for r in exp)
    assert all(r["chosen"] == -1 and r["filter"] == "" for r in ac.pipeline_expected(""))
    assert all(r["chosen"] == -1 and r["filter"] == "other:all" for r in ac.pipeline_expected("other"))
    # the filter matters: a query's alignment score under its filter is not the one without
    plain = ac.pipeline_expected("")
    assert any(a["log"].split("autofilter")[1].split(";", 1)[1] != b["log"].split(";", 1)[1]
               for a, b in zip(exp, plain) if a["chosen"] >= 0)


def test_weight_set_cases_reach_their_edges(oracle):
    W = ac.weight_vectors()
    fams, qms, sets = ac.graph_queries()
    width = wc.world_small()[0].width
    assert W.shape == (3, width - 37) and len(qms) == 14
    assert sets[:6] == [0, 1, 2, 2, 1, 0] and set(sets) == {0, 1, 2}
    assert any((W[a] != W[b]).any() for a in range(3) for b in range(a))
    assert len(qms[12]) > 512                                  # a second strip of 512 columns
    for ins in (0, 1):
        case, ref = ac.graphs_reference(ins)
        # the clamp at the vector's end: nodes in columns beyond it, for every query
        assert all(int(r["graph"]["pos"].max()) > W.shape[1] - 1 for r in ref)
        assert all(r["orc"]["status"] == 0 for r in ref)
    # long insertions (shift): the gap-extension weight is read further and further right of the node's column
    _, ref = ac.graphs_reference(0)
    assert wc.nast_numbers(ref[12]["orc"]["log"])[1] >= 100 and wc.nast_numbers(ref[13]["orc"]["log"])[1] >= 20
    # the set matters: the same query under another vector scores differently
    other = ac._per_set_reference(fams, qms, [(s + 1) % 3 for s in sets], width)
    assert all(a["walk"]["raw"] != b["walk"]["raw"] for a, b in zip(ref, other))


def test_family_cases_reach_their_edges(oracle):
    ids, qms, sets = ac.family_queries()
    case, ref = ac.families_reference()
    work = [r["graph"]["n"] * len(m) for r, m in zip(ref, qms)]
    assert sorted(work, reverse=True) != work                  # the dispatch order is not the input order
    assert (ids[0] == ids[1]).all() and (qms[0] == qms[1]).all() and sets[0] != sets[1]
    assert all((ref[0]["graph"][k] == ref[1]["graph"][k]).all() for k in ("pos", "mask", "pred"))   # one DAG ...
    assert ref[0]["walk"]["raw"] != ref[1]["walk"]["raw"]      # ... two results
    assert len(set(len(m) for m in qms)) >= 4
