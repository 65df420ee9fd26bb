"""A positional weight vector per query in one launch (sina_hip_align_graphs_wsets / sina_hip_align_families_wsets) and
famfinder's --auto-filter-field through the pipeline, on the device: the inputs of tests/autofilter_cases.py, which
tests/test_autofilter_cpu.py pins on the CPU.

  1. align_graphs_wsets equals the plain walk of every query under ITS vector, compared as tests/test_gpu_walk.py
     compares (every field, raw and sum_weight by their bits, out_pos entry for entry; bt_lanes 0 / 1 x assemble 0 / 1).
  2. align_families_wsets equals sina_hip_align_families called once per set with that set's queries, byte for byte, and
     the plain walk for every query; one DP launch.
  3. n_sets == 1 and weight_set == NULL are the plain entries; a set id out of range and a profile batch are refused
     before anything runs.
  4. The pipeline with auto-filter-field equals the oracle's famfinder + the restated vote + align(weights = chosen),
     in one DP launch per scheme; weight-sets off gives the same trays in one launch per filter.
"""
import numpy as np
import pytest

from sina_amd import capi, pipeline
from tests import autofilter_cases as ac, test_gpu_walk as tw, util, walk_cases as wc

pytestmark = pytest.mark.gpu


def _pack(qms):
    qoff = np.zeros(len(qms) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(m) for m in qms])
    return np.concatenate(qms), qoff


def _split(out, pos, qoff):
    return out.copy(), [pos[int(qoff[q]):int(qoff[q]) + int(out[q]["n_out"])].copy() for q in range(len(out))]


# ---------------------------------------------------------------- 1. graphs

@pytest.mark.parametrize("geom", ac.GEOMS, ids=["geom-own", "geom-128x8"])
@pytest.mark.parametrize("insertion", (0, 1), ids=["shift", "forbid"])
def test_align_graphs_wsets_against_the_plain_walk(oracle, monkeypatch, insertion, geom):
    case, ref = ac.graphs_reference(insertion)
    _, qms, sets = ac.graph_queries()
    W = ac.weight_vectors()
    util.set_knobs(monkeypatch, geom=geom, rho=None, lds_kb=None)
    ctx = capi.Context(0)
    try:
        gb = ctx.graph_batch([r["graph"] for r in ref], case.width)
        qmask, qoff = _pack(qms)
        popts = {k: v for k, v in case.opts.items() if k not in ("fs_no_graph", "weights")}
        got = {}
        for lanes in (0, 1):
            util.set_knobs(monkeypatch, bt_lanes=lanes)
            for asm in (0, 1):
                out, pos = ctx.align_graphs_wsets(gb, qmask, qoff, ctx.params_wsets(W, assemble=asm, **popts), sets, len(W))
                got[lanes, asm] = _split(out, pos, qoff)
    finally:
        ctx.close()
    tw._check(case, ref, got)


# ---------------------------------------------------------------- 2. families

@pytest.fixture(scope="module")
def small_ctx(oracle):
    refs = wc.world_small()[0]
    ctx = capi.Context(0)
    ctx.upload_refs(refs.ab, refs.off, refs.width)
    yield ctx
    ctx.close()


def _fam_pack(ids):
    foff = np.zeros(len(ids) + 1, np.uint64)
    foff[1:] = np.cumsum([len(f) for f in ids])
    return np.concatenate(ids), foff


def test_align_families_wsets_against_one_call_per_set(oracle, small_ctx):
    ctx = small_ctx
    ids, qms, sets = ac.family_queries()
    case, ref = ac.families_reference()
    W = ac.weight_vectors()
    fam, foff = _fam_pack(ids)
    qmask, qoff = _pack(qms)
    before = ctx.stats()["dp_launches"]
    out, pos = ctx.align_families_wsets(fam, foff, qmask, qoff, ctx.params_wsets(W), sets, len(W))
    assert ctx.stats()["dp_launches"] == before + 1
    got, got_pos = _split(out, pos, qoff)
    # the plain walk of every query under its own vector
    for q, r in enumerate(ref):
        wk, o, tag = r["walk"], got[q], ("query %d" % q, "set %d" % sets[q])
        assert o["status"] == 0, tag
        for f in tw._WALK_FIELDS:
            assert int(o[f]) == int(wk[f]), tag + (f, int(o[f]), int(wk[f]))
        assert util.f32_bits(o["raw"]) == util.f32_bits(wk["raw"]), tag + ("raw", o["raw"], wk["raw"])
        assert util.f32_bits(o["sum_weight"]) == util.f32_bits(wk["sum_weight"]), tag + ("sum_weight",)
        assert (got_pos[q].astype(np.int64) == wk["cols"]).all(), tag
    # ... and sina_hip_align_families, once per set
    for s in range(len(W)):
        mine = [q for q in range(len(qms)) if sets[q] == s]
        f1, fo1 = _fam_pack([ids[q] for q in mine])
        m1, qo1 = _pack([qms[q] for q in mine])
        o1, p1 = ctx.align_families(f1, fo1, m1, qo1, ctx.params(weights=W[s]))
        one, one_pos = _split(o1, p1, qo1)
        for x, q in enumerate(mine):
            assert one[x].tobytes() == got[q].tobytes(), (s, q)
            assert (one_pos[x] == got_pos[q]).all(), (s, q)
    # the same bases against the same family under two sets: two results, as the oracle's are
    assert got[0].tobytes() != got[1].tobytes() and ref[0]["walk"]["raw"] != ref[1]["walk"]["raw"]


# ---------------------------------------------------------------- 3. degenerate and refused

def test_one_set_and_no_set_ids_are_the_plain_entries(oracle, small_ctx):
    ctx = small_ctx
    ids, qms, sets = ac.family_queries()
    W = ac.weight_vectors()
    fam, foff = _fam_pack(ids)
    qmask, qoff = _pack(qms)
    plain = ctx.align_families(fam, foff, qmask, qoff, ctx.params(weights=W[0]))
    zeros = np.zeros(len(qms), np.uint32)
    for ws, n_sets, p in ((zeros, 1, ctx.params_wsets(W[:1])), (None, 1, ctx.params_wsets(W[:1])),
                          (None, 3, ctx.params_wsets(W))):
        out, pos = ctx.align_families_wsets(fam, foff, qmask, qoff, p, ws, n_sets)
        assert out.tobytes() == plain[0].tobytes() and (pos == plain[1]).all(), n_sets
    case, ref = ac.graphs_reference(0)
    _, gq, _ = ac.graph_queries()
    gb = ctx.graph_batch([r["graph"] for r in ref], case.width)
    qmask, qoff = _pack(gq)
    plain = ctx.align_graphs(gb, qmask, qoff, ctx.params(weights=W[0]))
    for ws, n_sets, p in ((np.zeros(len(gq), np.uint32), 1, ctx.params_wsets(W[:1])), (None, 3, ctx.params_wsets(W))):
        out, pos = ctx.align_graphs_wsets(gb, qmask, qoff, p, ws, n_sets)
        assert out.tobytes() == plain[0].tobytes() and (pos == plain[1]).all(), n_sets


def test_bad_set_ids_and_profile_batches_are_refused(oracle, small_ctx):
    ctx = small_ctx
    ids, qms, sets = ac.family_queries()
    W = ac.weight_vectors()
    fam, foff = _fam_pack(ids)
    qmask, qoff = _pack(qms)
    before = ctx.stats()
    bad = list(sets)
    bad[5] = 3
    with pytest.raises(capi.SinaHipError, match=r"weight set 3 of query 5 .*n_sets = 3"):
        ctx.align_families_wsets(fam, foff, qmask, qoff, ctx.params_wsets(W), bad, 3)
    assert not ctx.last_error_is_limit()
    case, ref = ac.graphs_reference(0)
    _, gq, gsets = ac.graph_queries()
    gb = ctx.graph_batch([r["graph"] for r in ref], case.width)
    gmask, goff = _pack(gq)
    bad = list(gsets)
    bad[-1] = 3
    with pytest.raises(capi.SinaHipError, match=r"weight set 3 of query 13 .*n_sets = 3"):
        ctx.align_graphs_wsets(gb, gmask, goff, ctx.params_wsets(W), bad, 3)
    assert not ctx.last_error_is_limit()
    # sets without weights, no sets at all
    with pytest.raises(capi.SinaHipError, match="need positional weights"):
        ctx.align_families_wsets(fam, foff, qmask, qoff, ctx.params(), sets, 3)
    with pytest.raises(capi.SinaHipError, match="n_sets must be at least 1"):
        ctx.align_families_wsets(fam, foff, qmask, qoff, ctx.params_wsets(W), sets, 0)
    # a profile batch takes no positional weights, so no sets
    fams = [ac.graph_queries()[0][0]]
    g, tab, self16 = wc.profile_tables(fams[0], wc.Case("p", case.width, fams, [gq[0]]).opts)
    pb = ctx.graph_batch([g], case.width, node_score16=tab, self_score16=self16)
    m1, o1 = _pack([gq[0]])
    with pytest.raises(capi.SinaHipError, match="profile batch takes no positional weights"):
        ctx.align_graphs_wsets(pb, m1, o1, ctx.params_wsets(W), [2], 3)
    assert not ctx.last_error_is_limit()
    after = ctx.stats()
    assert (after["dp_launches"], after["graph_launches"]) == (before["dp_launches"], before["graph_launches"])


# ---------------------------------------------------------------- 4. the pipeline

@pytest.fixture(scope="module")
def pipe_store(oracle):
    refs, qs, cs, idx, tax, filters = ac.world_pipeline()
    st = pipeline.Store(":mem:gpu-autofilter", refs)
    for i, t in tax.items():
        st.set_attr(i, ac.TAX_FIELD, t)
    for name, w in filters:
        st.add_filter(name, w)
    yield st
    st.close()


def _run(st, prefix, weight_sets):
    """One batch, one in flight: (results, attr align_filter_slv, DP launches the run made)."""
    qs = ac.world_pipeline()[1]
    ff = dict(ac.PIPE_FF_HOST)
    if prefix:
        ff["filter"] = prefix
    pl = pipeline.Pipeline(st, famfinder=ff, aligner={"weight-sets": weight_sets})
    before = st.stats()["dp_launches"]
    pl.run(qs.mask, qs.off, batch=qs.n, inflight=1)
    launches = st.stats()["dp_launches"] - before
    got = [dict(pl.result(q), filter=pl.attr(q, "align_filter_slv")) for q in range(qs.n)]
    pl.close()
    return got, launches


def _check_trays(got, exp):
    for q, (g, w) in enumerate(zip(got, exp)):
        assert g["family"] == "".join("ref%d.0:%.2f " % (i, s) for i, s in zip(w["ids"], w["sc"])), q
        assert g["status"] == w["status"] == 0, (q, g["log"], w["log"])
        assert (g["packed"] == w["packed"]).all(), q                       # columns and case bits
        assert (g["head"], g["tail"], g["qual"]) == (w["head"], w["tail"], w["qual"]), q
        assert g["filter"] == w["filter"], q
        assert g["log"] == w["log"], q                                     # "autofilter: ...;" in its place


@pytest.mark.parametrize("prefix", ("pv", "", "other"), ids=["filter-pv", "no-filter", "filter-other"])
def test_pipeline_auto_filter(oracle, pipe_store, prefix):
    exp = ac.pipeline_expected(prefix)
    filters_used = set(w["filter"] for w in exp)
    schemes = int("" in filters_used) + int(len(filters_used - {""}) > 0)
    on, launches_on = _run(pipe_store, prefix, True)
    _check_trays(on, exp)
    assert launches_on == schemes                    # one launch per scheme present: weighted, simple
    off, launches_off = _run(pipe_store, prefix, False)
    _check_trays(off, exp)
    assert launches_off == len(filters_used)         # one per distinct filter (the simple scheme counts as one)
    for a, b in zip(on, off):
        assert a["log"] == b["log"] and a["packed"].tobytes() == b["packed"].tobytes()
        assert {k: a[k] for k in ("status", "head", "tail", "qual", "family", "filter")} == \
            {k: b[k] for k in ("status", "head", "tail", "qual", "family", "filter")}
