"""Queries of more than SINA_HIP_MAX_QUERY_LEN = 10 240 bases on the GPU: the long k-mer count kernel behind
sina_hip_kmer_topk_any / sina_hip_kmer_scores_any against the oracle on every case of tests/long_cases.py (what each
case is there for is asserted in tests/test_long_cpu.py), the routing per query, and the pipeline with famfinder's
`long-queries` and the aligner's `wide-fallback`."""
import numpy as np
import pytest

from sina_amd import capi, pipeline, synth
from tests import long_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx_of():
    """A context per reference world, its index built on the device."""
    made = {}

    def get(wname):
        if wname not in made:
            refs, k, nofast = lc.world(wname)
            ctx = capi.Context(0)
            ctx.upload_refs(refs.ab, refs.off, refs.width)
            ctx.build_index(k, nofast)
            made[wname] = ctx
        return made[wname]

    yield get
    for ctx in made.values():
        ctx.close()


def _check_case(ctx, c):
    exp = lc.expected(c.name)
    n_long = sum(c.is_long())
    for mx in c.maxes:
        before = ctx.long_queries()
        ids, sc, n = ctx.kmer_topk_any(c.qmask, c.qoff, mx)
        assert ctx.long_queries() - before == n_long
        for qi in range(len(c.qmasks)):
            oi, os_ = exp[qi]["find"][mx]
            assert n[qi] == len(oi), (c.name, mx, qi)
            assert (ids[qi, :n[qi]] == oi).all(), (c.name, mx, qi)
            assert (sc[qi, :n[qi]] == os_).all(), (c.name, mx, qi)
    before = ctx.long_queries()
    for qi, m in enumerate(c.qmasks):
        assert (ctx.kmer_scores_any(m) == exp[qi]["scores"]).all(), (c.name, qi)
    assert ctx.long_queries() - before == n_long


@pytest.mark.parametrize("name", ["lengths", "seam-n", "multiplicity", "degenerate", "mixed"])
def test_cases_equal_oracle(oracle, ctx_of, name):
    c = lc.case(name)
    _check_case(ctx_of(c.world), c)


@pytest.mark.parametrize("wname", lc.TILE_WORLDS)
def test_three_tiles_and_dense_lists_equal_oracle(oracle, ctx_of, wname):
    """70 000 references: three tiles per chunk, more dense k-mers per chunk than the bit-sliced path takes (the rest go
    by cursor), with k = 8 and k = 10, fast and no-fast."""
    ctx = ctx_of(wname)
    _check_case(ctx, lc.tiles(wname))
    assert ctx.stats()["n_dense_lists"] > 0


def test_fullest_score_and_the_limit(oracle, ctx_of):
    """A 32767-base query whose every k-mer one reference holds: 32757, still positive as an int16.  One base more is
    refused as over a limit; the fast entries keep their own refusal of anything beyond 10 240 bases."""
    c = lc.fullest()
    ctx = ctx_of(c.world)
    _check_case(ctx, c)
    refs = lc.world(c.world)[0]
    ids, sc, n = ctx.kmer_topk_any(c.qmask, c.qoff, 1)
    assert (int(ids[0, 0]), float(sc[0, 0])) == (refs.n - 1, 32757.0)
    assert ctx.kmer_scores_any(c.qmasks[0])[refs.n - 1] == 32757
    before = ctx.long_queries()
    too = lc.too_long()
    off = np.array([0, len(too)], np.uint64)
    with pytest.raises(capi.SinaHipError, match="SINA_HIP_MAX_LONG_QUERY_LEN"):
        ctx.kmer_topk_any(too, off, 1)
    assert ctx.last_error_is_limit()
    with pytest.raises(capi.SinaHipError, match="SINA_HIP_MAX_LONG_QUERY_LEN"):
        ctx.kmer_scores_any(too)
    assert ctx.last_error_is_limit()
    # ... also in a batch whose other queries are fine: nothing is truncated, nothing is run
    both = np.concatenate([c.qmasks[0][:300], too])
    with pytest.raises(capi.SinaHipError, match="SINA_HIP_MAX_LONG_QUERY_LEN"):
        ctx.kmer_topk_any(both, np.array([0, 300, len(both)], np.uint64), 1)
    with pytest.raises(capi.SinaHipError, match="SINA_HIP_MAX_QUERY_LEN"):
        ctx.kmer_topk(c.qmask, c.qoff, 1)
    assert not ctx.last_error_is_limit()
    with pytest.raises(capi.SinaHipError, match="SINA_HIP_MAX_QUERY_LEN"):
        ctx.kmer_scores(c.qmasks[0])
    assert ctx.long_queries() == before


def test_routing_is_per_query(oracle, ctx_of):
    """The queries the fast kernel takes -- the short ones of the mixed batch, the 10240-base one -- give the bytes of
    sina_hip_kmer_topk on the same input and leave sina_hip_long_queries alone; the others raise it by their number."""
    c = lc.mixed()
    ctx = ctx_of(c.world)
    long_ = np.array(c.is_long())
    short = lc.Case("short", c.world, [m for m, lg in zip(c.qmasks, long_) if not lg])
    assert lc.FAST_MAX in [len(m) for m in short.qmasks]
    for mx in c.maxes:
        before = ctx.long_queries()
        want = ctx.kmer_topk(short.qmask, short.qoff, mx)
        alone = ctx.kmer_topk_any(short.qmask, short.qoff, mx)
        assert ctx.long_queries() == before
        got = ctx.kmer_topk_any(c.qmask, c.qoff, mx)
        assert ctx.long_queries() - before == int(long_.sum())
        for w, a, g in zip(want, alone, got):
            assert w.tobytes() == a.tobytes() == g[~long_].tobytes(), mx
    before = ctx.long_queries()
    m = short.qmasks[[len(x) for x in short.qmasks].index(lc.FAST_MAX)]
    assert ctx.kmer_scores_any(m).tobytes() == ctx.kmer_scores(m).tobytes()
    assert ctx.long_queries() == before


# ---------------------------------------------------------------- the pipeline

@pytest.fixture(scope="module")
def pipe_store(oracle):
    refs = lc.pipe_world()[0]
    st = pipeline.Store(":mem:gpu-long-queries", refs)
    yield st
    st.close()


def _check_trays(pl, qs, want):
    n_dp = 0
    for qi in range(qs.n):
        got, w = pl.result(qi), want[qi]
        if w["status"] == 2:
            assert got["status"] == 2 and got["log"] == w["log"]
            continue
        assert got["family"] == "".join("ref%d.0:%.2f " % (i, s) for i, s in zip(w["ids"], w["sc"])), qi
        assert got["status"] == w["status"], (qi, got["log"], w["log"])
        assert (got["packed"] == w["packed"]).all(), qi              # columns AND case bits
        assert (got["head"], got["tail"], got["qual"]) == (w["head"], w["tail"], w["qual"]), qi
        assert got["log"] == w["log"], qi                             # NAST + scoring text
        n_dp += w["status"] == 0
    return n_dp


def _run(st, qs, want, ff=None, al=None, search=None):
    """One pipeline run with long-queries + wide-fallback; gives the pipeline (open) after the checks every run shares:
    every tray equals the oracle's, the long ones went through the long count kernel, and exactly they through the wide
    DP kernel."""
    wide0, long0 = st.slow_path_queries()
    pl = pipeline.Pipeline(st, famfinder=dict(lc.PIPE_FF, **{"long-queries": True}, **(ff or {})),
                           aligner=dict({"wide-fallback": True}, **(al or {})), search=search)
    pl.run(qs.mask, qs.off, batch=qs.n, inflight=1)
    assert _check_trays(pl, qs, want) == qs.n
    wide1, long1 = st.slow_path_queries()
    assert wide1 - wide0 == len(lc.PIPE_LONG_AT)         # the ordinary queries kept the fast DP path
    assert long1 - long0 >= len(lc.PIPE_LONG_AT)
    return pl


def test_pipeline_aligns_long_queries_among_ordinary_ones(oracle, pipe_store):
    qs = lc.pipe_queries()
    _run(pipe_store, qs, lc.pipe_expected(0)).close()


def test_pipeline_long_queries_insertion_forbid(oracle, pipe_store):
    qs = lc.pipe_queries()
    _run(pipe_store, qs, lc.pipe_expected(1), al={"insertion": "forbid"}).close()


def test_pipeline_long_query_turned_back(oracle, pipe_store):
    """--turn all: a long query handed in reversed and complemented is recognised by the four top-1 searches (each of
    them through the long kernel), turned back and aligned as the oracle aligns the original."""
    qs = lc.pipe_queries()
    at = lc.PIPE_LONG_AT[1]
    masks = [qs.seq(i) for i in range(qs.n)]
    masks[at] = lc.COMPLEMENT[masks[at][::-1]]
    turned = synth.QuerySet(mask=np.concatenate(masks), off=qs.off, src=qs.src)
    pl = _run(pipe_store, turned, lc.pipe_expected(0), ff={"turn": "all"})
    for qi in range(qs.n):
        assert pl.attr(qi, "turn") == ("reversed and complemented" if qi == at else "none")
    pl.close()


def test_pipeline_long_queries_through_the_search_stage(oracle, pipe_store):
    """The search stage's own k-mer search takes the ALIGNED long query through kmer_search as well."""
    from oracle import pyoracle as po
    qs = lc.pipe_queries()
    want = lc.pipe_expected(0)
    idx = lc.pipe_world()[2]
    pl = _run(pipe_store, qs, want, search={})
    so = oracle.search_opts()
    for qi in lc.PIPE_LONG_AT:
        aligned = po.Cseq.from_packed("query%d" % qi, want[qi]["packed"], want[qi]["width"])
        want_ids, want_sc, _ = oracle.search(idx, aligned, so)
        got = pl.result(qi)
        assert len(want_ids) > 0 and (got["search_ids"] == want_ids).all(), qi
        assert (got["search_scores"].view(np.uint32) == np.asarray(want_sc, np.float32).view(np.uint32)).all(), qi
    pl.close()


def test_long_queries_without_wide_fallback_fail_in_the_aligner_alone(oracle, pipe_store):
    """long-queries on, wide-fallback off: the long trays are searched, then get the aligner's soft failure; the rest
    is aligned."""
    qs = lc.pipe_queries()
    want = lc.pipe_expected(0)
    wide0, _ = pipe_store.slow_path_queries()
    pl = pipeline.Pipeline(pipe_store, famfinder=dict(lc.PIPE_FF, **{"long-queries": True}))
    pl.run(qs.mask, qs.off, batch=qs.n, inflight=1)
    for qi in range(qs.n):
        got = pl.result(qi)
        if qi in lc.PIPE_LONG_AT:
            n = len(qs.seq(qi))
            assert got["status"] == 2 and len(got["packed"]) == 0
            assert got["family"] == "".join("ref%d.0:%.2f " % (i, s) for i, s in zip(want[qi]["ids"], want[qi]["sc"]))
            assert "unable to align: sequence of %d bases (device limit 10240);" % n in got["log"]
        else:
            assert got["status"] == want[qi]["status"] == 0 and (got["packed"] == want[qi]["packed"]).all()
            assert got["log"] == want[qi]["log"]
    assert pipe_store.slow_path_queries()[0] == wide0
    pl.close()
    # ... and with neither option the famfinder's own soft failure, as ever
    pl = pipeline.Pipeline(pipe_store, famfinder=lc.PIPE_FF)
    pl.run(qs.mask, qs.off, batch=qs.n, inflight=1)
    for qi in lc.PIPE_LONG_AT:
        got = pl.result(qi)
        assert got["status"] == 2 and "unable to align: sequence longer than 10240 bases;" in got["log"]
    pl.close()
