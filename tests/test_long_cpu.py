"""CPU side of the long-query k-mer search: the cases of tests/long_cases.py pinned to the oracle (Index.find and its
score vector are what tests/test_gpu_long.py compares the device against), the property every case is there for, the
chunk arithmetic of the long count kernel as a plain model, and the additions to the C ABI, its Python view and the
stages' options."""
import os
import re

import numpy as np
import pytest

from sina_amd import capi, pipeline
from tests import long_cases as lc
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sina_hip_kmer_topk_any", "sina_hip_kmer_scores_any", "sina_hip_long_queries")


def _model_scores(case_name, qi):
    """Score vector of a query from the window model and the oracle's CSR index: every window adds one to every
    reference of its k-mer's posting list."""
    c = lc.case(case_name)
    refs, k, nofast = lc.world(c.world)
    off, ids = lc.oracle_csr(c.world)
    w = lc.chunk_windows(c.qmasks[qi], k, not nofast)
    sc = np.zeros(refs.n, np.int64)
    for v in w[w >= 0]:
        np.add.at(sc, ids[off[v]:off[v + 1]], 1)
    return sc


def test_limits_and_chunk_size():
    header = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    assert "#define SINA_HIP_MAX_QUERY_LEN %du" % capi.MAX_QUERY_LEN in header
    assert "#define SINA_HIP_MAX_LONG_QUERY_LEN %du" % capi.MAX_LONG_QUERY_LEN in header
    assert "#define SINA_HIP_KMER_LONG_CHUNK %du" % capi.KMER_LONG_CHUNK in header
    assert (capi.MAX_QUERY_LEN, capi.MAX_LONG_QUERY_LEN) == (10240, 32767)
    assert 12 <= lc.C <= capi.MAX_QUERY_LEN        # a chunk's windows fit the fast kernel's lists; k <= 12
    assert lc.SEAMS and all(s % lc.C == 0 and s < lc.LONG_MAX for s in lc.SEAMS) and lc.SEAMS[-1] + lc.C >= lc.LONG_MAX


def test_abi_additions():
    header = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert sym in capi.ABI_SYMBOLS
        assert hasattr(capi.load(), sym)
    assert "#define SINA_HIP_ABI_VERSION 5" in header
    for name in ("kmer_topk_any", "kmer_scores_any", "long_queries"):
        assert callable(getattr(capi.Context, name))


def test_stages_take_the_options():
    H = pipeline.load_host()
    try:
        assert H.sina_host_set_option(b"famfinder", b"long-queries", b"1") == 0
        assert H.sina_host_set_option(b"famfinder", b"long-queries", b"0") == 0
        assert H.sina_host_set_option(b"aligner", b"wide-fallback", b"1") == 0
    finally:
        H.sina_host_reset_options()


@pytest.mark.parametrize("k,fast", [(10, True), (10, False), (8, True), (3, False), (12, True)])
def test_chunked_windows_are_the_windows(k, fast):
    """What the long kernel does per chunk -- window ends e0 .. e1 - 1 over bases b0 .. e1 - 1 -- gives K(query): a
    window belongs to one chunk, only the one on the query's last base is dropped, an ambiguous base invalidates the
    windows over it on either side of a seam, the fast prefix rule is per window.  Small chunks: many seams."""
    rng = np.random.default_rng(100 * k + fast)
    for chunk in (k, 16, 37):
        for n in (1, k - 1, k, k + 1, chunk, chunk + 1, 3 * chunk - 1, 3 * chunk, 3 * chunk + 1, 5 * chunk + k):
            m = rng.choice([1, 2, 4, 8], size=n).astype(np.uint8)
            m[rng.random(n) < 0.04] = lc.N_MASK
            want = lc.windows(m, k, fast)
            got = lc.chunk_windows(m, k, fast, chunk=chunk)
            assert (want == got).all(), (k, fast, chunk, n)


def test_lengths_sit_on_the_seams(oracle):
    c = lc.lengths()
    ls = [len(m) for m in c.qmasks]
    assert ls == sorted(ls) and {capi.MAX_QUERY_LEN, capi.MAX_QUERY_LEN + 1} <= set(ls) and ls[-1] == capi.MAX_LONG_QUERY_LEN
    for s in lc.SEAMS:
        assert set(range(s - 11, s + 12)) <= set(ls)
    assert c.is_long().count(False) == 12            # the lengths up to the first seam stay on the fast kernel
    # windows that count -- fast prefix, a posting list -- end on either side of every seam, so a window dropped or
    # taken twice there changes a score
    refs, k, nofast = lc.world(c.world)
    off, _ = lc.oracle_csr(c.world)
    w = lc.windows(c.qmasks[-1], k, not nofast)
    for s in lc.SEAMS:
        for side in (w[s - 11:s], w[s:s + 11]):
            assert any(v >= 0 and off[v + 1] > off[v] for v in side), s
    # ... and the model over chunks gives the oracle's scores, at the shortest long length and the longest
    for qi in (ls.index(capi.MAX_QUERY_LEN + 1), len(ls) - 1):
        assert (_model_scores("lengths", qi) == lc.expected("lengths")[qi]["scores"]).all()
    # a base more adds a window, and that is seen in the scores (fast: of the one window in four that starts with A)
    sc = [e["scores"].astype(np.int64).sum() for e in lc.expected("lengths")]
    assert all(b >= a for a, b in zip(sc, sc[1:])) and len(set(sc)) > len(sc) // 8


def test_seam_n_invalidates_windows_on_both_sides(oracle):
    c = lc.seam_n()
    assert len(c.qmasks) == 2 * lc.K + 1 and all(len(m) > capi.MAX_QUERY_LEN for m in c.qmasks)
    for d, m in zip(range(-lc.K, lc.K + 1), c.qmasks):
        assert list(np.flatnonzero(m == lc.N_MASK)) == [lc.C + d]
        w = lc.windows(m, lc.K, False)
        bad = np.flatnonzero(w[lc.K - 1:-1] < 0) + lc.K - 1
        assert list(bad) == list(range(lc.C + d, lc.C + d + lc.K))    # the k windows over the N, whichever chunk they end in
    assert (_model_scores("seam-n", 3) == lc.expected("seam-n")[3]["scores"]).all()
    totals = {int(e["scores"].astype(np.int64).sum()) for e in lc.expected("seam-n")}
    assert len(totals) > 1


def test_multiplicity_counts_every_repeat(oracle):
    c = lc.multiplicity()
    refs = lc.world("main")[0]
    assert len(c.qmasks[0]) == lc.BLOCK_LEN * lc.BLOCK_REPEATS == 30000
    exp = lc.expected("multiplicity")[0]
    holder, tied = refs.n - lc.N_TIED - 1, list(range(refs.n - lc.N_TIED, refs.n))
    once = lc.oracle_index("main").scores(lc.as_cseq(lc.block()))
    # (the window on the block's last base is dropped when the block stands alone; inside the query only once, at the end)
    assert exp["scores"][holder] >= lc.BLOCK_REPEATS * once[holder] > 6 * 1000
    assert exp["scores"][holder] == exp["scores"].max()
    assert len({int(exp["scores"][t]) for t in tied}) == 1 and exp["scores"][tied[0]] == lc.BLOCK_REPEATS * once[tied[0]] > 0
    ids, _ = exp["find"][3]
    assert list(ids) == [holder, tied[-1], tied[-2]]            # ties: the largest ids first
    assert (_model_scores("multiplicity", 0) == exp["scores"]).all()


def test_fullest_score_is_32757(oracle):
    c = lc.fullest()
    refs, k, nofast = lc.world("full")
    assert nofast and len(c.qmasks[0]) == capi.MAX_LONG_QUERY_LEN == refs.off[-1] - refs.off[-2]
    exp = lc.expected("fullest")[0]
    assert exp["scores"][refs.n - 1] == capi.MAX_LONG_QUERY_LEN - k == 32757 > 0
    ids, sc = exp["find"][1]
    assert list(ids) == [refs.n - 1] and list(sc) == [32757.0]
    assert len(lc.too_long()) == capi.MAX_LONG_QUERY_LEN + 1


@pytest.mark.parametrize("wname", lc.TILE_WORLDS)
def test_tiles_case_holds_more_dense_kmers_than_a_chunk_takes(oracle, wname):
    c = lc.tiles(wname)
    refs, k, nofast = lc.world(wname)
    assert refs.n == 70000 > 2 * 32768 and len(c.qmasks[0]) > 2 * lc.C
    w = lc.windows(c.qmasks[0], k, not nofast)
    kmers, inv = np.unique(w[w >= 0], return_inverse=True)
    ln = lc.posting_lengths(refs, k, not nofast, kmers)[inv]   # per window: with multiplicity
    # (the plain count above against the oracle's index, on a world small enough to ask it)
    m_refs, m_k, m_nofast = lc.world("main")
    m_off, _ = lc.oracle_csr("main")
    some = np.unique(lc.windows(lc.lengths().qmasks[0], m_k, not m_nofast))[1:200]
    assert (lc.posting_lengths(m_refs, m_k, not m_nofast, some) == np.diff(m_off.astype(np.int64))[some]).all()
    dense = ln > max(256, refs.n // 64)                         # (kmer_dense_threshold, csrc/kmer_plan.h)
    assert int(dense.sum()) > 1023
    assert int((ln > 0).sum()) > int(dense.sum())               # cursor lists beside them


def test_degenerate_and_mixed(oracle):
    d = lc.degenerate()
    assert len(d.qmasks[0]) > capi.MAX_QUERY_LEN and (lc.windows(d.qmasks[0], lc.K, False) < 0).all()
    assert not lc.expected("degenerate")[0]["scores"].any()
    m = lc.mixed()
    long_ = m.is_long()
    assert long_.count(True) == 4 and long_.count(False) == 6 and any(a != b for a, b in zip(long_, long_[1:]))
    assert capi.MAX_QUERY_LEN in [len(x) for x in m.qmasks] and capi.MAX_LONG_QUERY_LEN in [len(x) for x in m.qmasks]
    assert m.maxes == (1, 41, 410, 4096) and lc.world("main")[0].n > 4096


def test_pipeline_families_fit_the_wide_budget(oracle):
    """The wide kernel takes (N + L - 1) * min(N, L) <= 2^29 cells per query: the families the oracle picks for the
    pipeline's long queries, as DAGs, stay within it."""
    refs, cs, idx = lc.pipe_world()
    qs = lc.pipe_queries()
    lens = [len(qs.seq(i)) for i in range(qs.n)]
    assert [i for i, n in enumerate(lens) if n > capi.MAX_QUERY_LEN] == list(lc.PIPE_LONG_AT)
    assert max(lens) <= capi.MAX_LONG_QUERY_LEN
    for qi in lc.PIPE_LONG_AT:
        ids, _, _ = idx.famfinder(util.query_cseq(qs, qi, upper=False), oracle.ff_opts(**lc.PIPE_OFF))
        assert len(ids) == lc.PIPE_OFF["fs_max"]
        n, L = util.graph_dict([cs[i] for i in ids])["n"], lens[qi]
        assert (n + L - 1) * min(n, L) <= 1 << 29, (qi, n, L)
