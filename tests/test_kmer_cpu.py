"""tests/kmer_ref.py -- the plain model tests/test_gpu_kmer.py holds the k-mer count and select kernels against --
pinned to the oracle on a natural world; the query helpers of tests/kmer_cases.py pinned to long_cases.windows; and
every named case and fuzz seed built, which runs check_csr and the builders' own assertions that the edge a case exists
for is reached.  No GPU."""
import os

import numpy as np
import pytest

from sina_amd import synth
from tests import kmer_cases as kc
from tests import kmer_ref, long_cases, util


@pytest.mark.parametrize("k,nofast", [(6, False), (6, True), (10, False), (10, True)])
def test_ref_equals_oracle(oracle, k, nofast):
    """Index.csr() into kmer_ref.scores / topk gives Index.scores / Index.find: queries with ambiguity codes, max = 1,
    41 and more than there are positive scores (the zeros with the largest ids fill the result)."""
    refs = synth.make_refs(300, length=200, width=1500, seed=8001, n_clades=5, amb_rate=0.02)
    other = synth.make_refs(40, length=200, width=1500, seed=8002, n_clades=2)
    idx = oracle.Index(util.cseqs_from_refs(refs), k=k, nofast=nofast)
    off, ids = idx.csr()
    seen_fill = False
    for qs in (synth.make_queries(refs, 5, seed=8003, amb_rate=0.03), synth.make_queries(other, 3, seed=8004, amb_rate=0.03)):
        for qi in range(qs.n):
            q = util.query_cseq(qs, qi)
            s = kmer_ref.scores(off, ids, refs.n, qs.seq(qi), k, not nofast)
            assert s.dtype == np.int64 and (s == idx.scores(q)).all()
            for mx in (1, 41, 300, 1000):
                gi, gs = kmer_ref.topk(s, mx)
                oi, os_ = idx.find(q, mx)
                assert gi.dtype == np.uint32 and gs.dtype == np.float32 and len(gi) == min(mx, refs.n)
                assert (gi == oi).all() and (gs == os_).all(), (qi, mx)
                seen_fill |= mx >= 300 and (s > 0).sum() < 300
    assert seen_fill


def _windows(mask, k, fast):
    w = long_cases.windows(mask, k, fast)
    return w[w >= 0]


@pytest.mark.parametrize("k", [6, 8])
def test_query_helpers(k):
    """query_of gives exactly its k-mers, in order, and no other window; poly the k-mer of one base len - k times (one
    more in front of an N); pad_n adds no window; kmer_ref.window_values agrees with long_cases.windows throughout."""
    rng = np.random.default_rng(8010 + k)
    kmers = [int(x) for x in rng.integers(0, 1 << (2 * k), size=40)] + [0, (1 << (2 * k)) - 1]
    q = kc.query_of(kmers, k)
    assert len(q) == len(kmers) * (k + 1) and _windows(q, k, False).tolist() == kmers
    assert _windows(q, k, True).tolist() == [v for v in kmers if v >> (2 * (k - 1)) == 0]
    for base in "AGCT":
        p = kc.poly(base, k + 30)
        assert _windows(p, k, False).tolist() == [kc.poly_kmer(base, k)] * 30
        assert _windows(np.append(p, kc.N_MASK), k, False).tolist() == [kc.poly_kmer(base, k)] * 31
        assert (kc.kmer_mask(kc.poly_kmer(base, k), k) == kc.BASE_MASK[base]).all()
    padded = kc.pad_n(q, len(q) + 77)
    assert len(padded) == len(q) + 77 and _windows(padded, k, False).tolist() == kmers
    assert len(kc.query_of([], k)) == 0 and len(_windows(np.full(3 * k, kc.N_MASK), k, False)) == 0
    mixed = rng.choice([1, 2, 4, 8, 15, 3, 1 | 16], size=400).astype(np.uint8)
    for m in (q, padded, mixed, mixed[:k], mixed[:k + 1], mixed[:0]):
        for fast in (False, True):
            assert kmer_ref.window_values(m, k, fast).tolist() == _windows(m, k, fast).tolist()


def test_index_for_scores_and_check_csr():
    """The construction gives the score row it was asked for; check_csr refuses what the kernels must never see."""
    rng = np.random.default_rng(8020)
    row = rng.integers(0, 6, size=500)
    kmers = [9, 100, 7, 4000, 50]
    lists = kc.index_for_scores(row, kmers)
    c = kc.Case("t", 500, 6, True, lists, [kc.query_of(kmers, 6)], (7,))
    assert (c.expected[0]["scores"] == row).all()
    for bad in ({1: np.array([3, 3], np.uint32)}, {1: np.array([4, 2], np.uint32)}, {1: np.array([500], np.uint32)}):
        with pytest.raises(AssertionError):
            kc.Case("bad", 500, 6, True, bad, [kc.query_of([1], 6)], (1,))
    ok = {1: np.array([7, 9], np.uint32), 2: np.array([0, 9], np.uint32)}       # (descending across a list boundary is fine)
    kc.Case("ok", 500, 6, True, ok, [kc.query_of([1, 2], 6)], (1,))


@pytest.mark.parametrize("name", sorted(kc.ALL_CASES))
def test_case_reaches_its_edge(name):
    """Building a case runs check_csr and the builder's assertions on the edge it exists for."""
    c = kc.case(name)
    assert c.name == name and len(c.expected) == len(c.qmasks) == len(c.labels)


def test_every_edge_has_its_case():
    """The branches the matrix is meant to hold, by the plain restatements of kmer_cases."""
    c = kc.dense_nd()
    nds = [kc.n_dense_windows(c, 2 * x, None) for x in range(len(kc.DENSE_ND))]
    assert nds == list(kc.DENSE_ND) and {kc.nhi_of(nd) for nd in nds} == set(range(8))
    assert [kc.nhi_of(n) for n in (1, 7, 8, 15, 16, 511, 512, 1023, 1024, 5000)] == [0, 0, 1, 1, 2, 6, 7, 7, 7, 7]
    assert all(kc.n_dense_windows(c, qi, "1") == 0 for qi in range(len(c.qmasks)))
    assert [kc.n_dense_windows(kc.dense_overflow(), qi, None) for qi in range(2)] == [1024, 1100]
    # the select kernel's short cut: every exit
    for qi in (0, 1):
        m = kc.shortcut_model(kc.sample_high().expected[qi]["scores"], 410, len(kc.sample_high().qmasks[qi]), 6)
        assert m["exit"] == "fewer" and m["usable"] and m["T0"] == 9 and m["n_ge_t0"] < 410
    exits = set()
    for name, qi, mx in (("sample_blind", 0, 410), ("sample_blind", 1, 410), ("giant_group", 0, 41),
                         ("take_all_boundary", 0, 410), ("take_all_boundary", 1, 410), ("zeros_fill_20000", 0, 410)):
        cs = kc.case(name)
        m = kc.shortcut_model(cs.expected[qi]["scores"], mx, len(cs.qmasks[qi]), cs.k)
        exits.add((m["exit"], m.get("take_all")))
    assert exits == {("unusable", None), ("found", True), ("found", False)}
    assert kc.shortcut_model(kc.case("row_tail_16376").expected[0]["scores"], 41, 63, 6) is None
    assert kc.shortcut_model(kc.case("row_tail_16377").expected[0]["scores"], 41, 63, 6) is not None
    assert kc.shortcut_model(kc.top_8192().expected[0]["scores"], 41, kc.FAST_MAX, 6) is None
    # the candidate list: 4096 fit, 4097 do not; launches 1 / 2
    for n_cand, launches in ((4096, 1), (4097, 2)):
        cs = kc.cap(n_cand)
        assert all(kc.cand_model(cs.expected[0]["scores"], mx)["n_cand"] == n_cand for mx in cs.maxes)
        assert all(kc.expected_launches(cs, mx, None) == launches and kc.expected_launches(cs, mx, 1) == 1 for mx in cs.maxes)
    assert kc.expected_launches(kc.winners_elsewhere(), 41, None) == 2
    assert {"tile_geometry_%d" % n for n in kc.EDGE_N_REFS} <= set(kc.COUNT_CASES)
    assert set(kc.CURSOR_PREFIXES) >= {0, 1, 63, 64, 65, 575, 576, 577, 1091}


@pytest.mark.parametrize("seed", range(int(os.environ.get("SINA_FUZZ_SEEDS", "12"))))
def test_fuzz_world_is_inside_the_contract(seed):
    c = kc.fuzz_world(seed)
    ln = c.list_lengths()
    thr = kc.dense_threshold(c.n_refs, c.dense_divs[0])
    assert len(set(c.maxes)) == 3 and 3 <= len(c.qmasks) <= 6 and c.k in (6, 8)
    assert (ln[ln > 0] <= thr).any() and ((ln > thr).any() or c.n_refs <= thr)
