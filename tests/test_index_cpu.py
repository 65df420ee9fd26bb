"""tests/index_ref.py -- the plain index build tests/test_gpu_index.py holds sina_hip_build_index against -- pinned to
the oracle's Index.csr() on every named case and fuzz world of tests/index_cases.py, entry for entry, and kmer_ref's
scores over it to Index.scores for the cases' queries.  Building a case runs its own assertions that the store holds the
edge it is named for, and kmer_cases.check_csr on its plain indexes.  The one group kept out of the oracle comparison
is the cases that hold a word without any base bit: the oracle reads an arbitrary base from such a word (DESIGN section
4); they are compared on the GPU.  No GPU here."""
import os

import numpy as np
import pytest

from tests import index_cases as ic
from tests import index_ref, kmer_ref

SEEDS = range(int(os.environ.get("SINA_FUZZ_SEEDS", "12")))


def _cseqs(oracle, c):
    ab, off, width = c.packed()
    return [oracle.Cseq.from_packed("ref%d" % r, ab[int(off[r]):int(off[r + 1])], width) for r in range(c.n_refs)]


def _query_cseq(oracle, m):
    m = np.asarray(m, np.uint8) & 0x0f
    return oracle.Cseq.from_packed("q", np.arange(len(m), dtype=np.uint32) | (m.astype(np.uint32) << 24), max(len(m), 1))


def _pin(oracle, c):
    """The plain indexes of a case against the oracle's, and the scores of its queries."""
    cs = _cseqs(oracle, c)
    qs = [_query_cseq(oracle, m) for m in c.qmasks]
    for nofast in c.nofasts:
        idx = oracle.Index(cs, k=c.k, nofast=nofast)
        ooff, oids = idx.csr()
        off, ids = c.plain(nofast)
        assert off.dtype == np.uint32 and ids.dtype == np.uint32 and off[-1] == len(ids)
        assert index_ref.first_difference(off, ids, ooff, oids, c.k) is None, (c.name, nofast, index_ref.first_difference(off, ids, ooff, oids, c.k))
        for q, m, e in zip(qs, c.qmasks, c.expected(nofast)):
            assert (e["scores"] == idx.scores(q)).all(), (c.name, nofast, m.tolist())


def _properties(c):
    """What holds for the plain indexes of any store."""
    assert c.mask0 == c.holds_mask0(), c.name              # the flag is true to the data
    ic.quarter_lists_equal(c)
    for nofast in c.nofasts:
        off, ids = c.plain(nofast)
        per_ref = [set(index_ref.window_values(s, c.k, nofast).tolist()) for s in c.seqs]
        assert len(ids) == sum(len(x) for x in per_ref)
        for r, (s, vals) in enumerate(zip(c.seqs, per_ref)):
            assert vals == set(kmer_ref.window_values(s, c.k, not nofast).tolist())     # (a reference read as a query)
            assert all(r in ids[int(off[v]):int(off[v + 1])] for v in list(vals)[:40])


@pytest.mark.parametrize("name", list(ic.CASES))
def test_case_holds_its_edge_and_the_plain_build_equals_the_oracle(oracle, name):
    c = ic.case(name)                                      # (the builder's assertions and check_csr)
    _properties(c)
    assert c.mask0 == (name in ic.MASK0_CASES)
    if c.mask0:
        return                                             # compared with the device only (tests/test_gpu_index.py)
    _pin(oracle, c)


def test_mask0_is_outside_the_oracle():
    """The flagged cases are exactly those with a word without a base bit, and every other kind of edge is pinned."""
    flagged = [n for n in ic.CASES if ic.case(n).holds_mask0()]
    assert tuple(flagged) == ic.MASK0_CASES
    assert {ic.case(n).k for n in ic.CASES} == {1, 2, 4, 6, 8, 10, 12}


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_world_equals_the_oracle(oracle, seed):
    c = ic.fuzz_world(seed)
    _properties(c)
    assert 1 <= c.n_refs <= 400 and max(len(s) for s in c.seqs) <= 300 and c.k in (1, 2, 4, 6, 8)
    _pin(oracle, c)


def test_first_difference_names_the_list():
    off, ids = index_ref.build([ic.seq("ACGUACGG"), ic.seq("GGACGUGG")], 4, True)
    assert index_ref.first_difference(off, ids, off, ids, 4) is None
    bad = ids.copy()
    v = ic.value_of("ACGU")
    bad[off[v] + 1] = 7
    assert "(ACGU)" in index_ref.first_difference(off, bad, off, ids, 4)
    off2, ids2 = index_ref.build([ic.seq("ACGUACGG"), ic.seq("GGACCUGG")], 4, True)
    assert "(ACGU)" in index_ref.first_difference(off2, ids2, off, ids, 4)      # (the first list by value: ACGU < ACCU)
    assert index_ref.kmer_str(0, 3) == "AAA" and index_ref.kmer_str(63, 3) == "UUU" and index_ref.kmer_str(6, 2) == "GC"
