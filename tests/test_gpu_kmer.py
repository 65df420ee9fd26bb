"""kmer_count_kernel<false / true>, kmer_count_long_kernel, kmer_select_kernel<> and kmer_select_cand_kernel on hand-built
posting lists: the named cases and fuzz worlds of tests/kmer_cases.py, uploaded with sina_hip_upload_index, against
tests/kmer_ref.py's plain model -- the full score vector of every query and the top-`max` of every `max`, ids, scores and
n, exactly, under every SINA_HIP_TEST setting the case names (tests/test_kmer_cpu.py pins that model to the oracle and
asserts that every case reaches its edge).  Beside the results: the number of lists the index keeps as bitmaps, and by
how many launches a search advanced (a candidate list that overflows costs a second one)."""
import os

import numpy as np
import pytest

from sina_amd import capi
from tests import kmer_cases as kc
from tests import util

pytestmark = pytest.mark.gpu


def _check(ctx, c, tag, rows):
    for qi, (m, e) in enumerate(zip(c.qmasks, c.expected)):
        got = ctx.kmer_scores(m, long_ok=c.long_api)
        bad = np.flatnonzero(got != e["scores"])
        assert len(bad) == 0, (tag, c.labels[qi], "%d scores differ, first: reference %d got %d want %d"
                               % (len(bad), bad[0], got[bad[0]], e["scores"][bad[0]]))
    for mx in c.maxes:
        before = ctx.stats()["kmer_launches"]
        gi, gs, gn = ctx.kmer_topk(c.qmask, c.qoff, mx, long_ok=c.long_api)
        if not c.long_api:
            assert ctx.stats()["kmer_launches"] - before == kc.expected_launches(c, mx, rows), (tag, mx)
        for qi, e in enumerate(c.expected):
            wi, ws = e["find"][mx]
            assert gn[qi] == len(wi), (tag, c.labels[qi], mx, int(gn[qi]), len(wi))
            bad = np.flatnonzero((gi[qi, :len(wi)] != wi) | (gs[qi, :len(wi)] != ws))
            assert len(bad) == 0, (tag, c.labels[qi], mx, "%d entries differ, first: rank %d got (%d, %g) want (%d, %g)"
                                   % (len(bad), bad[0], gi[qi, bad[0]], gs[qi, bad[0]], wi[bad[0]], ws[bad[0]]))


def _run(c, monkeypatch):
    c.expected                                            # (the model's share of the time first)
    ctx = capi.Context(0)
    try:
        ctx.upload_refs(*c.ref_store())
        for dd in c.dense_divs:
            util.set_knobs(monkeypatch, dense_div=dd, kmer_rows=None)
            ctx.upload_index(c.k, c.nofast, c.off, c.ids)          # (bitmaps are rebuilt by the first search after this)
            for rows in c.kmer_rows:
                util.set_knobs(monkeypatch, kmer_rows=rows)
                long_before = ctx.long_queries()
                _check(ctx, c, (c.name, "dense_div", dd, "kmer_rows", rows), rows)
                assert ctx.stats()["n_dense_lists"] == kc.n_dense_lists(c, dd), (c.name, dd)
                if c.long_api:
                    assert ctx.long_queries() - long_before == c.n_long * (1 + len(c.maxes))
                else:
                    assert ctx.long_queries() == long_before
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(kc.COUNT_CASES))
def test_kmer_count_cases(monkeypatch, name):
    """Bit-sliced bitmaps at every plane count, the 1023-window limit, multiplicities, cursor streaming at the probe's
    and the loop's exits, tile ends, a fast index, a mixed batch: with bitmaps on, off and everywhere."""
    _run(kc.case(name), monkeypatch)


@pytest.mark.parametrize("name", list(kc.SELECT_CASES))
def test_kmer_select_cases(monkeypatch, name):
    """Score rows built to order: every exit of the sampled short cut, the take-all boundary, the tie split of the
    ordered pass at wave-range, iteration and vector boundaries, narrow score ranges, rows behind long queries."""
    _run(kc.case(name), monkeypatch)


@pytest.mark.parametrize("name", list(kc.CAND_CASES))
def test_kmer_cand_cases(monkeypatch, name):
    """The candidate-list path: where tile 0's threshold lands, a list of exactly 4096 and of 4097, ties over three
    tiles; each also with the score rows forced, which must give the same bytes."""
    _run(kc.case(name), monkeypatch)


@pytest.mark.parametrize("seed", range(int(os.environ.get("SINA_FUZZ_SEEDS", "12"))))
def test_kmer_index_fuzz(monkeypatch, seed):
    """Seeded worlds of random posting lists on both sides of the dense threshold, random k-mer queries with
    multiplicities and N padding, a random threshold and three random max values."""
    _run(kc.fuzz_world(seed), monkeypatch)
