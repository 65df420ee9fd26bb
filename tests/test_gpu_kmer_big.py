"""kmer_select_big_kernel, the segmented sort behind it and its launch ranges: the cases of tests/kmer_big_cases.py
through sina_hip_kmer_topk / sina_hip_kmer_topk_any against tests/kmer_ref.py -- ids, scores and n exactly, for every
max --, with sina_hip_big_select_queries advancing by the number of queries wherever min(max, n_refs) is above 4096 and by
nothing otherwise, and kmer_launches by the number of launch ranges (tests/test_kmer_big_cpu.py pins the model and the
cases' edges)."""
import os

import numpy as np
import pytest

from sina_amd import capi
from tests import kmer_big_cases as kb
from tests import util

pytestmark = pytest.mark.gpu


def _topk(ctx, c, mx, tag, budget=kb.BIG_BUDGET):
    """One kmer_topk of the case's batch, checked against the model; returns the raw arrays."""
    big0, l0 = ctx.big_select_queries(), ctx.stats()["kmer_launches"]
    gi, gs, gn = ctx.kmer_topk(c.qmask, c.qoff, mx, long_ok=c.long_api)
    assert ctx.big_select_queries() - big0 == kb.big_queries(c, mx), (tag, mx)
    assert ctx.stats()["kmer_launches"] - l0 == kb.launches_model(c, mx, budget), (tag, mx)
    for qi, e in enumerate(c.expected):
        wi, ws = e["find"][mx]
        assert gn[qi] == len(wi), (tag, c.labels[qi], mx, int(gn[qi]), len(wi))
        bad = np.flatnonzero((gi[qi, :len(wi)] != wi) | (gs[qi, :len(wi)] != ws))
        assert len(bad) == 0, (tag, c.labels[qi], mx, "%d entries differ, first: rank %d got (%d, %g) want (%d, %g)"
                               % (len(bad), bad[0], gi[qi, bad[0]], gs[qi, bad[0]], wi[bad[0]], ws[bad[0]]))
    return gi, gs, gn


def _run(c, monkeypatch):
    c.expected
    ctx = capi.Context(0)
    try:
        ctx.upload_refs(*c.ref_store())
        for dd in c.dense_divs:
            util.set_knobs(monkeypatch, dense_div=dd, kmer_rows=None, big_sel_bytes=None)
            ctx.upload_index(c.k, c.nofast, c.off, c.ids)
            for mx in c.maxes:
                _topk(ctx, c, mx, (c.name, "dense_div", dd))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(kb.BIG_CASES))
def test_kmer_big_select_cases(monkeypatch, name):
    """The 4096 / 4097 seam, clipping to n_refs, zeros filling the list, the tie split at wave-range, iteration and
    vector boundaries with more than 4096 ties, every exit of the sampled short cut at M > 4096, M == n_refs across
    tiles, a row behind a long query, a mixed batch whose segments must not leak into each other."""
    _run(kb.case(name), monkeypatch)


@pytest.mark.parametrize("seam", list(kb.seam_budgets()))
def test_kmer_big_select_range_seam(monkeypatch, seam):
    """The mixed batch under SINA_HIP_TEST=big_sel_bytes=N: the launch ranges the budget cuts give the bytes of the
    one-range run, in as many launches as there are ranges."""
    c = kb.mixed_batch()
    budget, ranges = kb.seam_budgets()[seam]
    ctx = capi.Context(0)
    try:
        ctx.upload_refs(*c.ref_store())
        ctx.upload_index(c.k, c.nofast, c.off, c.ids)
        util.set_knobs(monkeypatch, big_sel_bytes=None)
        one = _topk(ctx, c, kb.MIXED_M, (c.name, "one range"))
        util.set_knobs(monkeypatch, big_sel_bytes=budget)
        l0 = ctx.stats()["kmer_launches"]
        cut = _topk(ctx, c, kb.MIXED_M, (c.name, seam), budget)
        assert ctx.stats()["kmer_launches"] - l0 == len(ranges) > 1
        for a, b in zip(one, cut):
            assert a.tobytes() == b.tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", kb.fuzz_seeds(int(os.environ.get("SINA_FUZZ_SEEDS", "12"))))
def test_kmer_big_select_fuzz(monkeypatch, seed):
    """The seeded worlds of kmer_cases.fuzz_world with more than 4097 references, three random max values in 4097 ..
    n_refs + 10 each."""
    _run(kb.fuzz_big(seed), monkeypatch)
