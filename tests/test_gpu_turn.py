"""turn_orient_kernel and turn_pick_kernel around the k-mer search, through sina_hip_kmer_topk_turn: the named cases and
fuzz calls of tests/turn_cases.py under every setting they name, against tests/turn_ref.py's plain model -- the chosen
orientation and the four top-1 scores -- and the rows against both the model and a sina_hip_kmer_topk_any call on the
chosen variant's bytes on the same context, exactly (tests/test_turn_cpu.py pins the model to the oracle and asserts
that every case sits on its edge).  Beside the results: sina_hip_turn_stats' queries, turned queries and launches as the
case predicts them, and that a context which has served a turn call answers sina_hip_kmer_topk_any as before."""
import os

import numpy as np
import pytest

from sina_amd import capi
from tests import turn_cases as tc
from tests import turn_ref as tr
from tests import util

pytestmark = pytest.mark.gpu

KNOBS = ("kmer_rows", "turn_range", "big_sel_bytes", "dense_div", "turn_fail")


@pytest.fixture(scope="module")
def contexts():
    """One context per world, shared by the cases on it."""
    made = {}

    def get(w):
        if id(w) not in made:
            ctx = capi.Context(0)
            ctx.upload_refs(*w.ref_store())
            ctx.upload_index(w.k, w.nofast, w.off, w.ids)
            made[id(w)] = ctx
        return made[id(w)]
    yield get
    for ctx in made.values():
        ctx.close()


def _offsets(masks):
    off = np.zeros(len(masks) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in masks])
    return off


def _run(ctx, c, monkeypatch):
    c.why(c)
    for r in c.runs:
        util.set_knobs(monkeypatch, **{k: r["knobs"].get(k) for k in KNOBS})
        tag = (c.name, r)
        want = c.expected(r["all"], r["mx"])
        s0, long0 = ctx.turn_stats(), ctx.long_queries()
        turn, top1, ids, sc, n = ctx.kmer_topk_turn(c.qmask, c.qoff, r["mx"], r["all"])
        s1 = ctx.turn_stats()
        chosen = [tr.variant(m, int(t)) for m, t in zip(c.qmasks, turn)]
        ai, asc, an = ctx.kmer_topk_any(np.concatenate(chosen), _offsets(chosen), r["mx"])
        assert ctx.turn_stats() == s1                                  # (a plain search leaves the record alone)
        for qi, e in enumerate(want):
            lb = c.labels[qi]
            assert turn[qi] == e["turn"], (tag, lb, int(turn[qi]), e["turn"], top1[qi].tolist(), e["top1"].tolist())
            assert (top1[qi] == e["top1"]).all(), (tag, lb, top1[qi].tolist(), e["top1"].tolist())
            k = len(e["ids"])
            assert n[qi] == k == an[qi], (tag, lb, int(n[qi]), k, int(an[qi]))
            bad = np.flatnonzero((ids[qi, :k] != e["ids"]) | (sc[qi, :k] != e["scores"]))
            assert len(bad) == 0, (tag, lb, "%d entries differ from the model, first: rank %d got (%d, %g) want (%d, %g)"
                                   % (len(bad), bad[0], ids[qi, bad[0]], sc[qi, bad[0]], e["ids"][bad[0]], e["scores"][bad[0]]))
            assert (ids[qi, :k] == ai[qi, :k]).all() and (sc[qi, :k].view(np.uint32) == asc[qi, :k].view(np.uint32)).all(), (tag, lb)
        assert s1["queries"] - s0["queries"] == len(c.qmasks), tag
        assert s1["turned"] - s0["turned"] == sum(e["turn"] != 0 for e in want), tag
        assert s1["launches"] - s0["launches"] == 1 + c.pick_launches(r["knobs"]), tag
        assert s1["kernel_ms"] > s0["kernel_ms"], tag
        assert ctx.long_queries() - long0 == 2 * c.n_long(), tag        # (the turn call's and the plain call's)


@pytest.mark.parametrize("name", tc.NAMES)
def test_turn_cases(contexts, monkeypatch, name):
    """Lengths at every byte offset, the whole alphabet, a winner at each orientation, ties, nothing found, score rows and
    candidate lists, an overflow in a later variant, the big select, a long query, ranges of one to three queries."""
    c = tc.case(name)
    _run(contexts(c.world), c, monkeypatch)


@pytest.mark.parametrize("seed", range(int(os.environ.get("SINA_FUZZ_SEEDS", str(tc.FUZZ_SEEDS)))))
def test_turn_fuzz(contexts, monkeypatch, seed):
    c = tc.fuzz(seed)
    _run(contexts(c.world), c, monkeypatch)


def test_plain_search_unchanged_after_a_turn_call(monkeypatch):
    """A fresh context answers sina_hip_kmer_topk_any; then serves turn calls (score rows, and a query of no bases among
    them); then answers the same plain call with the same bytes.  A refused call (max = 0) leaves the outputs alone."""
    util.set_knobs(monkeypatch, **{k: None for k in KNOBS})
    c = tc.case("winners_small")
    w = c.world
    ctx = capi.Context(0)
    try:
        ctx.upload_refs(*w.ref_store())
        ctx.upload_index(w.k, w.nofast, w.off, w.ids)
        before = ctx.kmer_topk_any(c.qmask, c.qoff, 41)
        masks = c.qmasks[:3] + [np.zeros(0, np.uint8)] + c.qmasks[3:]
        turn, top1, ids, sc, n = ctx.kmer_topk_turn(np.concatenate(masks), _offsets(masks), 41, True)
        want = c.expected(True, 41)
        assert [int(t) for t in turn] == [e["turn"] for e in want[:3]] + [0] + [e["turn"] for e in want[3:]]
        assert (top1[3] == 0).all() and n[3] == 41
        ctx.kmer_topk_turn(c.qmask, c.qoff, 129, False)
        after = ctx.kmer_topk_any(c.qmask, c.qoff, 41)
        for a, b in zip(before, after):
            assert (a.view(np.uint32) == b.view(np.uint32)).all()
        with pytest.raises(RuntimeError, match="max must be 1 or more"):
            ctx.kmer_topk_turn(c.qmask, c.qoff, 0, True)
        util.set_knobs(monkeypatch, turn_fail=1)
        with pytest.raises(RuntimeError, match="turn_fail"):
            ctx.kmer_topk_turn(c.qmask, c.qoff, 41, True)
    finally:
        ctx.close()
