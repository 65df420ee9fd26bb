"""sina_hip_build_index (ref_kmer_keys, mark_unique, scatter_unique) and the bitmaps of the first search after it
(mark_dense, fill_dense) on the named stores and fuzz worlds of tests/index_cases.py, against tests/index_ref.py's plain
build: the downloaded index word for word, what the store reports, the score vector of every query and the top-`max`
exactly (tests/kmer_ref.py over the plain index), and the number of lists kept as bitmaps -- under both nofast settings
and with bitmaps at the default threshold, off and wherever a list is longer than 256.  tests/test_index_cpu.py pins the
plain build to the oracle and asserts that every case holds its edge.  Then the store's life cycle on one context: index
after index of other k, built and uploaded in turn, and what sina_hip_upload_refs leaves of an index."""
import os

import numpy as np
import pytest

from sina_amd import capi
from tests import index_cases as ic
from tests import index_ref, kmer_ref, util
from tests import kmer_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _same_index(ctx, want, k, tag):
    off, ids = ctx.download_index()
    diff = index_ref.first_difference(off, ids, want[0], want[1], k)
    assert diff is None, (tag, diff)


def _view(ctx):
    v = ctx.store_view()
    return int(v.n_postings), int(v.k), int(v.nofast), int(v.idx_ids_bytes), int(v.idx_offsets_bytes)


def _same_scores(ctx, qmasks, expected, maxes, tag):
    for qi, (m, e) in enumerate(zip(qmasks, expected)):
        got = ctx.kmer_scores(m)
        bad = np.flatnonzero(got != e["scores"])
        assert len(bad) == 0, (tag, "query %d" % qi, "%d scores differ, first: reference %d got %d want %d"
                               % (len(bad), bad[0], got[bad[0]], e["scores"][bad[0]]))
    qmask = np.concatenate(qmasks) if qmasks else np.zeros(0, np.uint8)
    qoff = np.zeros(len(qmasks) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(m) for m in qmasks])
    for mx in maxes:
        gi, gs, gn = ctx.kmer_topk(qmask, qoff, mx)
        for qi, e in enumerate(expected):
            wi, ws = e["find"][mx]
            assert gn[qi] == len(wi), (tag, "query %d" % qi, mx, int(gn[qi]), len(wi))
            bad = np.flatnonzero((gi[qi, :len(wi)] != wi) | (gs[qi, :len(wi)] != ws))
            assert len(bad) == 0, (tag, "query %d" % qi, mx, "%d entries differ, first: rank %d got (%d, %g) want (%d, %g)"
                                   % (len(bad), bad[0], gi[qi, bad[0]], gs[qi, bad[0]], wi[bad[0]], ws[bad[0]]))


def _run(ctx, c, monkeypatch):
    for nofast in c.nofasts:
        c.expected(nofast)                                # (the model's share of the time first)
    ctx.upload_refs(*c.packed())
    for nofast in c.nofasts:
        want = c.plain(nofast)
        for x, dd in enumerate(c.dense_divs):
            tag = (c.name, "nofast", nofast, "dense_div", dd)
            util.set_knobs(monkeypatch, dense_div=dd, kmer_rows=None, big_sel_bytes=None)
            ctx.build_index(c.k, nofast)                  # (bitmaps are rebuilt by the first search after this)
            if c.k < 12 or x == 0:                        # (k = 12: 64 MiB of offsets, once per nofast setting)
                _same_index(ctx, want, c.k, tag)
            assert _view(ctx) == (len(want[1]), c.k, int(nofast), 4 * len(want[1]), 4 * len(want[0])), tag
            _same_scores(ctx, c.qmasks, c.expected(nofast), c.maxes, tag)
            assert ctx.stats()["n_dense_lists"] == c.n_dense_lists(nofast, dd), tag


@pytest.mark.parametrize("name", list(ic.CASES))
def test_index_cases(ctx, monkeypatch, name):
    """Lengths around k, empty references, the window on the last word, ambiguity codes and words without a base bit at
    every place of a window, lower case, repeated k-mers and repeated references, block boundaries, both ends of the
    table, k from 1 to 12, stores without a window, lists on either side of the bitmap threshold."""
    _run(ctx, ic.case(name), monkeypatch)


@pytest.mark.parametrize("seed", range(int(os.environ.get("SINA_FUZZ_SEEDS", "12"))))
def test_index_fuzz(ctx, monkeypatch, seed):
    _run(ctx, ic.fuzz_world(seed), monkeypatch)


# ---------------------------------------------------------------- the store's life cycle

def _world(seed, n_refs=300, shortest=30, length=60, alphabet="AGCU"):
    """A store of its own for the life-cycle tests: (sequences, packed arrays, queries)."""
    rng = np.random.default_rng(9400 + seed)
    seqs = [ic.seq(ic.text_of(rng, int(n), alphabet)) for n in rng.integers(shortest, length + 1, size=n_refs)]
    off = np.zeros(n_refs + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    ab = np.concatenate([np.arange(len(s), dtype=np.uint32) | (s.astype(np.uint32) << 24) for s in seqs])
    return seqs, (ab, off, length), [seqs[r] for r in (0, 1, n_refs // 2, n_refs - 1)] + [ic.seq(ic.text_of(rng, 120, alphabet))]


def _expected(seqs, qs, k, nofast, maxes=(41,)):
    off, ids = index_ref.build(seqs, k, nofast)
    out = []
    for m in qs:
        s = kmer_ref.scores(off.astype(np.int64), ids, len(seqs), m, k, not nofast)
        out.append(dict(scores=s, find={mx: kmer_ref.topk(s, mx) for mx in maxes}))
    return (off, ids), out


def _dense_model(seqs, index, dd=None):
    return int((np.diff(index[0].astype(np.int64)) > kc.dense_threshold(len(seqs), dd)).sum())


def test_index_after_index_on_one_context(ctx, monkeypatch):
    """k = 6, 8, 6 again, 12 and 2 on one store of 300 references over two letters: the index buffers grow and shrink,
    every build leaves the plain index of its k and the scores follow it; at k = 2 every list is a bitmap, at the other
    k none is, and the number of bitmaps follows."""
    util.set_knobs(monkeypatch, dense_div=None, kmer_rows=None, big_sel_bytes=None)
    seqs, packed, qs = _world(1, alphabet="AG")
    ctx.upload_refs(*packed)
    dense = []
    for step, (k, nofast) in enumerate([(6, True), (8, False), (6, True), (12, True), (2, True)]):
        want, exp = _expected(seqs, qs, k, nofast)
        ctx.build_index(k, nofast)
        _same_index(ctx, want, k, ("step", step, "k", k))
        assert _view(ctx)[:3] == (len(want[1]), k, int(nofast))
        _same_scores(ctx, qs, exp, (41,), ("step", step, "k", k))
        dense.append(ctx.stats()["n_dense_lists"])
        assert dense[-1] == _dense_model(seqs, want), (step, k)
    assert dense == [0, 0, 0, 0, 4]


def test_refused_k_changes_nothing(ctx, monkeypatch):
    """k = 0 and k = 13 are refused by build_index and upload_index with their message; the index before stays."""
    util.set_knobs(monkeypatch, dense_div=None, kmer_rows=None, big_sel_bytes=None)
    seqs, packed, qs = _world(2, n_refs=50)
    want, exp = _expected(seqs, qs, 6, False)
    ctx.upload_refs(*packed)
    ctx.build_index(6, False)
    before = _view(ctx)
    for k in (0, 13):
        with pytest.raises(capi.SinaHipError, match="build_index: k must be in 1..12"):
            ctx.build_index(k, True)
        with pytest.raises(capi.SinaHipError, match="upload_index: k must be in 1..12"):
            ctx.upload_index(k, True, np.zeros(2, np.uint32), np.zeros(0, np.uint32))
        assert _view(ctx) == before
        _same_index(ctx, want, 6, ("after k", k))
        _same_scores(ctx, qs, exp, (41,), ("after k", k))


def test_uploaded_and_built_indexes_in_turn(ctx, monkeypatch):
    """upload_index of the plain no-fast index, searches; build_index on the same references as a fast index, searches;
    upload_index of what download_index returned: the same bytes as the build it came from."""
    util.set_knobs(monkeypatch, dense_div=None, kmer_rows=None, big_sel_bytes=None)
    seqs, packed, qs = _world(3)
    k = 4
    slow, exp_slow = _expected(seqs, qs, k, True)
    fast, exp_fast = _expected(seqs, qs, k, False)
    assert len(fast[1]) < len(slow[1])
    ctx.upload_refs(*packed)
    ctx.upload_index(k, True, *slow)
    _same_index(ctx, slow, k, "uploaded")
    _same_scores(ctx, qs, exp_slow, (41,), "uploaded")
    ctx.build_index(k, False)
    _same_index(ctx, fast, k, "built")
    assert _view(ctx)[:3] == (len(fast[1]), k, 0)
    _same_scores(ctx, qs, exp_fast, (41,), "built")
    built = [ctx.kmer_scores(m).tobytes() for m in qs] + [x.tobytes() for x in ctx.kmer_topk(np.concatenate(qs), np.cumsum([0] + [len(m) for m in qs]).astype(np.uint64), 41)]
    off, ids = ctx.download_index()
    ctx.upload_index(k, False, off, ids)
    _same_index(ctx, fast, k, "uploaded again")
    again = [ctx.kmer_scores(m).tobytes() for m in qs] + [x.tobytes() for x in ctx.kmer_topk(np.concatenate(qs), np.cumsum([0] + [len(m) for m in qs]).astype(np.uint64), 41)]
    assert again == built


def test_bitmaps_go_with_the_index_that_had_them(ctx, monkeypatch):
    """A store whose k = 2 index has bitmaps, then build_index with k = 8, at which the same references have none:
    n_dense_lists goes to 0 and the scores stay right; and back."""
    util.set_knobs(monkeypatch, dense_div=None, kmer_rows=None, big_sel_bytes=None)
    seqs, packed, qs = _world(4)
    ctx.upload_refs(*packed)
    for k, some in ((2, True), (8, False), (2, True)):
        want, exp = _expected(seqs, qs, k, True)
        assert (_dense_model(seqs, want) > 0) == some
        ctx.build_index(k, True)
        _same_scores(ctx, qs, exp, (41,), ("k", k))
        assert ctx.stats()["n_dense_lists"] == _dense_model(seqs, want)
        _same_index(ctx, want, k, ("k", k))


def test_upload_refs_forgets_the_index(ctx, monkeypatch):
    """After sina_hip_upload_refs of other references the index is gone: download_index and the searches say "no index",
    the store view shows none, no bitmap is left; build_index then gives the new store's index.  The second store has
    exactly as many references as the first, and the download is asserted first: where the index survived the upload,
    the test ends there and no search has run over lists of other references."""
    util.set_knobs(monkeypatch, dense_div=None, kmer_rows=None, big_sel_bytes=None)
    k = 2
    seqs_a, packed_a, qs_a = _world(5)
    seqs_b, packed_b, qs_b = _world(6)
    assert len(seqs_a) == len(seqs_b) and any(len(a) != len(b) or (a != b).any() for a, b in zip(seqs_a, seqs_b))
    want_a, exp_a = _expected(seqs_a, qs_a, k, True)
    ctx.upload_refs(*packed_a)
    ctx.build_index(k, True)
    _same_scores(ctx, qs_a, exp_a, (41,), "first store")
    assert ctx.stats()["n_dense_lists"] == _dense_model(seqs_a, want_a) > 0
    ctx.upload_refs(*packed_b)
    with pytest.raises(capi.SinaHipError, match="no index"):
        ctx.download_index()
    v = ctx.store_view()
    assert (int(v.n_postings), int(v.k), int(v.idx_ids_bytes), int(v.idx_offsets_bytes)) == (0, 0, 0, 0)
    assert not v.idx_offsets and not v.idx_ids and int(v.n_refs) == len(seqs_b)
    assert ctx.stats()["n_dense_lists"] == 0
    with pytest.raises(capi.SinaHipError, match="no index"):
        ctx.kmer_scores(qs_b[0])
    with pytest.raises(capi.SinaHipError, match="no index"):
        ctx.kmer_topk(qs_b[0], np.array([0, len(qs_b[0])], np.uint64), 41)
    want_b, exp_b = _expected(seqs_b, qs_b, k, True)
    ctx.build_index(k, True)
    _same_index(ctx, want_b, k, "second store")
    _same_scores(ctx, qs_b, exp_b, (41,), "second store")
    assert ctx.stats()["n_dense_lists"] == _dense_model(seqs_b, want_b) > 0
