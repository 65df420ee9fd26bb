"""match_count_kernel and its two entry points against a plain walk.

sina_hip_match_count (Context.match_counts): the `match` counter of every (query, candidate) pair of tests/msc_cases.py
and of the named cases and fuzz seeds of tests/compare_cases.py equals the lock-step walk's (tests/compare_ref.py,
optimistic rule, no filter), integer for integer, and sina_hip_compare's on the same pairs; sub-ranges of larger
arrays, every refusal, scratch reuse.  The two compare_cases worlds of 524 288 columns (lds_wide, lds_limit) are wider
than the kernel's LDS table allows (327 680 columns): for them the test asserts the refusal as a limit, which is what
sends the host stage to its walk.

sina_hip_kmer_topk_match (Context.kmer_topk_match) on the hand-built posting-list worlds of tests/kmer_cases.py and
tests/kmer_big_cases.py: ids, scores and n byte-equal to sina_hip_kmer_topk_any's, every match count equal to the
walk's for its (query, id), across launch ranges, the long-query reordering and a repeated candidate-list pass."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from sina_amd import capi
from tests import compare_cases as cc
from tests import kmer_big_cases as kb
from tests import kmer_cases as kc
from tests import msc_cases as mc
from tests import util

pytestmark = pytest.mark.gpu

SENTINEL = 0xBEEF


def _upload(ctx, width, refs):
    ctx.upload_refs(cc.flat(refs), cc.offsets(refs), width)


def _launch(ctx, qs, cand):
    return ctx.match_counts(cc.flat(qs), cc.offsets(qs), cc.flat(cand), cc.offsets(cand))


def _equal(got, want, cand, tag):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, tag
    bad = np.flatnonzero(got != want)
    if len(bad):
        at = int(bad[0])
        qi = int(np.searchsorted(cc.offsets(cand), at, side="right")) - 1
        raise AssertionError((tag, "%d of %d pairs differ, first: pair %d (query %d, reference %d) got %d want %d"
                              % (len(bad), len(want), at, qi, int(cc.flat(cand)[at]), got[at], want[at])))


def _check_world(ctx, width, refs, qs, cand, want6, tag, compare=True):
    _upload(ctx, width, refs)
    p0 = ctx.match_stats()
    _equal(_launch(ctx, qs, cand), want6[:, 4], cand, (tag, "walk"))
    p1 = ctx.match_stats()
    n_pairs = sum(len(c) for c in cand)
    assert p1["pairs"] - p0["pairs"] == n_pairs and p1["launches"] - p0["launches"] == (1 if n_pairs else 0), tag
    assert p1["cand_bases"] - p0["cand_bases"] == sum(len(refs[int(i)]) for c in cand for i in c), tag
    if compare:      # the same pairs through the search stage's kernel
        six = ctx.compare(cc.flat(qs), cc.offsets(qs), cc.flat(cand), cc.offsets(cand), 0, False)
        _equal(six[:, 4], want6[:, 4], cand, (tag, "compare_kernel"))


def _too_wide(ctx, width, refs, qs, cand, tag):
    assert width > mc.MAX_WIDTH
    _upload(ctx, width, refs)
    out = np.full(max(1, sum(len(c) for c in cand)), SENTINEL, np.uint16)
    rc = _raw(ctx, cc.flat(qs), cc.offsets(qs), len(qs), cc.flat(cand), cc.offsets(cand), out)
    assert rc != 0 and "too wide for the device match count" in _error(ctx) and ctx.last_error_is_limit(), tag
    assert (out == SENTINEL).all()


@pytest.mark.parametrize("name", mc.NAMES)
def test_match_counts_msc_cases(oracle, gpu_ctx, name):
    if name == "list_chunks_above_floor":           # (built for this device's compute units)
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        width, refs, qs, cand = mc.list_chunks_above_floor(n_cu)
        mc.check_wellformed(width, refs, qs, cand)
        memo = {}
        rows = [memo.setdefault((q.tobytes(), int(i)), cc.compare_ref.compare_ref(q, refs[int(i)], 0, False))
                for q, ids in zip(qs, cand) for i in ids]
        want = np.asarray(rows, np.int32).reshape(-1, 6)
    else:
        width, refs, qs, cand = mc.case(name)
        want = mc.expected(name)
    # (sina_hip_compare is given queries inside the alignment only)
    inside = all(len(q) == 0 or cc.cols(q)[-1] < width for q in qs)
    _check_world(gpu_ctx, width, refs, qs, cand, want, name, compare=inside)


@pytest.mark.parametrize("name", cc.NAMES)
def test_match_counts_compare_cases(oracle, gpu_ctx, name):
    width, refs, qs, cand = cc.case(name)
    if width > mc.MAX_WIDTH:
        assert name in ("lds_wide", "lds_limit")
        _too_wide(gpu_ctx, width, refs, qs, cand, name)
        return
    _check_world(gpu_ctx, width, refs, qs, cand, cc.expected(name)[0, False], name)


@pytest.mark.parametrize("seed", range(int(os.environ.get("SINA_FUZZ_SEEDS", "12"))))
def test_match_counts_fuzz(oracle, gpu_ctx, seed):
    width, refs, qs, cand = cc.fuzz_case(seed)
    _check_world(gpu_ctx, width, refs, qs, cand, cc.expected("fuzz", seed)[0, False], "seed %d" % seed)


# ---------------------------------------------------------------- the entry point

def _raw(ctx, q_ab, q_off, nq, cand_ids, cand_off, out):
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    return ctx.L.sina_hip_match_count(ctx.h, p(q_ab, capi.u32p), p(q_off, capi.u64p), nq, p(cand_ids, capi.u32p),
                                      p(cand_off, capi.u64p), p(out, capi.u16p))


def _error(ctx):
    return ctx.L.sina_hip_last_error().decode()


def test_match_counts_subrange_of_larger_arrays(oracle, gpu_ctx):
    """q_off[0] != 0 and cand_off[0] != 0: queries 3 .. 7 of `cand_lists` addressed inside the full arrays; the counts
    land at cand_off[lo] .. cand_off[hi] - 1 of the output and nothing is written before or behind them."""
    width, refs, qs, cand = cc.case("cand_lists")
    q_ab, q_off, c_ids, c_off = cc.flat(qs), cc.offsets(qs), cc.flat(cand), cc.offsets(cand)
    lo, hi = 3, 8
    assert q_off[lo] != 0 and c_off[lo] != 0 and c_off[hi] < c_off[-1]
    a, b = int(c_off[lo]), int(c_off[hi])
    _upload(gpu_ctx, width, refs)
    want = cc.expected("cand_lists")[0, False][:, 4]
    out = np.full(len(c_ids) + 4, SENTINEL, np.uint16)
    assert _raw(gpu_ctx, q_ab, q_off[lo:], hi - lo, c_ids, c_off[lo:], out) == 0, _error(gpu_ctx)
    _equal(out[a:b], want[a:b], cand[lo:hi], "sub-range")
    assert (out[:a] == SENTINEL).all() and (out[b:] == SENTINEL).all()
    _equal(_launch(gpu_ctx, qs[lo:hi], cand[lo:hi]), want[a:b], cand[lo:hi], "alone")


def test_match_counts_reuses_its_buffers(oracle):
    """One context: a large launch, a small one, the large one again; then stores of other widths."""
    ctx = capi.Context(0)
    try:
        width, refs, qs, cand = cc.case("lengths")
        want = cc.expected("lengths")[0, False][:, 4]
        _upload(ctx, width, refs)
        small_q, small_c = qs[:1], [cand[0][:1]]
        for tag in ("first", "second"):
            _equal(_launch(ctx, qs, cand), want, cand, ("large", tag))
            _equal(_launch(ctx, small_q, small_c), want[:1], small_c, ("small", tag))
        assert cc.case("ranges")[0] != width and cc.case("nwords_257")[0] > width
        for name in ("ranges", "nwords_257", "lengths"):
            w, r, q, c = cc.case(name)
            _upload(ctx, w, r)
            _equal(_launch(ctx, q, c), cc.expected(name)[0, False][:, 4], c, name)
    finally:
        ctx.close()


def test_match_counts_refusals(oracle):
    """Every argument check returns nonzero with its message, before any launch and with the output untouched, and the
    context computes a small case correctly afterwards."""
    ctx = capi.Context(0)
    try:
        width, refs, qs, cand = cc.case("ranges")
        q_ab, q_off, c_ids, c_off = cc.flat(qs), cc.offsets(qs), cc.flat(cand), cc.offsets(cand)
        nq = len(qs)
        want = cc.expected("ranges")[0, False][:, 4]

        def refused(message, *args, out=Ellipsis, limit=False):
            o = np.full(len(c_ids) + 8, SENTINEL, np.uint16) if out is Ellipsis else out
            launches = ctx.match_stats()["launches"]
            assert _raw(ctx, *args, o) != 0, message
            assert message in _error(ctx), (message, _error(ctx))
            assert ctx.last_error_is_limit() == limit
            assert o is None or (o == SENTINEL).all()
            assert ctx.match_stats()["launches"] == launches
            if ctx.n_refs == len(refs):
                _equal(_launch(ctx, qs, cand), want, cand, ("after", message))

        refused("upload references first", q_ab, q_off, nq, c_ids, c_off)
        _upload(ctx, width, refs)
        refused("null argument", None, q_off, nq, c_ids, c_off)
        refused("null argument", q_ab, None, nq, c_ids, c_off)
        refused("null argument", q_ab, q_off, nq, None, c_off)
        refused("null argument", q_ab, q_off, nq, c_ids, None)
        refused("null argument", q_ab, q_off, nq, c_ids, c_off, out=None)
        ids = c_ids.copy()
        ids[-1] = len(refs)
        refused("reference id out of range", q_ab, q_off, nq, ids, c_off)
        one = np.array([0, 1], np.uint64)
        refused("query longer than 65535 bases", cc.seq(range(65536)), np.array([0, 65536], np.uint64), 1,
                np.zeros(1, np.uint32), one)
        twice = np.array([5 | 1 << 24, 9 | 2 << 24, 9 | 4 << 24, 12 | 1 << 24], np.uint32)       # two equal columns
        refused("query columns do not ascend strictly", twice, np.array([0, 4], np.uint64), 1, np.zeros(1, np.uint32), one)
        back = np.array([5 | 1 << 24, 4 | 2 << 24], np.uint32)
        refused("query columns do not ascend strictly", back, np.array([0, 2], np.uint64), 1, np.zeros(1, np.uint32), one)
        # nothing to do: no query, or only empty lists
        out = np.full(4, SENTINEL, np.uint16)
        assert _raw(ctx, q_ab, q_off, 0, c_ids, c_off, out) == 0 and (out == SENTINEL).all()
        assert _raw(ctx, q_ab, q_off, 3, c_ids, np.zeros(4, np.uint64), out) == 0 and (out == SENTINEL).all()
        # a query of exactly 65535 bases is taken
        q65535 = cc.seq(range(65535))
        got = ctx.match_counts(q65535, np.array([0, 65535], np.uint64), np.zeros(1, np.uint32), one)
        assert int(got[0]) == mc.match_ref(q65535, refs[0])
        # the widest alignment the table holds, and one column more
        wide_ref = [cc.seq([0, 9, mc.MAX_WIDTH - 1], [1, 2, 4])]
        _upload(ctx, mc.MAX_WIDTH, wide_ref)
        got = ctx.match_counts(wide_ref[0], np.array([0, 3], np.uint64), np.zeros(1, np.uint32), one)
        assert int(got[0]) == 3
        _upload(ctx, mc.MAX_WIDTH + 1, wide_ref)
        refused("too wide for the device match count", wide_ref[0], np.array([0, 3], np.uint64), 1, np.zeros(1, np.uint32), one,
                limit=True)
    finally:
        ctx.close()


# ---------------------------------------------------------------- sina_hip_kmer_topk_match

WORLD_WIDTH = 48


def _world_refs(n_refs):
    """n_refs references of three bases each inside WORLD_WIDTH columns, as (flat packed words, offsets, cols, masks)."""
    i = np.arange(n_refs, dtype=np.int64)
    cols = np.stack([i % 7, 8 + i % 11, 20 + (i * 7) % 23], axis=1)
    masks = np.stack([1 << (i % 4), 1 << ((i // 4) % 4), np.where(i % 5 == 0, 15, 1 << ((i // 16) % 4))], axis=1)
    assert (np.diff(cols, axis=1) > 0).all() and cols.max() < WORLD_WIDTH
    ab = (cols | (masks << 24)).astype(np.uint32).reshape(-1)
    return ab, np.arange(n_refs + 1, dtype=np.uint64) * 3, cols, masks


def _packed_queries(qmasks, stride):
    """The k-mer cases' mask bytes as aligned queries: base i in column stride * i."""
    return [(np.arange(len(m), dtype=np.uint32) * stride) | (m.astype(np.uint32) << 24) for m in qmasks]


def _want_match(q, cols, masks, ids):
    tab = np.zeros(WORLD_WIDTH, np.int64)
    inside = cc.cols(q) < WORLD_WIDTH
    tab[cc.cols(q)[inside]] = cc.masks(q)[inside] & 0xF
    return ((tab[cols[ids]] & masks[ids]) != 0).sum(axis=1)


def _topk_match(ctx, qmasks, mx, cols, masks, tag, stride=1):
    qs = _packed_queries(qmasks, stride)
    q_ab, q_off = cc.flat(qs), cc.offsets(qs)
    wi, ws, wn = ctx.kmer_topk_any(np.concatenate(qmasks), q_off, mx)
    s0 = ctx.match_stats()
    gi, gs, gn, gm = ctx.kmer_topk_match(q_ab, q_off, mx)
    s1 = ctx.match_stats()
    assert gi.tobytes() == wi.tobytes() and gs.tobytes() == ws.tobytes() and gn.tobytes() == wn.tobytes(), (tag, mx)
    assert s1["pairs"] - s0["pairs"] == int(gn.sum()), (tag, mx)
    for qi, q in enumerate(qs):
        n = int(gn[qi])
        want = _want_match(q, cols, masks, gi[qi, :n].astype(np.int64))
        bad = np.flatnonzero(gm[qi, :n] != want)
        assert len(bad) == 0, (tag, mx, "query %d: %d of %d counts differ, first: rank %d id %d got %d want %d"
                               % (qi, len(bad), n, bad[0], gi[qi, bad[0]], gm[qi, bad[0]], want[bad[0]]))
    return s1["launches"] - s0["launches"]


def test_topk_match_maxes_and_launch_ranges(monkeypatch):
    """The mixed batch of kmer_big_cases: max 1, 41, 4096, 4097 and above n_refs; then 4500 under a budget that cuts
    the four queries into several launch ranges -- one match launch per range, the same bytes."""
    c = kb.mixed_batch()
    ctx = capi.Context(0)
    try:
        ab, off, cols, masks = _world_refs(c.n_refs)
        ctx.upload_refs(ab, off, WORLD_WIDTH)
        util.set_knobs(monkeypatch, dense_div=None, kmer_rows=None, big_sel_bytes=None)
        ctx.upload_index(c.k, c.nofast, c.off, c.ids)
        for mx in (1, 41, 4096, 4097, c.n_refs + 10):
            assert _topk_match(ctx, c.qmasks, mx, cols, masks, c.name) == 1
        assert _topk_match(ctx, c.qmasks, 41, cols, masks, (c.name, "stride 2"), stride=2) == 1
        for seam, (budget, ranges) in kb.seam_budgets().items():
            util.set_knobs(monkeypatch, big_sel_bytes=budget)
            assert _topk_match(ctx, c.qmasks, kb.MIXED_M, cols, masks, (c.name, seam)) == len(ranges) > 1
    finally:
        ctx.close()


def test_topk_match_long_query_among_short_ones(monkeypatch):
    """A query above 10 240 bases between two short ones: the long count kernel's range runs behind the others, the
    rows -- match counts included -- come back in the caller's order."""
    c = kb.long_query()
    qmasks = [c.qmasks[0], c.qmasks[2], kc.poly("A", 50), c.qmasks[1], kc.poly("C", 30)]
    assert [len(m) > kc.FAST_MAX for m in qmasks] == [False, True, False, True, False]
    ctx = capi.Context(0)
    try:
        ab, off, cols, masks = _world_refs(c.n_refs)
        ctx.upload_refs(ab, off, WORLD_WIDTH)
        util.set_knobs(monkeypatch, dense_div=None, kmer_rows=None, big_sel_bytes=None)
        ctx.upload_index(c.k, c.nofast, c.off, c.ids)
        long0 = ctx.long_queries()
        for mx in (41, 5000):
            assert _topk_match(ctx, qmasks, mx, cols, masks, c.name) == 2       # the fast range and the long one
        assert ctx.long_queries() - long0 == 2 * 2 * 2                          # (two calls per max, two long queries)
    finally:
        ctx.close()


def test_topk_match_after_a_candidate_list_overflow(monkeypatch):
    """cap_4097: the candidate list of the first pass overflows, the range is repeated with the score rows; the
    overflowed pass launches no match count, the rows are those of the final select."""
    c = kc.cap(4097)
    ctx = capi.Context(0)
    try:
        ab, off, cols, masks = _world_refs(c.n_refs)
        ctx.upload_refs(ab, off, WORLD_WIDTH)
        util.set_knobs(monkeypatch, dense_div=None, kmer_rows=None, big_sel_bytes=None)
        ctx.upload_index(c.k, c.nofast, c.off, c.ids)
        for mx in (41, 128):
            l0 = ctx.stats()["kmer_launches"]
            assert _topk_match(ctx, c.qmasks, mx, cols, masks, c.name) == 1
            assert ctx.stats()["kmer_launches"] - l0 == 2 * 2                    # (topk_any and topk_match: two passes each)
        c1 = kc.cap(4096)                                                        # ... and the list that just fits
        ctx.upload_index(c1.k, c1.nofast, c1.off, c1.ids)
        l0 = ctx.stats()["kmer_launches"]
        assert _topk_match(ctx, c1.qmasks, 41, cols, masks, c1.name) == 1
        assert ctx.stats()["kmer_launches"] - l0 == 2
    finally:
        ctx.close()


def test_topk_match_refuses_unsorted_columns(gpu_ctx):
    ab, off, cols, masks = _world_refs(100)
    gpu_ctx.upload_refs(ab, off, WORLD_WIDTH)
    gpu_ctx.build_index(6, True)
    q = np.array([3 | 1 << 24, 3 | 2 << 24, 5 | 4 << 24] * 4, np.uint32)
    with pytest.raises(RuntimeError, match="query columns do not ascend strictly"):
        gpu_ctx.kmer_topk_match(q, np.array([0, len(q)], np.uint64), 5)
    assert not gpu_ctx.last_error_is_limit()
