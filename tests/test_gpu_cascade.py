"""family_cascade_kernel and its two entry points against the plain loop of tests/cascade_ref.py.

sina_hip_family_cascade (Context.family_cascade): every case of tests/cascade_cases.py, rows equal word for word --
the cases of one rule in one call (lists of different lengths share a launch) and each case alone; every refusal with
the outputs untouched; the counters.

sina_hip_kmer_topk_family (Context.kmer_topk_family) on the hand-built posting-list worlds of tests/kmer_cases.py and
tests/kmer_big_cases.py, against kmer_topk_match + the plain loop: max of 1, 41, the store's size and above 4096,
several launch ranges, a long query among short ones, a repeated candidate-list pass, with and without an identity
limit and self lists."""
import ctypes as C

import numpy as np
import pytest

from sina_amd import capi
from tests import cascade_cases as fc
from tests import cascade_ref as cr
from tests import compare_cases as cc
from tests import kmer_big_cases as kb
from tests import kmer_cases as kc
from tests import util

pytestmark = pytest.mark.gpu

SENTINEL = 0xBEEFBEEF


def _crule(rule):
    return capi.FamilyRule(**rule._asdict())


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    width, refs, _ = fc.store()
    c.upload_refs(cc.flat(refs), cc.offsets(refs), width)
    yield c
    c.close()


def _call(ctx, names):
    """The named cases (of one rule) through one call."""
    cases = [fc.case(n) for n in names]
    rule = cases[0].rule
    assert all(c.rule == rule for c in cases)
    ids = [c.ids for c in cases]
    scores = np.concatenate([c.scores for c in cases] + [np.zeros(0, np.float32)])
    match = None if cases[0].match is None else np.concatenate([c.match for c in cases])
    selfs = None
    if any(c.selfs is not None for c in cases):
        selfs = [c.selfs if c.selfs is not None else np.zeros(0, np.uint32) for c in cases]
    return ctx.family_cascade(cc.flat(ids), scores, match, cc.offsets(ids), [c.query_bases for c in cases], _crule(rule),
                              None if selfs is None else cc.flat(selfs), None if selfs is None else cc.offsets(selfs))


def _same_row(got, want, tag):
    assert got.shape == want.shape, tag
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (tag, "%d words differ, first: word %d got %d want %d; kept %d want %d, flags %d want %d"
                           % (len(bad), bad[0], got[bad[0]], want[bad[0]], got[0], want[0], got[1], want[1]))


@pytest.mark.parametrize("rule_no", range(len(fc.groups())))
def test_cases_of_one_rule_in_one_call(ctx, rule_no):
    rule, names = list(fc.groups().items())[rule_no]
    s0 = ctx.family_stats()
    rows = _call(ctx, names)
    s1 = ctx.family_stats()
    assert rows.shape == (len(names), cr.row_words(rule))
    for row, name in zip(rows, names):
        _same_row(row, fc.expected(name), name)
    assert s1["launches"] - s0["launches"] == 1 and s1["queries"] - s0["queries"] == len(names)
    assert s1["candidates_listed"] - s0["candidates_listed"] == sum(len(fc.case(n).ids) for n in names)
    assert s1["candidates_scanned"] - s0["candidates_scanned"] == sum(fc.scanned(fc.case(n)) for n in names)


@pytest.mark.parametrize("name", fc.NAMES)
def test_case_alone(ctx, name):
    s0 = ctx.family_stats()
    _same_row(_call(ctx, [name])[0], fc.expected(name), name)
    s1 = ctx.family_stats()
    c = fc.case(name)
    assert s1["candidates_scanned"] - s0["candidates_scanned"] == fc.scanned(c) <= len(c.ids) == s1["candidates_listed"] - s0["candidates_listed"]
    if name == "early_exit":
        assert s1["candidates_scanned"] - s0["candidates_scanned"] < s1["candidates_listed"] - s0["candidates_listed"]


def test_stats_move_only_with_the_entry(ctx):
    s0 = ctx.family_stats()
    c = fc.case("len_65")
    ctx.match_counts(np.array([1 | 1 << 24], np.uint32), np.array([0, 1], np.uint64), c.ids[:3], np.array([0, 3], np.uint64))
    assert ctx.family_stats() == s0
    _call(ctx, ["len_65"])
    s1 = ctx.family_stats()
    assert (s1["launches"], s1["queries"]) == (s0["launches"] + 1, s0["queries"] + 1) and s1["kernel_ms"] > s0["kernel_ms"]


# ---------------------------------------------------------------- refusals

def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _raw_cascade(ctx, ids, scores, match, off, qb, nq, rule, self_ids, self_off, out):
    return ctx.L.sina_hip_family_cascade(ctx.h, _p(ids, capi.u32p), _p(scores, capi.f32p), _p(match, capi.u16p), _p(off, capi.u64p),
                                         _p(qb, capi.u32p), nq, None if rule is None else C.byref(rule), _p(self_ids, capi.u32p),
                                         _p(self_off, capi.u64p), _p(out, capi.u32p))


def _raw_topk(ctx, q_ab, q_off, nq, mx, rule, self_ids, self_off, out):
    return ctx.L.sina_hip_kmer_topk_family(ctx.h, _p(q_ab, capi.u32p), _p(q_off, capi.u64p), nq, mx, None if rule is None else C.byref(rule),
                                           _p(self_ids, capi.u32p), _p(self_off, capi.u64p), _p(out, capi.u32p))


def _error(ctx):
    return ctx.L.sina_hip_last_error().decode()


def test_refusals():
    """Every argument check of both entries returns nonzero with its message, before any launch and with the rows
    untouched; the context computes a case correctly afterwards."""
    c = capi.Context(0)
    try:
        width, refs, _ = fc.store()
        case = fc.case("identity_limit")
        rule = _crule(case.rule)
        ids, sc, mt = case.ids.copy(), case.scores.copy(), case.match.copy()
        off, qb = np.array([0, len(ids)], np.uint64), np.array([case.query_bases], np.uint32)
        s_ids, s_off = np.array([3], np.uint32), np.array([0, 1], np.uint64)
        q_ab = (np.arange(12, dtype=np.uint32) * 2) | np.uint32(1 << 24)
        q_off = np.array([0, len(q_ab)], np.uint64)

        def refused(message, raw, *args, limit=False):
            out = np.full(cr.row_words(case.rule) + 8, SENTINEL, np.uint32)
            launches = c.family_stats()["launches"]
            args = list(args)
            has_out = args[-1] is not None
            if has_out:
                args[-1] = out
            assert raw(c, *args) != 0, message
            assert message in _error(c), (message, _error(c))
            assert bool(c.last_error_is_limit()) == limit, message
            assert (out == SENTINEL).all() and c.family_stats()["launches"] == launches

        full = (ids, sc, mt, off, qb, 1, rule, s_ids, s_off, True)
        refused("upload references first", _raw_cascade, *full)
        c.upload_refs(cc.flat(refs), cc.offsets(refs), width)
        c.build_index(4, True)
        for hole in (0, 1, 2, 3, 4, 6, 7, 8, 9):              # every pointer; the match counts because the rule reads them
            args = list(full)
            args[hole] = None
            refused("null argument", _raw_cascade, *args)
        bad = ids.copy()
        bad[-1] = len(refs)
        refused("reference id out of range", _raw_cascade, bad, sc, mt, off, qb, 1, rule, s_ids, s_off, True)
        refused("self id out of range", _raw_cascade, ids, sc, mt, off, qb, 1, rule, np.array([len(refs)], np.uint32), s_off, True)
        over = capi.FamilyRule(fs_min=1000, fs_max=1000, fs_req_full=25, fs_msc_max=0.9)
        refused("more than 1024 entries", _raw_cascade, ids, sc, mt, off, qb, 1, over, s_ids, s_off, True, limit=True)
        # the search entry
        topk = (q_ab, q_off, 1, 5, rule, s_ids, s_off, True)
        for hole in (0, 1, 4, 5, 6, 7):
            args = list(topk)
            args[hole] = None
            refused("null argument", _raw_topk, *args)
        refused("self id out of range", _raw_topk, q_ab, q_off, 1, 5, rule, np.array([len(refs)], np.uint32), s_off, True)
        refused("more than 1024 entries", _raw_topk, q_ab, q_off, 1, 5, over, s_ids, s_off, True, limit=True)
        twice = q_ab.copy()
        twice[5] = twice[4]
        refused("query columns do not ascend strictly", _raw_topk, twice, q_off, 1, 5, rule, s_ids, s_off, True)
        # ... which a rule without an identity limit does not look at; its match counts may be missing too
        free = _crule(case.rule._replace(fs_msc_max=1.0))
        out = np.full(cr.row_words(case.rule), SENTINEL, np.uint32)
        assert _raw_topk(c, twice, q_off, 1, 5, free, None, None, out) == 0, _error(c)
        assert out[0] <= 5 and out[1] <= 3
        assert _raw_cascade(c, ids, sc, None, off, qb, 1, free, None, None, out) == 0, _error(c)
        _same_row(out, cr.row(fc.meta(), ids, sc, None, 10, None, case.rule._replace(fs_msc_max=1.0)), "no counts")
        # nothing to do
        out = np.full(4, SENTINEL, np.uint32)
        assert _raw_cascade(c, ids, sc, mt, off, qb, 0, rule, None, None, out) == 0 and (out == SENTINEL).all()
        # a store wider than the match count's table: a limit for a rule with an identity limit, and only for it
        wide_ref = [cc.seq([0, 9, 327680], [1, 2, 4])]
        c.upload_refs(cc.flat(wide_ref), cc.offsets(wide_ref), 327681)
        c.build_index(4, True)
        z = np.zeros(1, np.uint32)
        one = np.array([0, 1], np.uint64)
        refused("too wide for the device match count", _raw_cascade, z, np.ones(1, np.float32), np.zeros(1, np.uint16), one, qb, 1, rule,
                None, None, True, limit=True)
        refused("too wide for the device match count", _raw_topk, q_ab, q_off, 1, 5, rule, None, None, True, limit=True)
        got = c.family_cascade(z, np.ones(1, np.float32), None, one, qb, free)
        _same_row(got[0], cr.row(cr.meta_of(wide_ref), z, np.ones(1, np.float32), None, 10, None, case.rule._replace(fs_msc_max=1.0)), "wide")
        # the context still computes
        c.upload_refs(cc.flat(refs), cc.offsets(refs), width)
        _same_row(_call(c, ["identity_limit"])[0], fc.expected("identity_limit"), "after")
    finally:
        c.close()


# ---------------------------------------------------------------- sina_hip_kmer_topk_family

WORLD_WIDTH = 48


def _world_refs(n_refs):
    """n_refs references of one to three bases inside WORLD_WIDTH columns; every seventh starts in column 0."""
    i = np.arange(n_refs, dtype=np.int64)
    cols = np.stack([i % 7, 8 + i % 11, 20 + (i * 7) % 23], axis=1)
    masks = np.stack([1 << (i % 4), 1 << ((i // 4) % 4), np.where(i % 5 == 0, 15, 1 << ((i // 16) % 4))], axis=1)
    refs = [(cols[x, :1 + x % 3] | (masks[x, :1 + x % 3] << 24)).astype(np.uint32) for x in range(n_refs)]
    return refs


RULES = (cr.Rule(fs_min=5, fs_max=8, fs_req_full=2, fs_full_len=3, fs_min_len=2, fs_cover_gene=2, fs_msc=2.5, fs_msc_max=0.03),
         cr.Rule(fs_min=3, fs_max=40, fs_req_full=1, fs_full_len=3, fs_min_len=0, fs_cover_gene=0, fs_msc=1000.0, fs_msc_max=2.0))


def _topk_family(ctx, refs, qmasks, mx, tag, stride=1):
    """Both rules, with self lists (the best candidate of every other query, and a reference that is no candidate) and
    without, against kmer_topk_match + the plain loop.  Returns the cascade launches of the first call."""
    qs = [(np.arange(len(m), dtype=np.uint32) * stride) | (m.astype(np.uint32) << 24) for m in qmasks]
    q_ab, q_off = cc.flat(qs), cc.offsets(qs)
    gi, gs, gn, gm = ctx.kmer_topk_match(q_ab, q_off, mx)
    meta = cr.meta_of(refs)
    selfs = [np.array([gi[qi, 0], len(refs) - 1] if qi % 2 == 0 and gn[qi] else [], np.uint32) for qi in range(len(qs))]
    first = None
    for rule in RULES:
        for with_self in (True, False):
            s0, m0 = ctx.family_stats(), ctx.match_stats()
            rows = ctx.kmer_topk_family(q_ab, q_off, mx, _crule(rule), cc.flat(selfs) if with_self else None,
                                        cc.offsets(selfs) if with_self else None)
            s1, m1 = ctx.family_stats(), ctx.match_stats()
            for qi, q in enumerate(qs):
                n = int(gn[qi])
                want = cr.row(meta, gi[qi, :n], gs[qi, :n], gm[qi, :n] if rule.fs_msc_max < 1 else None, len(q),
                              selfs[qi] if with_self else None, rule)
                _same_row(rows[qi], want, (tag, mx, rule, with_self, "query %d" % qi))
            launches = s1["launches"] - s0["launches"]
            assert s1["queries"] - s0["queries"] == len(qs) and s1["candidates_listed"] - s0["candidates_listed"] == int(gn.sum())
            assert m1["launches"] - m0["launches"] == (launches if rule.fs_msc_max < 1 else 0)      # no limit: no match count
            first = launches if first is None else first
            assert launches == first
    return first


def _open(c, monkeypatch):
    ctx = capi.Context(0)
    refs = _world_refs(c.n_refs)
    ctx.upload_refs(cc.flat(refs), cc.offsets(refs), WORLD_WIDTH)
    util.set_knobs(monkeypatch, dense_div=None, kmer_rows=None, big_sel_bytes=None)
    ctx.upload_index(c.k, c.nofast, c.off, c.ids)
    return ctx, refs


def test_topk_family_maxes_and_launch_ranges(monkeypatch):
    """The mixed batch of kmer_big_cases: max 1, 41, above 4096 (the big select), the store's size and beyond; then
    4500 under a budget that cuts the queries into several launch ranges -- one cascade launch per range."""
    c = kb.mixed_batch()
    ctx, refs = _open(c, monkeypatch)
    try:
        big0 = ctx.big_select_queries()
        for mx in (1, 41, 4097, c.n_refs, c.n_refs + 10):
            assert _topk_family(ctx, refs, c.qmasks, mx, c.name) == 1
        assert ctx.big_select_queries() > big0
        assert _topk_family(ctx, refs, c.qmasks, 41, (c.name, "stride 2"), stride=2) == 1
        seam, (budget, ranges) = sorted(kb.seam_budgets().items())[0]
        util.set_knobs(monkeypatch, big_sel_bytes=budget)
        assert _topk_family(ctx, refs, c.qmasks, kb.MIXED_M, (c.name, seam)) == len(ranges) > 1
    finally:
        ctx.close()


def test_topk_family_long_query_among_short_ones(monkeypatch):
    """A query above 10 240 bases between short ones: its range runs behind the others, the rows and the self lists
    come back in the caller's order."""
    c = kb.long_query()
    qmasks = [c.qmasks[0], c.qmasks[2], kc.poly("A", 50), c.qmasks[1], kc.poly("C", 30)]
    assert [len(m) > kc.FAST_MAX for m in qmasks] == [False, True, False, True, False]
    ctx, refs = _open(c, monkeypatch)
    try:
        long0 = ctx.long_queries()
        assert _topk_family(ctx, refs, qmasks, 41, c.name) == 2          # the fast range and the long one
        assert ctx.long_queries() > long0
    finally:
        ctx.close()


def test_topk_family_after_a_candidate_list_overflow(monkeypatch):
    """cap_4097: the first pass's candidate list overflows and launches no cascade; its repeat does."""
    c = kc.cap(4097)
    ctx, refs = _open(c, monkeypatch)
    try:
        l0 = ctx.stats()["kmer_launches"]
        assert _topk_family(ctx, refs, c.qmasks, 41, c.name) == 1
        assert ctx.stats()["kmer_launches"] - l0 == 2 * (1 + 2 * len(RULES))      # (two passes per search call)
    finally:
        ctx.close()
