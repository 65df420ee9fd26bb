"""rank_kernel, rank_merge_kernel and their entry points against tests/rank_ref.py: ids and score BITS of the max_result
best of every query, the counts and the flags, on the directed cases of tests/rank_cases.py (list lengths, ties decided
by the name, zero scores, scores above one, candidates without a score, duplicated ids, forced chunks, every reference
without an id list) and on tests/compare_cases.py's worlds under every rule; sina_hip_kmer_topk_rank against
sina_hip_kmer_topk_any followed by sina_hip_compare_rank (also with long queries among short ones, which the driver
puts last, and after a candidate-list overflow); then every refusal.  tests/test_rank_cpu.py pins rank_ref to
the host stage and to the reference, and checks that every case reaches its edge."""
import contextlib
import os

import numpy as np
import pytest

from sina_amd import capi, synth
from tests import compare_cases as cc
from tests import kmer_big_cases as kb
from tests import kmer_cases as kc
from tests import rank_cases as rc
from tests import rank_ref
from tests import util
from tests.test_gpu_msc import WORLD_WIDTH, _packed_queries, _world_refs

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _chunk_knob(chunk):
    old = os.environ.get("SINA_HIP_TEST")
    if chunk:
        os.environ["SINA_HIP_TEST"] = "rank_chunk=%d" % chunk
    try:
        yield
    finally:
        if chunk:
            if old is None:
                del os.environ["SINA_HIP_TEST"]
            else:
                os.environ["SINA_HIP_TEST"] = old


def _upload(ctx, width, refs, names):
    ctx.upload_refs(cc.flat(refs), cc.offsets(refs), width)
    ctx.upload_name_order(rank_ref.name_order(names))


def _check(got, want, tag):
    """Flags and counts everywhere; ids and score bits of every query that is not flagged (a flagged query's rows are
    unspecified)."""
    ids, sc, n, flag = got
    w_ids, w_bits, w_n, w_flag = want
    assert (flag == w_flag).all(), (tag, "flags", flag.tolist(), w_flag.tolist())
    bits = sc.view(np.uint32)
    for q in np.flatnonzero(w_flag == 0):
        assert n[q] == w_n[q], (tag, "query %d" % q, int(n[q]), int(w_n[q]))
        k = int(n[q])
        assert (ids[q, :k] == w_ids[q, :k]).all(), (tag, "query %d ids" % q, ids[q, :k].tolist(), w_ids[q, :k].tolist())
        assert (bits[q, :k] == w_bits[q, :k]).all(), (tag, "query %d score bits" % q, sc[q, :k].tolist())


def _launch(ctx, case):
    cand = case["cand"]
    with _chunk_knob(case["chunk"]):
        return ctx.compare_rank(cc.flat(case["qs"]), cc.offsets(case["qs"]), None if cand is None else cc.flat(cand),
                                None if cand is None else cc.offsets(cand), case["rule"], case["flc"], case["cover"],
                                case["n_best"])


@pytest.mark.parametrize("name", rc.NAMES)
def test_rank_directed(gpu_ctx, name):
    case = rc.case(name)
    want = rc.expected(name)
    _upload(gpu_ctx, case["width"], case["refs"], case["names"])
    before = gpu_ctx.rank_stats()
    got = _launch(gpu_ctx, case)
    _check(got, want, name)
    assert int(got[3].sum()) == case["flagged"]
    # the kernel's own counters: every pair scored once, every base of its candidate counted, one launch (two with a merge)
    lists = rc.lists_of(case)
    after = gpu_ctx.rank_stats()
    assert after["pairs"] - before["pairs"] == sum(len(x) for x in lists)
    assert after["cand_bases"] - before["cand_bases"] == sum(len(case["refs"][int(i)]) for x in lists for i in x)
    chunks = rc.plan(len(lists), max(len(x) for x in lists), 256, forced=case["chunk"] or 0)[1]    # (256 compute units)
    assert not case["chunk"] or chunks > 1
    assert after["launches"] - before["launches"] == (2 if chunks > 1 else 1)


def test_rank_identity_order_is_id_descending(gpu_ctx):
    """The identity permutation as name order: equal scores by id descending, sina_hip_kmer_topk's own tie rule."""
    case = rc.case("ties")
    gpu_ctx.upload_refs(cc.flat(case["refs"]), cc.offsets(case["refs"]), case["width"])
    gpu_ctx.upload_name_order(np.arange(len(case["refs"]), dtype=np.uint32))
    ids, sc, n, flag = _launch(gpu_ctx, case)
    tied = [i for i in range(20) if i not in (0, 3, 7, 11, 15, 19)]
    assert list(ids[0]) == [0, 3, 11] + sorted(tied, reverse=True)[:7]


@pytest.mark.parametrize("world", rc.CC_WORLDS)
def test_rank_compare_worlds_all_settings(gpu_ctx, world):
    """Three IUPAC rules x the lower-case filter x nine cover rules on compare_cases' worlds (on the widest ones: every
    cover rule under two settings), counters by the plain walk."""
    width, refs, qs, cand = cc.case(world)
    _upload(gpu_ctx, width, refs, rc._names(len(refs)))
    q_ab, q_off, c_ids, c_off = cc.flat(qs), cc.offsets(qs), cc.flat(cand), cc.offsets(cand)
    settings = cc.SETTINGS if width <= 3000 else [(0, False), (1, True)]
    for rule, flc in settings:
        for cover in range(9):
            n_best = (3, 1, 10)[cover % 3]
            got = gpu_ctx.compare_rank(q_ab, q_off, c_ids, c_off, rule, flc, cover, n_best)
            _check(got, rc.cc_expected(world, cover, rule, flc, n_best), (world, rule, flc, rank_ref.COVERS[cover]))


def test_rank_subrange_of_larger_arrays(gpu_ctx):
    """q_off[0] != 0 and cand_off[0] != 0: queries 3 .. 7 of `cand_lists` addressed inside the full arrays."""
    width, refs, qs, cand = cc.case("cand_lists")
    _upload(gpu_ctx, width, refs, rc._names(len(refs)))
    q_ab, q_off, c_ids, c_off = cc.flat(qs), cc.offsets(qs), cc.flat(cand), cc.offsets(cand)
    lo, hi = 3, 8
    assert q_off[lo] != 0 and c_off[lo] != 0
    want = rc.cc_expected("cand_lists", 4, 2, True, 3)
    ids = np.full((hi - lo + 1, 3), 77, np.uint32)
    sc = np.full((hi - lo + 1, 3), 7.0, np.float32)
    n = np.full(hi - lo + 1, 77, np.uint32)
    flag = np.full(hi - lo + 1, 77, np.uint32)
    rc_ = gpu_ctx.L.sina_hip_compare_rank(gpu_ctx.h, q_ab.ctypes.data_as(capi.u32p), q_off[lo:].ctypes.data_as(capi.u64p), hi - lo,
                                          c_ids.ctypes.data_as(capi.u32p), c_off[lo:].ctypes.data_as(capi.u64p), 2, 1, 4, 3,
                                          ids.ctypes.data_as(capi.u32p), sc.ctypes.data_as(capi.f32p),
                                          n.ctypes.data_as(capi.u32p), flag.ctypes.data_as(capi.u32p))
    assert rc_ == 0, gpu_ctx.L.sina_hip_last_error().decode()
    _check((ids[:-1], sc[:-1], n[:-1], flag[:-1]), tuple(x[lo:hi] for x in want), "sub-range")
    assert (ids[-1] == 77).all() and (sc[-1] == 7.0).all() and n[-1] == 77 and flag[-1] == 77    # nothing past them


def test_kmer_topk_rank_equals_topk_then_compare_rank(gpu_ctx):
    """On a 300-reference world: the fused entry gives what sina_hip_kmer_topk_any's candidates give when handed to
    sina_hip_compare_rank as lists -- with fewer candidates than references (a real selection), with more, with the
    launch cut into chunks, and for two sets of rules."""
    refs = synth.make_refs(300, length=300, width=3000, seed=661, amb_rate=0.01, lower_rate=0.03)
    names = ["ref%d" % i for i in range(refs.n)]
    gpu_ctx.upload_refs(refs.ab, refs.off, refs.width)
    gpu_ctx.build_index(10, False)
    gpu_ctx.upload_name_order(rank_ref.name_order(names))
    rng = np.random.default_rng(662)
    qs = []
    for i in range(9):
        ab = refs.seq(int(rng.integers(refs.n))).copy()
        a, b = (0, len(ab)) if i % 3 else (20, 220)
        ab = ab[a:b]
        m = (ab >> 24).astype(np.uint32)
        sub = rng.random(len(ab)) < 0.05
        m[sub] = rng.choice([1, 2, 4, 8], size=int(sub.sum()))
        qs.append(((ab & 0xFFFFFF) | (m << 24)).astype(np.uint32))
    q_ab, q_off = cc.flat(qs), cc.offsets(qs)
    mask = (q_ab >> 24).astype(np.uint8)
    for kmer_candidates, chunk, rule, flc, cover, n_best in ((40, None, 0, False, "query", 10), (1000, None, 1, True, "all", 64),
                                                             (40, 7, 2, False, "min", 5)):
        ids, _, n = gpu_ctx.kmer_topk_any(mask, q_off, kmer_candidates)
        assert (n == min(kmer_candidates, refs.n)).all()
        cand = [ids[q, :n[q]] for q in range(len(qs))]
        with _chunk_knob(chunk):
            two_step = gpu_ctx.compare_rank(q_ab, q_off, cc.flat(cand), cc.offsets(cand), rule, flc, cover, n_best)
            before = gpu_ctx.rank_stats()
            fused = gpu_ctx.kmer_topk_rank(q_ab, q_off, kmer_candidates, rule, flc, cover, n_best)
            after = gpu_ctx.rank_stats()
        assert (two_step[3] == 0).all() and (two_step[2] == min(n_best, kmer_candidates, refs.n)).all()
        for a, b in zip(fused, two_step):
            assert a.tobytes() == b.tobytes()
        chunks = rc.plan(len(qs), min(kmer_candidates, refs.n), 256, forced=chunk or 0)[1]
        assert after["pairs"] - before["pairs"] == int(n.sum()) and after["launches"] - before["launches"] == (2 if chunks > 1 else 1)


def _fused_equals_two_step(ctx, qmasks, kmer_candidates):
    """kmer_topk_rank on the k-mer cases' mask bytes as aligned queries (base i in column i) against kmer_topk_any
    followed by compare_rank on its lists, byte for byte; gives the lengths of the lists and by how much the fused call
    moved the k-mer launches and the rank kernel's counters."""
    qs = _packed_queries(qmasks, 1)
    q_ab, q_off = cc.flat(qs), cc.offsets(qs)
    ids, _, n = ctx.kmer_topk_any(np.concatenate(qmasks), q_off, kmer_candidates)
    cand = [ids[q, :n[q]] for q in range(len(qs))]
    two_step = ctx.compare_rank(q_ab, q_off, cc.flat(cand), cc.offsets(cand), 0, False, "query", 10)
    l0, before = ctx.stats()["kmer_launches"], ctx.rank_stats()
    fused = ctx.kmer_topk_rank(q_ab, q_off, kmer_candidates, 0, False, "query", 10)
    l1, after = ctx.stats()["kmer_launches"], ctx.rank_stats()
    for a, b in zip(fused, two_step):
        assert a.tobytes() == b.tobytes(), kmer_candidates
    return n, l1 - l0, {k: after[k] - before[k] for k in ("pairs", "launches")}


def _kmer_world(ctx, c, width, monkeypatch):
    """The case's hand-built index over the three-base references of tests/test_gpu_msc.py, in an alignment of `width`
    columns, names in id order."""
    ab, off, _, _ = _world_refs(c.n_refs)
    ctx.upload_refs(ab, off, width)
    util.set_knobs(monkeypatch, dense_div=None, kmer_rows=None, big_sel_bytes=None)
    ctx.upload_index(c.k, c.nofast, c.off, c.ids)
    ctx.upload_name_order(np.arange(c.n_refs, dtype=np.uint32))


def test_kmer_topk_rank_long_query_among_short_ones(monkeypatch):
    """Queries above 10 240 bases between short ones: the long count kernel's range runs behind the others and is
    ranked in a launch of its own; ids, scores, counts and flags come back in the caller's order."""
    c = kb.long_query()
    qmasks = [c.qmasks[0], c.qmasks[2], kc.poly("A", 50), c.qmasks[1], kc.poly("C", 30)]
    assert [len(m) > kc.FAST_MAX for m in qmasks] == [False, True, False, True, False]
    width = max(len(m) for m in qmasks)                 # every query column inside the alignment
    assert width > WORLD_WIDTH and 6 * (width // 32) + width < 150 * 1024
    ctx = capi.Context(0)
    try:
        _kmer_world(ctx, c, width, monkeypatch)
        long0 = ctx.long_queries()
        n, _, moved = _fused_equals_two_step(ctx, qmasks, 41)
        assert (n == 41).all()
        assert ctx.long_queries() - long0 == 2 * 2      # (two search calls, two long queries)
        assert moved["launches"] == 2                    # the fast range and the long one
    finally:
        ctx.close()


def test_kmer_topk_rank_after_a_candidate_list_overflow(monkeypatch):
    """cap_4097: the candidate list of the first pass overflows and the range is repeated with the score rows; the
    overflowed pass ranks nothing, the rows ranked are those of the final select.  cap_4096: the list just fits."""
    c = kc.cap(4097)
    ctx = capi.Context(0)
    try:
        _kmer_world(ctx, c, max(WORLD_WIDTH, max(len(m) for m in c.qmasks)), monkeypatch)
        for kmer_candidates in (41, 128):
            n, kmer_launches, moved = _fused_equals_two_step(ctx, c.qmasks, kmer_candidates)
            assert kmer_launches == 2                    # the overflowed pass and its repeat
            assert moved == {"launches": 1, "pairs": int(n.sum())}
        c1 = kc.cap(4096)
        assert c1.n_refs == c.n_refs and [len(m) for m in c1.qmasks] == [len(m) for m in c.qmasks]
        ctx.upload_index(c1.k, c1.nofast, c1.off, c1.ids)
        n, kmer_launches, moved = _fused_equals_two_step(ctx, c1.qmasks, 41)
        assert kmer_launches == 1 and moved == {"launches": 1, "pairs": int(n.sum())}
    finally:
        ctx.close()


def test_kmer_topk_rank_refuses_more_than_the_lds_select_sorts():
    """min(kmer_candidates, n_refs) above 4096 is refused as a limit, outputs untouched; 4096 is taken."""
    refs = synth.make_refs(4200, length=100, width=1000, seed=671)
    ctx = capi.Context(0)
    try:
        ctx.upload_refs(refs.ab, refs.off, refs.width)
        ctx.build_index(10, False)
        ctx.upload_name_order(np.arange(refs.n, dtype=np.uint32))
        q_ab = np.ascontiguousarray(refs.seq(17), np.uint32)
        q_off = np.array([0, len(q_ab)], np.uint64)
        outs = _outs(1, 10)
        p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
        rc_ = ctx.L.sina_hip_kmer_topk_rank(ctx.h, p(q_ab, capi.u32p), p(q_off, capi.u64p), 1, 5000, 0, 0, 1, 10, p(outs[0], capi.u32p),
                                            p(outs[1], capi.f32p), p(outs[2], capi.u32p), p(outs[3], capi.u32p))
        assert rc_ != 0 and ctx.last_error_is_limit() and "more than 4096 candidates" in ctx.L.sina_hip_last_error().decode()
        assert _untouched(outs)
        ids, sc, n, flag = ctx.kmer_topk_rank(q_ab, q_off, 4096, 0, False, "abs", 10)      # (abs: the match count itself)
        assert n[0] == 10 and flag[0] == 0 and ids[0, 0] == 17 and sc[0, 0] == len(q_ab)
    finally:
        ctx.close()


# ---------------------------------------------------------------- refusals

SENT = 0x5A5A5A5A


def _raw(ctx, q_ab, q_off, nq, c_ids, c_off, rule, flc, cover, n_best, outs):
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    return ctx.L.sina_hip_compare_rank(ctx.h, p(q_ab, capi.u32p), p(q_off, capi.u64p), nq, p(c_ids, capi.u32p), p(c_off, capi.u64p),
                                       rule, int(flc), cover, n_best, p(outs[0], capi.u32p), p(outs[1], capi.f32p),
                                       p(outs[2], capi.u32p), p(outs[3], capi.u32p))


def _outs(nq, rows=64):
    return [np.full((nq, rows), SENT, np.uint32), np.full((nq, rows), 3.5, np.float32), np.full(nq, SENT, np.uint32),
            np.full(nq, SENT, np.uint32)]


def _untouched(outs):
    return all(o is None or (o == (3.5 if o.dtype == np.float32 else SENT)).all() for o in outs)


def _refused(ctx, message, *args, outs=None, limit=False):
    outs = _outs(8) if outs is None else outs
    assert _raw(ctx, *args, outs) != 0, message
    err = ctx.L.sina_hip_last_error().decode()
    assert message in err, (message, err)
    assert ctx.last_error_is_limit() == limit and _untouched(outs)


def test_rank_refusals():
    """Every argument check of the ranking entries returns nonzero with its message, before any launch and with the
    outputs untouched, and the context ranks a small case correctly afterwards."""
    ctx = capi.Context(0)
    try:
        case = rc.case("nan_overlap")
        refs, qs, cand = case["refs"], case["qs"], case["cand"]
        q_ab, q_off, c_ids, c_off = cc.flat(qs), cc.offsets(qs), cc.flat(cand), cc.offsets(cand)
        nq = len(qs)
        good = (q_ab, q_off, nq, c_ids, c_off, 0, 0, 1, 3)
        _refused(ctx, "upload references first", *good)
        ctx.upload_refs(cc.flat(refs), cc.offsets(refs), case["width"])
        _refused(ctx, "upload the name order first", *good)
        # the name order itself: a permutation of 0 .. n_refs - 1, from the context that owns the store
        n_refs = len(refs)
        for bad, msg in ((np.arange(n_refs - 1, dtype=np.uint32), "one rank per reference"),
                         (np.array([0, 1, 2, 3, 4, 4], np.uint32), "not a permutation"),
                         (np.array([0, 1, 2, 3, 4, 6], np.uint32), "not a permutation")):
            assert ctx.L.sina_hip_upload_name_order(ctx.h, bad.ctypes.data_as(capi.u32p), len(bad)) != 0
            assert msg in ctx.L.sina_hip_last_error().decode()
        _refused(ctx, "upload the name order first", *good)
        fork = ctx.fork()
        order = rank_ref.name_order(case["names"])
        assert fork.L.sina_hip_upload_name_order(fork.h, order.ctypes.data_as(capi.u32p), n_refs) != 0
        assert "forked context" in fork.L.sina_hip_last_error().decode()
        fork.close()
        ctx.upload_name_order(order)
        _check(_launch(ctx, case), rc.expected("nan_overlap"), "after the order")
        # upload_refs forgets the order
        ctx.upload_refs(cc.flat(refs), cc.offsets(refs), case["width"])
        _refused(ctx, "upload the name order first", *good)
        ctx.upload_name_order(order)
        # null pointers
        for k in (0, 1):
            a = list(good)
            a[k] = None
            _refused(ctx, "null argument", *a)
        _refused(ctx, "null argument", q_ab, q_off, nq, c_ids, None, 0, 0, 1, 3)
        for k in range(4):
            outs = _outs(8)
            outs[k] = None
            _refused(ctx, "null argument", *good, outs=outs)
        # rules and the number of rows
        _refused(ctx, "unknown iupac rule", q_ab, q_off, nq, c_ids, c_off, 3, 0, 1, 3)
        _refused(ctx, "unknown iupac rule", q_ab, q_off, nq, c_ids, c_off, -1, 0, 1, 3)
        _refused(ctx, "unknown cover rule", q_ab, q_off, nq, c_ids, c_off, 0, 0, 9, 3)
        _refused(ctx, "unknown cover rule", q_ab, q_off, nq, c_ids, c_off, 0, 0, -1, 3)
        _refused(ctx, "max_result outside 1..64", q_ab, q_off, nq, c_ids, c_off, 0, 0, 1, 0)
        _refused(ctx, "max_result outside 1..64", q_ab, q_off, nq, c_ids, c_off, 0, 0, 1, 65, outs=_outs(8, 65))
        # an id one past the store
        ids = c_ids.copy()
        ids[-1] = n_refs
        _refused(ctx, "reference id out of range", q_ab, q_off, nq, ids, c_off, 0, 0, 1, 3)
        # columns that do not ascend strictly; a query of 65536 bases
        twice = q_ab.copy()
        twice[1] = twice[0]
        _refused(ctx, "do not ascend strictly", twice, q_off, nq, c_ids, c_off, 0, 0, 1, 3)
        long_q = cc.seq(range(65536))
        _refused(ctx, "query longer than 65535 bases", long_q, np.array([0, 65536], np.uint64), 1, np.zeros(1, np.uint32),
                 np.array([0, 1], np.uint64), 0, 0, 1, 3)
        _refused(ctx, "query longer than 65535 bases", long_q, np.array([0, 65536], np.uint64), 1, None, None, 0, 0, 1, 3)
        # the fused entry checks the same before it searches
        outs = _outs(8)
        p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
        assert ctx.L.sina_hip_kmer_topk_rank(ctx.h, p(q_ab, capi.u32p), p(q_off, capi.u64p), nq, 40, 0, 0, 9, 3, p(outs[0], capi.u32p),
                                             p(outs[1], capi.f32p), p(outs[2], capi.u32p), p(outs[3], capi.u32p)) != 0
        assert _untouched(outs)
        # nothing to do: no query; only empty lists (counts and flags are zero)
        outs = _outs(8)
        assert _raw(ctx, q_ab, q_off, 0, c_ids, c_off, 0, 0, 1, 3, outs) == 0 and _untouched(outs)
        outs = _outs(3, 3)
        assert _raw(ctx, q_ab, q_off, 3, c_ids, np.zeros(4, np.uint64), 0, 0, 1, 3, outs) == 0
        assert (outs[2] == 0).all() and (outs[3] == 0).all()
        _check(_launch(ctx, case), rc.expected("nan_overlap"), "after the refusals")
        # the limit, by width: refused before any launch, as a limit
        wide = 32 * 40000
        assert 6 * (wide // 32) > 150 * 1024
        ctx.upload_refs(cc.flat(refs), cc.offsets(refs), wide)
        ctx.upload_name_order(order)
        _refused(ctx, "too wide for the device comparison", *good, limit=True)
        _refused(ctx, "too wide for the device comparison", q_ab, q_off, nq, None, None, 0, 0, 1, 3, limit=True)
        ctx.upload_refs(cc.flat(refs), cc.offsets(refs), case["width"])
        ctx.upload_name_order(order)
        _check(_launch(ctx, case), rc.expected("nan_overlap"), "after the limit")
    finally:
        ctx.close()


def test_rank_prewarm_covers_the_new_scratch():
    """sina_hip_prewarm(ctx, 2) on a fresh fork after a chunked launch: the fork then ranks the same call without
    growing a buffer (its capacities are already the hinted ones; observable as equal results and no error -- the
    allocation trace is SINA_HIP_TRACE_ALLOC's)."""
    ctx = capi.Context(0)
    try:
        case = rc.case("all_refs_13")
        _upload(ctx, case["width"], case["refs"], case["names"])
        _check(_launch(ctx, case), rc.expected("all_refs_13"), "root")
        fork = ctx.fork()
        assert fork.L.sina_hip_prewarm(fork.h, 2) == 0
        _check(_launch(fork, case), rc.expected("all_refs_13"), "fork")
        fork.close()
    finally:
        ctx.close()
