"""compare_kernel and its entry point against a plain walk: the six counters of every (query, candidate) pair of the named
cases and fuzz seeds of tests/compare_cases.py equal tests/compare_ref.py's lock-step walk, integer for integer, under
three IUPAC rules x two filter settings (tests/test_compare_cpu.py pins that walk to the oracle's traverse() and to the
host's counters, and asserts that every case reaches its edge).  Then the entry point itself: sub-ranges of larger
offset arrays, scratch buffers reused across launch sizes and stores, and every refusal."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from sina_amd import capi
from tests import compare_cases as cc

pytestmark = pytest.mark.gpu


def _upload(ctx, width, refs):
    ctx.upload_refs(cc.flat(refs), cc.offsets(refs), width)


def _launch(ctx, qs, cand, rule, flc):
    return ctx.compare(cc.flat(qs), cc.offsets(qs), cc.flat(cand), cc.offsets(cand), rule, flc)


def _equal(got, want, cand, tag):
    assert got.shape == want.shape, tag
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad):
        at = int(bad[0])
        qi = int(np.searchsorted(cc.offsets(cand), at, side="right")) - 1
        raise AssertionError(tag + ("%d of %d pairs differ, first: pair %d (query %d, reference %d)"
                                    % (len(bad), len(want), at, qi, int(cc.flat(cand)[at])),
                                    "got", got[at].tolist(), "want", want[at].tolist()))


def _run_case(ctx, name, settings=cc.SETTINGS, upload=True):
    width, refs, qs, cand = cc.case(name)
    exp = cc.expected(name)
    if upload:
        _upload(ctx, width, refs)
    for rule, flc in settings:
        _equal(_launch(ctx, qs, cand, rule, flc), exp[rule, flc], cand, (name, "rule %d" % rule, "filter_lc %d" % flc))


@pytest.mark.parametrize("name", cc.NAMES)
def test_compare_matrix(oracle, gpu_ctx, name):
    """Every named case; compare_cases' builders say which edge each one holds."""
    cc.expected(name)                      # (the plain walk's share of the time is not the launch's)
    t0 = time.perf_counter()
    _run_case(gpu_ctx, name)
    print("%s: upload + 6 launches %.3f s" % (name, time.perf_counter() - t0))


@pytest.mark.parametrize("seed", range(int(os.environ.get("SINA_FUZZ_SEEDS", "12"))))
def test_compare_fuzz(oracle, gpu_ctx, seed):
    """Seeded random widths, densities, ambiguity and lower-case rates, windows, shifted columns and list sizes; every
    pair is compared, and the seed must reach every counter and a side without a remaining base."""
    width, refs, qs, cand = cc.fuzz_case(seed)
    cc.fuzz_coverage(seed)
    exp = cc.expected("fuzz", seed)
    _upload(gpu_ctx, width, refs)
    for rule, flc in cc.SETTINGS:
        _equal(_launch(gpu_ctx, qs, cand, rule, flc), exp[rule, flc], cand, ("seed %d" % seed, rule, flc))


# ---------------------------------------------------------------- the entry point

SENTINEL = -7


def _raw(ctx, q_ab, q_off, nq, cand_ids, cand_off, rule, flc, out):
    """sina_hip_compare as a foreign host calls it: any argument may be None, offsets may be views into larger arrays."""
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    return ctx.L.sina_hip_compare(ctx.h, p(q_ab, capi.u32p), p(q_off, capi.u64p), nq, p(cand_ids, capi.u32p),
                                  p(cand_off, capi.u64p), rule, int(flc), p(out, C.c_void_p))


def _error(ctx):
    return ctx.L.sina_hip_last_error().decode()


def test_compare_subrange_of_larger_arrays(oracle, gpu_ctx):
    """q_off[0] != 0 and cand_off[0] != 0: queries 3 .. 7 of `cand_lists` addressed inside the full arrays give the rows
    of the same queries passed alone, from out[0] on, and nothing is written past them."""
    width, refs, qs, cand = cc.case("cand_lists")
    q_ab, q_off, c_ids, c_off = cc.flat(qs), cc.offsets(qs), cc.flat(cand), cc.offsets(cand)
    lo, hi = 3, 8
    assert q_off[lo] != 0 and c_off[lo] != 0 and c_off[hi] < c_off[-1]
    n = int(c_off[hi] - c_off[lo])
    _upload(gpu_ctx, width, refs)
    for rule, flc in cc.SETTINGS:
        want = cc.expected("cand_lists")[rule, flc][int(c_off[lo]):int(c_off[hi])]
        out = np.full((n + 4, 6), SENTINEL, np.int32)
        rc = _raw(gpu_ctx, q_ab, q_off[lo:], hi - lo, c_ids, c_off[lo:], rule, flc, out)
        assert rc == 0, _error(gpu_ctx)
        _equal(out[:n], want, cand[lo:hi], ("sub-range", rule, flc))
        assert (out[n:] == SENTINEL).all()
        alone = _launch(gpu_ctx, qs[lo:hi], cand[lo:hi], rule, flc)
        _equal(alone, want, cand[lo:hi], ("alone", rule, flc))


def test_compare_reuses_its_buffers(oracle):
    """One context: a large launch, a small one, the large one again; then another store of another width."""
    ctx = capi.Context(0)
    try:
        width, refs, qs, cand = cc.case("lengths")
        exp = cc.expected("lengths")
        _upload(ctx, width, refs)
        small_q, small_c = qs[:1], [cand[0][:1]]
        assert len(cc.flat(small_q)) == 1 and len(cc.flat(qs)) > 1000
        for rule, flc in ((0, True), (2, False)):
            _equal(_launch(ctx, qs, cand, rule, flc), exp[rule, flc], cand, ("large", rule, flc))
            _equal(_launch(ctx, small_q, small_c, rule, flc), exp[rule, flc][:1], small_c, ("small", rule, flc))
            _equal(_launch(ctx, qs, cand, rule, flc), exp[rule, flc], cand, ("large again", rule, flc))
        assert cc.case("ranges")[0] != width and cc.case("nwords_257")[0] > width
        _run_case(ctx, "ranges")               # a second upload_refs: narrower, fewer bases
        _run_case(ctx, "nwords_257")           # a third: wider
        _run_case(ctx, "lengths", settings=[(1, True)])
    finally:
        ctx.close()


def _refused(ctx, message, *args):
    out = np.full((8, 6), SENTINEL, np.int32) if args[-1] is Ellipsis else args[-1]
    rc = _raw(ctx, *args[:-1], out)
    assert rc != 0, message
    assert message in _error(ctx), (message, _error(ctx))
    assert out is None or (out == SENTINEL).all()
    # the context goes on working
    _run_case(ctx, "ranges", settings=[(0, True), (2, False)], upload=ctx.n_refs != len(cc.case("ranges")[1]))


def test_compare_refusals(oracle):
    """Every argument check of sina_hip_compare returns nonzero with its message, before any launch, and the context
    computes a small case correctly afterwards."""
    ctx = capi.Context(0)
    try:
        width, refs, qs, cand = cc.case("ranges")
        q_ab, q_off, c_ids, c_off = cc.flat(qs), cc.offsets(qs), cc.flat(cand), cc.offsets(cand)
        nq = len(qs)
        out = np.full((len(c_ids), 6), SENTINEL, np.int32)
        assert _raw(ctx, q_ab, q_off, nq, c_ids, c_off, 0, 0, out) != 0
        assert "upload references first" in _error(ctx) and (out == SENTINEL).all()
        _run_case(ctx, "ranges", settings=[(0, True)])
        # null pointers
        _refused(ctx, "null argument", None, q_off, nq, c_ids, c_off, 0, 0, ...)
        _refused(ctx, "null argument", q_ab, None, nq, c_ids, c_off, 0, 0, ...)
        _refused(ctx, "null argument", q_ab, q_off, nq, c_ids, None, 0, 0, ...)
        _refused(ctx, "null argument", q_ab, q_off, nq, c_ids, c_off, 0, 0, None)
        _refused(ctx, "null candidate ids", q_ab, q_off, nq, None, c_off, 0, 0, ...)
        # rules
        _refused(ctx, "unknown iupac rule", q_ab, q_off, nq, c_ids, c_off, -1, 0, ...)
        _refused(ctx, "unknown iupac rule", q_ab, q_off, nq, c_ids, c_off, 3, 0, ...)
        # an id one past the store
        ids = c_ids.copy()
        ids[-1] = len(refs)
        _refused(ctx, "reference id out of range", q_ab, q_off, nq, ids, c_off, 0, 0, ...)
        # a query of 65536 bases (the 16-bit rank ends at 65535)
        long_q = cc.seq(range(65536))
        one = np.array([0, 1], np.uint64)
        _refused(ctx, "query longer than 65535 bases", long_q, np.array([0, 65536], np.uint64), 1,
                 np.zeros(1, np.uint32), one, 0, 0, ...)
        # nothing to do: no query, or only empty lists
        out = np.full((4, 6), SENTINEL, np.int32)
        assert _raw(ctx, q_ab, q_off, 0, c_ids, c_off, 0, 0, out) == 0 and (out == SENTINEL).all()
        assert _raw(ctx, q_ab, q_off, 3, c_ids, np.zeros(4, np.uint64), 0, 0, out) == 0 and (out == SENTINEL).all()
        assert _raw(ctx, q_ab, q_off, 3, None, np.full(4, 5, np.uint64), 0, 0, out) == 0 and (out == SENTINEL).all()
        _run_case(ctx, "ranges", settings=[(1, False)], upload=False)
        # the LDS request: 4 * nwords + 2 * (nwords + 2) + max_la + 31 against 150 KB, stepped on the query's length
        wide, wrefs, wq, wcand = cc.lds_limit(1)
        assert cc.lds_bytes(wide, len(wq[0])) == cc.LDS_LIMIT + 1
        _upload(ctx, wide, wrefs)
        _refused(ctx, "too wide for the device comparison", wq[0], cc.offsets(wq), 1, cc.flat(wcand), cc.offsets(wcand),
                 0, 0, ...)
        assert cc.lds_bytes(wide, len(cc.case("lds_limit")[2][0])) == cc.LDS_LIMIT
        _run_case(ctx, "lds_limit")            # one base fewer: accepted, and right
    finally:
        ctx.close()
