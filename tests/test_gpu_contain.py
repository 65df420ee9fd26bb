"""find_bases_kernel and its entry point (sina_hip_find_bases) against tests/contain_ref.py, word for word: every case of
tests/contain_cases.py in one call (also cut into launch ranges of 1, 3 and 64 pairs), seeded fuzz over a two-letter
alphabet, sub-ranges of larger offset arrays, the refusals and the kernel's counters.  tests/test_contain_cpu.py pins
contain_ref to the host's walk and checks that every case sits on its edge.  All comparisons are exact."""
import contextlib
import os

import numpy as np
import pytest

from sina_amd import capi
from tests import contain_cases as kc
from tests import contain_ref as cr

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _knob(text):
    old = os.environ.get("SINA_HIP_TEST")
    os.environ["SINA_HIP_TEST"] = text
    try:
        yield
    finally:
        if old is None:
            del os.environ["SINA_HIP_TEST"]
        else:
            os.environ["SINA_HIP_TEST"] = old


def _upload(ctx, case):
    ab, off = kc.flat_refs(case)
    ctx.upload_refs(ab, off, kc.width_of(case))


def _same(got, want, tag, own=None):
    bad = np.flatnonzero(got != want)
    where = [n for n, s in (own or {}).items() if len(bad) and s.start <= bad[0] < s.stop]
    assert len(bad) == 0, (tag, where, "pair %d" % bad[0], int(got[bad[0]]), int(want[bad[0]]), "%d pairs differ" % len(bad))


@pytest.fixture(scope="module")
def world(gpu_ctx):
    case, own = kc.merged()
    want = np.concatenate([kc.expected(n) for n in kc.NAMES])
    assert all((want[own[n]] == kc.expected(n)).all() for n in kc.NAMES)
    want.setflags(write=False)
    return case, own, want


def test_every_named_case_in_one_call(gpu_ctx, world):
    case, own, want = world
    _upload(gpu_ctx, case)
    args = kc.flat_call(case)
    before = gpu_ctx.find_bases_stats()
    _same(gpu_ctx.find_bases(*args), want, "one call", own)
    after = gpu_ctx.find_bases_stats()
    # the kernel's own counters: every pair once, its reference's bases, one launch
    assert after["pairs"] - before["pairs"] == len(want)
    assert after["ref_bases"] - before["ref_bases"] == sum(len(case["refs"][int(i)]) for ids in case["lists"] for i in ids)
    assert after["launches"] - before["launches"] == 1 and after["kernel_ms"] > before["kernel_ms"]


@pytest.mark.parametrize("n", (1, 3, 64))
def test_every_named_case_in_launch_ranges(gpu_ctx, world, n):
    case, own, want = world
    _upload(gpu_ctx, case)
    before = gpu_ctx.find_bases_stats()
    with _knob("contain_pairs=%d" % n):
        _same(gpu_ctx.find_bases(*kc.flat_call(case)), want, "ranges of %d" % n, own)
    after = gpu_ctx.find_bases_stats()
    assert after["launches"] - before["launches"] == (len(want) + n - 1) // n > 1
    assert after["pairs"] - before["pairs"] == len(want)


@pytest.mark.parametrize("seed", kc.FUZZ_SEEDS)
def test_fuzz_over_two_letters(gpu_ctx, seed):
    case, want = kc.fuzz(seed)
    _upload(gpu_ctx, case)
    _same(gpu_ctx.find_bases(*kc.flat_call(case)), want, ("fuzz", seed))
    with _knob("contain_pairs=37"):
        _same(gpu_ctx.find_bases(*kc.flat_call(case)), want, ("fuzz", seed, "ranges of 37"))


def test_subrange_of_larger_arrays(gpu_ctx):
    """Offsets that do not start at zero: queries 1 .. of `pair_layout` (the empty list between two full ones among them)
    addressed inside the full arrays; the words in front of the sub-range stay as they were."""
    case, want = kc.case("pair_layout"), kc.expected("pair_layout")
    _upload(gpu_ctx, case)
    qmask, q_off, ids, c_off = kc.flat_call(case)
    nq = len(q_off) - 2
    out = np.full(len(want), 77, np.uint32)
    p = capi._ptr
    gpu_ctx._check(gpu_ctx.L.sina_hip_find_bases(gpu_ctx.h, p(qmask, capi.u8p), p(q_off[1:].copy(), capi.u64p), nq, p(ids, capi.u32p),
                                                 p(c_off[1:].copy(), capi.u64p), p(out, capi.u32p)))
    first = int(c_off[1])
    assert q_off[1] != 0 and first == 41 and (out[:first] == 77).all()
    _same(out[first:], want[first:], "subrange")


def test_refusals_leave_the_answers_untouched(gpu_ctx):
    case = kc.case("lengths_and_masks")
    _upload(gpu_ctx, case)
    qmask, q_off, ids, c_off = kc.flat_call(case)
    nq = len(q_off) - 1
    out = np.full(len(ids), 0xABCD, np.uint32)
    L, h, p = gpu_ctx.L, gpu_ctx.h, capi._ptr

    def call(qmask=qmask, q_off=q_off, ids=ids, c_off=c_off, out=out, n=nq, ctx=h):
        q = lambda x, t: None if x is None else p(x, t)  # noqa: E731
        return L.sina_hip_find_bases(ctx, q(qmask, capi.u8p), q(q_off, capi.u64p), n, q(ids, capi.u32p), q(c_off, capi.u64p),
                                     q(out, capi.u32p))

    def refused(rc, text):
        assert rc != 0 and text in L.sina_hip_last_error().decode(), L.sina_hip_last_error()
        assert (out == 0xABCD).all()

    before = gpu_ctx.find_bases_stats()
    for missing in ("qmask", "q_off", "ids", "c_off", "out"):
        refused(call(**{missing: None}), "null argument")
    refused(call(ctx=None), "null argument")
    bad = ids.copy()
    bad[-1] = len(case["refs"])
    refused(call(ids=bad), "reference id out of range")
    for which in ("q_off", "c_off"):
        desc = {"q_off": q_off, "c_off": c_off}[which].copy()
        desc[-1] = desc[-2] - 1                     # (the last query ends before it begins: nothing beyond the arrays is read)
        refused(call(**{which: desc}), "offsets descend")
    empty = q_off.copy()
    empty[1:] -= np.uint64(len(case["queries"][0]))  # (query 0 has no bases; the rest keep their lengths)
    refused(call(q_off=empty), "query of 0 bases")
    long_off = np.array([0, 65536], np.uint64)
    refused(call(qmask=np.full(65536, kc.A, np.uint8), q_off=long_off, c_off=np.array([0, 2], np.uint64), n=1), "longer than 65535 bases")
    with _knob("contain_fail=1"):
        refused(call(), "refused by the test knob")
    fresh = capi.Context(0)
    try:
        refused(call(ctx=fresh.h), "upload references first")
    finally:
        fresh.close()
    assert gpu_ctx.find_bases_stats() == before     # nothing ran
    # the empty call: no candidates at all, and a sub-range whose candidates are none
    none_off = np.zeros(nq + 1, np.uint64) + np.uint64(3)
    assert call(c_off=none_off) == 0 and (out == 0xABCD).all()
    assert call(n=0) == 0 and (out == 0xABCD).all()
    assert gpu_ctx.find_bases_stats() == before     # ... launches nothing
    # 65535 bases are taken
    big = np.full(65535, kc.A, np.uint8)
    one = np.full(2, 0xABCD, np.uint32)
    assert call(qmask=big, q_off=np.array([0, 65535], np.uint64), ids=np.array([0, 1], np.uint32), c_off=np.array([0, 2], np.uint64),
                out=one, n=1) == 0
    assert (one == cr.NONE).all()
    after = gpu_ctx.find_bases_stats()
    assert after["launches"] - before["launches"] == 1 and after["pairs"] - before["pairs"] == 2
