"""The device assembly with shifted insertions (sina_hip_align_params::assemble == 2), everything that needs no GPU:
the hand-built cases reach the branches they are there for, the plain restatement (tests/shift_ref.py) equals the
oracle's so_cseq_fix_duplicate_positions and the host's sina_host_fix_duplicates in words, return code and log text,
must_assemble_shift is false exactly for the cap cases, the new symbols are exported and declared, and the inputs of the
through-DP GPU test do shift (so that test cannot pass by shifting nothing)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sina_amd import capi, pipeline
from tests import shift_cases as sc, shift_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sina_hip_staged_shift_log", "sina_hip_assemble_stats", "sina_hip_debug_assemble", "sina_hip_debug_assemble_ms")


def _fx(case):
    colm = sr.append_rule(case.emitted)
    if any(c >= case.width for c in colm):
        return colm, None
    return colm, sr.fix_up(sr.mirror(colm, case.width), case.width)


@pytest.mark.parametrize("case", sc.CASES, ids=[c.name for c in sc.CASES])
def test_case_reaches_its_branch(case):
    colm, fx = _fx(case)
    assert case.why(fx), case.name
    assert sr.must_assemble_shift(case.n, colm, case.width, fx) == (not case.cap), case.name


def test_cases_cover_the_widening_loop():
    """Counted over all cases by the restatement: widenings to both sides, ties, events, absorbed runs, both ends."""
    steps, events = [], 0
    for case in sc.CASES:
        fx = _fx(case)[1]
        if fx:
            steps += fx["steps"]
            events += len(fx["events"])
    assert sum(s["side"] == "L" for s in steps) >= 20 and sum(s["side"] == "R" for s in steps) >= 20
    assert any(s["tie"] for s in steps) and events >= 80
    assert any(s["dup_absorbed"] for s in steps) and any(s["placed_absorbed"] for s in steps)
    assert any(s["reached_first"] for s in steps) and any(s["reached_last"] for s in steps)
    assert max(s["absorbed"] for s in steps) > 2000          # (the capacity cases: scans over dozens of ballots)


def _lists():
    """(name, words, width) of every case whose columns stay below the width, and of 300 seeded random lists."""
    out = []
    for case in sc.CASES:
        colm = sr.append_rule(case.emitted)
        if all(c < case.width for c in colm):
            out.append((case.name, sr.mirror(colm, case.width), case.width))
    rng = np.random.default_rng(2024)
    for i in range(300):
        cols, width = sc.random_cols(rng)
        out.append(("random %d" % i, cols, width))
    res = []
    rng = np.random.default_rng(7)
    for name, cols, width in out:
        mask = rng.choice(np.array([1, 2, 4, 8, 15, 17], np.uint32), size=len(cols))
        res.append((name, (np.array(cols, np.uint32) | (mask << 24)).astype(np.uint32), width))
    return res


def test_restatement_equals_oracle(oracle):
    L = oracle.lib()
    n_shift = n_throw = 0
    for name, ab, width in _lists():
        for lowercase in (0, 1):
            rc, words, txt, fx = sr.fix_words(ab, width, lowercase)
            c = oracle.Cseq.from_packed("x", ab, width)
            lg = oracle.new_log()
            orc = L.so_cseq_fix_duplicate_positions(c.h, C.byref(lg), lowercase, 0)
            otxt = oracle.log_text(lg)
            L.so_log_free(C.byref(lg))
            assert rc == orc, name
            if rc == 0:
                assert (words == c.packed()).all(), name
                assert txt == otxt, name
                n_shift += bool(fx["events"])
            else:
                n_throw += 1
    assert n_shift > 100 and n_throw > 2


def test_restatement_equals_host():
    H = pipeline.load_host()
    for name, ab, width in _lists():
        for lowercase in (0, 1):
            rc, words, txt, _ = sr.fix_words(ab, width, lowercase)
            mine = ab.copy()
            log = C.create_string_buffer(1 << 16)
            hrc = H.sina_host_fix_duplicates(mine.ctypes.data_as(capi.u32p), len(mine), width, lowercase, 0, log, len(log))
            assert (hrc == 2) == (rc == -1) and hrc in (0, 2), name
            if rc == 0:
                assert (mine == words).all(), name
                assert log.value.decode() == txt, name


def test_new_symbols_and_version():
    text = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", text)
    assert re.search(r"#define SINA_ASSEMBLE_SHIFT 2\b", text) and re.search(r"#define SINA_HIP_SHIFT_LOG 32u\b", text)
    assert re.search(r"\bconst uint32_t \*sina_hip_staged_shift_log\(sina_hip_ctx \*ctx\);", text)
    assert re.search(r"\bint sina_hip_assemble_stats\(sina_hip_ctx \*ctx, uint64_t \*queries, uint64_t \*assembled, "
                     r"uint64_t \*shifted_queries,\s+uint64_t \*shifted_runs\);", text)
    assert re.search(r"\bint sina_hip_debug_assemble\(sina_hip_ctx \*ctx, const sina_hip_align_params \*p, uint32_t width, "
                     r"const uint8_t \*qmask,\s+const uint64_t \*qoff, uint32_t nq, sina_hip_align_out \*out, uint32_t \*out_pos\);", text)
    L = capi.load()
    assert L.sina_hip_abi_version() == 5
    for name in NEW:
        assert hasattr(L, name) and name in capi.ABI_SYMBOLS
    assert capi.ASSEMBLE_SHIFT == 2 and capi.SHIFT_LOG == sr.SHIFT_LOG == 32
    stub = open(os.path.join(ROOT, "tools", "hoststub", "fake_hip.cpp")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, stub), name
    for name in ("staged_shift_log", "assemble_stats", "debug_assemble", "debug_assemble_ms"):
        assert callable(getattr(capi.Context, name))
    # (no context: the getters refuse, nothing is touched)
    assert not L.sina_hip_staged_shift_log(None) and b"staged_shift_log" in L.sina_hip_last_error()
    a = C.c_uint64()
    assert L.sina_hip_assemble_stats(None, C.byref(a), C.byref(a), C.byref(a), C.byref(a)) != 0
    assert b"assemble_stats" in L.sina_hip_last_error()


def test_dp_inputs_shift(oracle):
    """The block-layout store of the through-DP GPU test: by the oracle's logs at least half of its queries shift and
    none has more than 32 events -- the device must finish every one of them."""
    w = sc.dp_world()
    refs = w["refs"]
    assert 40 <= refs.n <= 60 and all(120 <= refs.off[i + 1] - refs.off[i] <= 300 for i in range(refs.n))
    events = [len(sc.log_events(r["log"])) for r in w["want"]]
    assert all(r["status"] == 0 for r in w["want"])
    assert sum(e > 0 for e in events) * 2 >= len(events) and max(events) <= sr.SHIFT_LOG, events
    assert max(events) >= 3
