"""CPU side of the orientation on the device (device-turn): every case of tests/turn_cases.py sits on its edge;
tests/turn_ref.py equals the oracle's so_turn_check (orientation and the four scores) and its variants equal
so_cseq_reverse / so_cseq_complement, on stores indexed by the oracle; csrc/turn_plan.h in a stand-alone program under
the address and undefined-behaviour sanitizers; the additions to the C ABI; the stage option.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sina_amd import capi, pipeline, synth
from tests import turn_cases as tc
from tests import turn_ref as tr
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", tc.NAMES)
def test_case_sits_on_its_edge(name):
    c = tc.case(name)
    c.why(c)
    for r in c.runs:
        for e in c.expected(r["all"], r["mx"]):
            assert e["turn"] in tr.ORDER[r["all"]] and len(e["ids"]) == min(r["mx"], c.world.n_refs)
            assert all(e["top1"][o] == 0 for o in range(4) if o not in tr.ORDER[r["all"]])


def test_cases_cover_the_list():
    runs = [(c.world.n_refs, r["mx"], r["all"], tuple(sorted(r["knobs"].items()))) for c in map(tc.case, tc.NAMES) for r in c.runs]
    for n_refs in (tc.SMALL, tc.BIG):
        assert {mx for n, mx, _, _ in runs if n == n_refs} >= {1, 41, 128, 129}
    assert tc.SMALL < 65536 <= tc.BIG
    assert any(n == tc.BIG and kn == (("kmer_rows", 1),) for n, _, _, kn in runs)
    assert any(n == tc.SMALL and mx == 4097 for n, mx, _, _ in runs)
    assert {kn for _, _, _, kn in runs} >= {(("turn_range", x),) for x in (1, 2, 3)}
    assert {a for _, _, a, _ in runs} == {True, False}
    assert any(len(tc.case(n).qmasks) == 1 for n in tc.NAMES) and tc.case("long_query").n_long() == 1
    for seed in range(tc.FUZZ_SEEDS):
        c = tc.fuzz(seed)
        assert 3 <= len(c.qmasks) <= 9 and len(c.runs) == 2
    assert {tc.fuzz(s).world.n_refs for s in range(tc.FUZZ_SEEDS)} == {tc.SMALL, tc.BIG}


def _cseq(oracle, masks):
    m = np.asarray(masks, np.uint8)
    return oracle.Cseq.from_packed("q", np.arange(len(m), dtype=np.uint32) | (m.astype(np.uint32) << 24), len(m))


def test_variants_equal_the_oracles_reverse_and_complement(oracle):
    rng = np.random.default_rng(77)
    queries = [np.array(tc.ALL30, np.uint8), tc.case("alphabet").qmasks[0]] + [rng.integers(1, 32, size=n).astype(np.uint8) for n in (1, 2, 63, 64, 257)]
    for m in queries:
        m = m[m != 16]
        for o in range(4):
            q = _cseq(oracle, m)
            if o & 1:
                oracle.lib().so_cseq_reverse(q.h)
            if o & 2:
                oracle.lib().so_cseq_complement(q.h)
            got = (q.packed() >> 24).astype(np.uint8)
            assert (got == tr.variant(m, o)).all(), (len(m), o)
            assert (np.diff((q.packed() & 0xFFFFFF).astype(np.int64)) > 0).all()          # (columns still ascend)


@pytest.mark.parametrize("nofast", (False, True))
def test_ref_equals_the_oracles_turn_check(oracle, nofast):
    """500 references indexed by the oracle, 12 queries handed in all four orientations (the shape of
    tests/test_gpu_scale.py::test_turn_orientations_equal_oracle), and three that are no relatives of anything."""
    refs = synth.make_refs(500, length=320, width=3200, seed=51)
    k = 8
    idx = oracle.Index(util.cseqs_from_refs(refs), k=k, nofast=nofast)
    off, ids = idx.csr()
    base = synth.make_queries(refs, 12, seed=57)
    rng = np.random.default_rng(58)
    masks = [tr.variant(base.seq(qi), qi % 4) for qi in range(base.n)]
    masks += [rng.choice([1, 2, 4, 8], size=n).astype(np.uint8) for n in (3, k, 200)]
    turned = 0
    for qi, m in enumerate(masks):
        rows = tr.rows_of(off, ids, refs.n, m, k, not nofast)
        for all_four in (False, True):
            want_o, want_sc = idx.turn_check(_cseq(oracle, m), all_four)
            got = tr.orient(rows, all_four, 1)
            assert got["turn"] == want_o and (got["top1"] == want_sc).all(), (qi, all_four, got["top1"], want_sc)
            if all_four and qi < base.n:
                assert want_o == qi % 4
                turned += want_o != 0
    assert turned == 9
    for sc in ([0, 0, 0, 0], [2, 2, 2, 2], [1, 3, 3, 1], [0, 0, 0, 1], [1, 0, 0, 1]):
        assert tr.pick(sc) == int(np.argmax(sc)) if max(sc) > 0 else tr.pick(sc) == 0


def test_plan_against_plain_arithmetic(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "turn_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "sina_amd", "csrc"), os.path.join(ROOT, "tests", "turn_plan_check.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert run.returncode == 0 and "turn_plan_check: ok" in run.stdout, run.stdout[-4000:]
    plan = open(os.path.join(ROOT, "sina_amd", "csrc", "turn_plan.h")).read()
    assert "#include <hip" not in plan and "hip_runtime" not in plan
    assert "kTurnOrder[4] = {0, 3, 1, 2}" in plan


def test_abi_additions():
    header = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    protos = {
        "sina_hip_kmer_topk_turn": "int sina_hip_kmer_topk_turn(sina_hip_ctx *ctx, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, "
                                   "uint32_t max, int all, uint8_t *out_turn, float *out_top1 /* [nq][4] */, "
                                   "uint32_t *out_ids, float *out_scores, uint32_t *out_n);",
        "sina_hip_turn_stats": "int sina_hip_turn_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *queries, uint64_t *turned, "
                               "uint64_t *launches);",
    }
    stub = open(os.path.join(ROOT, "tools", "hoststub", "fake_hip.cpp")).read()
    L = capi.load()
    for sym, proto in protos.items():
        assert proto in flat, sym
        assert sym in capi.ABI_SYMBOLS and hasattr(L, sym)
        assert re.search(r"\bint %s\(" % sym, stub)
        assert getattr(L, sym).argtypes is not None
    for method in ("kmer_topk_turn", "turn_stats"):
        assert callable(getattr(capi.Context, method))
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", header) and L.sina_hip_abi_version() == 5
    assert "src/famfinder.cpp:344-378" in header
    src = open(os.path.join(ROOT, "sina_amd", "csrc", "turn.hip")).read()
    assert "turn_orient_kernel" in src and "turn_pick_kernel" in src and "asm" not in src and "atomic" not in src.replace("no atomics", "")
    make = open(os.path.join(ROOT, "sina_amd", "csrc", "Makefile")).read()
    assert "$(B)/turn.o" in make and "$(B)/turn.o: turn_plan.h" in make


def test_famfinder_takes_device_turn():
    """The stage option, through the host library and without a device (before the feature: "unknown option")."""
    H = pipeline.load_host()
    H.sina_host_reset_options()
    try:
        assert H.sina_host_set_option(b"famfinder", b"device-turn", b"1") == 0, H.sina_host_last_error()
        assert H.sina_host_set_option(b"famfinder", b"device-turn", b"0") == 0
        assert H.sina_host_set_option(b"famfinder", b"device-tunr", b"1") != 0
        assert b"unknown option device-tunr" in H.sina_host_last_error()
    finally:
        H.sina_host_reset_options()
    assert hasattr(H, "sina_host_store_turn_stats")
    assert callable(pipeline.Store.turn_stats)
