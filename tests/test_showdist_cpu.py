"""CPU side of --show-dist on the device (the aligner's device-dist): every case of tests/showdist_cases.py reaches its
edge; tests/showdist_ref.py pinned to the oracle (counters, float bits, the closest relative) and the host's
show_dist_report pinned to both, walking and from rows; csrc/showdist_plan.h in a stand-alone program under the address
and undefined-behaviour sanitizers; the additions to the C ABI; the stage option.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from sina_amd import capi, pipeline
from tests import compare_cases as cc
from tests import showdist_cases as sc
from tests import showdist_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.float32(x).tobytes()


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_reaches_its_edge(name):
    case = sc.case(name)
    rows = sc.expected(name)
    assert rows.shape == (len(case["orig"]), 20) and (rows[:, sr.FLAGS] & sr.FLAG_COMPUTED).all()
    case["why"](case, rows)


def test_cases_cover_the_list():
    sizes = {len(x) for n in sc.NAMES for x in sc.case(n)["lists"]}
    assert {0, 1, 4, 5, 41} <= sizes
    assert {sc.case(n)["width"] for n in sc.NAMES} >= {33, 64, 8224, 50000}
    for seed in sc.FUZZ_SEEDS:
        c, rows = sc.fuzz(seed)
        assert len(rows) == len(c["orig"]) >= 4 and any(len(set(x.tolist())) < len(x) for x in c["lists"])   # an id twice


def _oracle_rows(oracle, case, queries):
    """The rows from the reference's own comparator: counters by compare_counts, the closest relative by a sort of its
    float scores and the names."""
    cs = [oracle.Cseq.from_packed(n, r, case["width"]) for n, r in zip(case["names"], case["refs"])]
    out = {}
    for q in queries:
        o = oracle.Cseq.from_packed("o", case["orig"][q], case["width"])
        a = oracle.Cseq.from_packed("a", case["aligned"][q], case["width"])
        row = np.zeros(20, np.uint32)
        row[0:6] = oracle.compare_counts(o, a, "exact", False)
        floats = [oracle.compare(o, a, "exact", "none", "query")]
        scored, flags = [], sr.FLAG_COMPUTED
        for i in case["lists"][q]:
            s = oracle.compare(o, cs[int(i)], "optimistic", "none", "query")
            if np.isnan(s):
                flags |= sr.FLAG_NAN
            else:
                scored.append((float(s), case["names"][int(i)].encode(), int(i)))
        row[18] = sr.NONE
        if scored:
            closest = sorted(scored)[-1][2]
            row[6:12] = oracle.compare_counts(o, cs[closest], "optimistic", False)
            row[12:18] = oracle.compare_counts(a, cs[closest], "optimistic", False)
            row[18] = closest
            floats += [oracle.compare(o, cs[closest], "optimistic", "none", "query"),
                       oracle.compare(a, cs[closest], "optimistic", "none", "query")]
        row[19] = flags
        out[q] = (row, floats)
    return out


@pytest.mark.parametrize("name", sc.NAMES)
def test_ref_equals_the_oracle(oracle, name):
    case = sc.case(name)
    rows = sc.expected(name)
    queries = list(range(min(len(rows), 24)))
    for q, (row, floats) in _oracle_rows(oracle, case, queries).items():
        assert (rows[q] == row).all(), (name, q, rows[q].tolist(), row.tolist())
        mine = [sr.score(rows[q][at:at + 6]) for at in (sr.SELF, sr.BEFORE, sr.AFTER)][:len(floats)]
        assert all((np.isnan(x) and np.isnan(y)) or _bits(x) == _bits(y) for x, y in zip(mine, floats)), (name, q, mine, floats)


def test_ref_equals_the_oracle_on_fuzz(oracle):
    for seed in sc.FUZZ_SEEDS:
        case, rows = sc.fuzz(seed)
        for q, (row, _) in _oracle_rows(oracle, case, range(len(rows))).items():
            assert (rows[q] == row).all(), (seed, q)


def _host_reports(store, case, rows=None):
    H = store.H
    o_ab, o_off, a_ab, a_off, ids, l_off = sc.flat_call(case)
    nq = len(o_off) - 1
    out = np.zeros((nq, 3), np.float32)
    flags, closest = np.zeros(nq, np.uint32), np.zeros(nq, np.uint32)
    text = C.create_string_buffer(200 * nq + 16)
    p = lambda x, t: x.ctypes.data_as(t)  # noqa: E731
    rp = None if rows is None else p(np.ascontiguousarray(rows, np.uint32), capi.u32p)
    pipeline._chk(H.sina_host_show_dist_reports(store.key.encode(), p(o_ab, capi.u32p), p(o_off, capi.u64p), p(a_ab, capi.u32p),
                                                p(a_off, capi.u64p), nq, p(ids, capi.u32p), p(l_off, capi.u64p), rp,
                                                p(out, capi.f32p), p(flags, capi.u32p), p(closest, capi.u32p), text, len(text)))
    return out, flags, closest, text.value.decode()


@pytest.mark.parametrize("name", [n for n in sc.NAMES if n != "nq_600"] + ["nq_600"])
def test_host_report_walking_and_from_rows(name):
    """show_dist_report: the walk gives showdist_ref's floats (bit for bit, NaN for NaN), flags and closest relative; a
    set row gives what the walk gives, text included -- on every query whose row is not flagged (a flagged tray keeps
    the walk)."""
    case = sc.case(name)
    rows = sc.expected(name)
    refs = types.SimpleNamespace(ab=cc.flat(case["refs"]), off=cc.offsets(case["refs"]), n=len(case["refs"]), width=case["width"])
    st = pipeline.Store(":mem:showdist-cpu-" + name, refs)
    try:
        assert [st.name(i) for i in range(min(refs.n, 12))] == case["names"][:12]
        walk = _host_reports(st, case)
        keep = [q for q in range(len(rows)) if not rows[q][sr.FLAGS] & sr.FLAG_NAN]
        assert keep
        for q in keep:
            want = sr.report(rows[q], len(case["lists"][q]))
            got = walk[0][q]
            assert walk[1][q] == (1 | (2 if want["has_closest"] else 0))
            for x, y in zip(got, (want["sps"], want["idty"], want["cpm"])):
                assert (np.isnan(x) and np.isnan(y)) or _bits(x) == _bits(y), (name, q, got, want)
            assert walk[2][q] == want["closest"]
        sub = dict(case, orig=[case["orig"][q] for q in keep], aligned=[case["aligned"][q] for q in keep],
                   lists=[case["lists"][q] for q in keep])
        a, b = _host_reports(st, sub), _host_reports(st, sub, rows[keep])
        assert a[0].tobytes() == b[0].tobytes() and (a[1] == b[1]).all() and (a[2] == b[2]).all() and a[3] == b[3]
        reports = [sr.report(rows[q], len(case["lists"][q])) for q in keep]
        if not any(np.isnan(r["sps"]) or np.isnan(r["cpm"]) for r in reports):      # (C prints a NaN with its sign)
            assert a[3] == "".join(r["text"] for r in reports)
        assert "reference / search result empty?" in a[3] or all(len(x) for x in sub["lists"])
    finally:
        st.close()


def test_plan_against_plain_arithmetic(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "showdist_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "sina_amd", "csrc"), os.path.join(ROOT, "tests", "showdist_plan_check.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert run.returncode == 0 and "showdist_plan_check: ok" in run.stdout, run.stdout[-4000:]
    plan = open(os.path.join(ROOT, "sina_amd", "csrc", "showdist_plan.h")).read()
    assert "#include <hip" not in plan and "hip_runtime" not in plan
    assert "kShowDistRowWords = %d" % sr.ROW_WORDS in plan
    for word, at in (("Self", sr.SELF), ("Before", sr.BEFORE), ("After", sr.AFTER), ("Closest", sr.CLOSEST), ("Flags", sr.FLAGS)):
        assert re.search(r"kShowDist%s = %d;" % (word, at), plan), word


def test_abi_additions():
    header = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    protos = {
        "sina_hip_show_dist": "int sina_hip_show_dist(sina_hip_ctx *ctx, const uint32_t *orig_ab, const uint64_t *orig_off, "
                              "const uint32_t *al_ab, const uint64_t *al_off, uint32_t nq, const uint32_t *ref_ids, "
                              "const uint64_t *ref_off, uint32_t *rows);",
        "sina_hip_show_dist_stats": "int sina_hip_show_dist_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *sequences, "
                                    "uint64_t *pairs, uint64_t *launches);",
    }
    stub = open(os.path.join(ROOT, "tools", "hoststub", "fake_hip.cpp")).read()
    L = capi.load()
    for sym, proto in protos.items():
        assert proto in flat, sym
        assert sym in capi.ABI_SYMBOLS and hasattr(L, sym)
        assert re.search(r"\bint %s\(" % sym, stub)
        assert getattr(L, sym).argtypes is not None
    for method in ("show_dist", "show_dist_stats"):
        assert callable(getattr(capi.Context, method))
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", header) and L.sina_hip_abi_version() == 5
    assert "} sina_hip_match_counts;" in header and "} sina_hip_stats;" in header      # no struct changed
    src = open(os.path.join(ROOT, "sina_amd", "csrc", "showdist.hip")).read()
    assert "show_dist_kernel" in src and src.count("build_query_tables(") == 2 and "asm" not in src
    make = open(os.path.join(ROOT, "sina_amd", "csrc", "Makefile")).read()
    assert "$(B)/showdist.o" in make and "fast-math" not in make and "-Ofast" not in make


def test_aligner_takes_device_dist_and_host_takes_show_dist():
    H = pipeline.load_host()
    H.sina_host_reset_options()
    try:
        assert H.sina_host_set_option(b"aligner", b"device-dist", b"1") == 0
        assert H.sina_host_set_option(b"aligner", b"device-dist", b"0") == 0
        assert H.sina_host_set_option(b"aligner", b"device-dits", b"1") != 0
        assert b"unknown option device-dits" in H.sina_host_last_error()
        assert H.sina_host_set_option(b"host", b"show-dist", b"1") == 0
    finally:
        H.sina_host_reset_options()
    for sym in ("sina_host_store_show_dist_stats", "sina_host_result_dist", "sina_host_show_dist_reports"):
        assert hasattr(H, sym)
    assert callable(pipeline.Store.show_dist_stats)
