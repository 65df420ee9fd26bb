"""CPU side of the aligner's exact-relative test on the device (device-copy): every case of tests/contain_cases.py sits
on its edge; tests/contain_ref.py equals Python's find on the host-rendered, upper-cased base strings and the host's
own find_bases; the sixteen base codes render to sixteen different characters, T and U to one; csrc/contain_plan.h in a
stand-alone program under the address and undefined-behaviour sanitizers; the additions to the C ABI; the stage option.
No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sina_amd import capi, pipeline
from tests import contain_cases as kc
from tests import contain_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", kc.NAMES)
def test_case_sits_on_its_edge(name):
    case, want = kc.case(name), kc.expected(name)
    assert len(want) == sum(len(x) for x in case["lists"]) and want.dtype == np.uint32
    case["why"](case, want)


def test_cases_cover_the_list():
    lens = {len(q) for n in kc.NAMES for q in kc.case(n)["queries"]}
    assert set(kc.NEEDLE_LENGTHS) <= lens
    for n in kc.NEEDLE_LENGTHS:
        rl = {len(r) for r in kc.case("needle_%d" % n)["refs"]}
        assert {n, n + 1, 63, 64, 65, 127, 128, 129} <= rl and max(rl) >= 1500
    world, own = kc.merged()
    assert sum(s.stop - s.start for s in own.values()) == sum(len(x) for x in world["lists"])
    assert any(len(x) == 0 for x in world["lists"])
    for seed in kc.FUZZ_SEEDS:
        c, want = kc.fuzz(seed)
        lens = [len(q) for q in c["queries"]] + [len(r) for r in c["refs"]]
        assert 200 <= len(want) <= 900 and min(lens) >= 1 and max(lens) <= 300
        hits = (want != cr.NONE).sum()
        assert hits >= len(want) // 8 and len(want) - hits >= len(want) // 8           # hits and misses are both frequent
        assert {int(x) for r in c["refs"] for x in r} == {kc.A, kc.C}


def _host_find(H, ref, query):
    """The host's walk on one pair (getBases, upper-cased, find_bases): its answer and the two strings."""
    h, n = kc.packed(ref), kc.packed(query)
    at = C.c_uint32()
    cap = max(len(h), len(n)) + 8
    ht, nt = C.create_string_buffer(cap), C.create_string_buffer(cap)
    pipeline._chk(H.sina_host_find_bases_packed(h.ctypes.data_as(capi.u32p), len(h), n.ctypes.data_as(capi.u32p), len(n), C.byref(at),
                                                ht, nt, cap))
    return at.value, ht.value.decode(), nt.value.decode()


@pytest.mark.parametrize("name", kc.NAMES)
def test_ref_equals_find_on_the_host_rendered_strings(name):
    H = pipeline.load_host()
    case, want = kc.case(name), kc.expected(name)
    at = 0
    for q, ids in zip(case["queries"], case["lists"]):
        for i in ids:
            got, hay, nd = _host_find(H, case["refs"][int(i)], q)
            assert len(hay) == len(case["refs"][int(i)]) and len(nd) == len(q) and hay == hay.upper() and nd == nd.upper()
            py = hay.find(nd)
            assert (cr.NONE if py < 0 else py) == want[at] == got, (name, at)
            assert cr.is_query_itself(int(want[at]), len(q), len(hay)) == (hay == nd)
            at += 1


def test_ref_equals_the_host_walk_on_fuzz():
    H = pipeline.load_host()
    c, want = kc.fuzz(kc.FUZZ_SEEDS[0])
    at = 0
    for q, ids in zip(c["queries"], c["lists"]):
        for i in ids:
            got, hay, nd = _host_find(H, c["refs"][int(i)], q)
            assert got == want[at] and (hay == nd) == cr.is_query_itself(int(want[at]), len(q), len(hay))
            at += 1


def test_sixteen_codes_render_one_to_one():
    """Upper-cased characters of two bases are equal exactly when their four base bits are: sixteen codes, sixteen
    characters, with the case bit and without; T and U are read as one code."""
    H = pipeline.load_host()
    upper = [_host_find(H, np.array([m], np.uint8), np.array([m], np.uint8))[1] for m in range(16)]
    lower = [_host_find(H, np.array([m | kc.LOWER], np.uint8), np.array([m], np.uint8))[1] for m in range(16)]
    assert all(len(ch) == 1 for ch in upper) and len(set(upper)) == 16 and upper == lower
    for a in range(16):
        for b in range(16):
            at, _, _ = _host_find(H, np.array([a | kc.LOWER], np.uint8), np.array([b], np.uint8))
            assert (at == 0) == (a == b) and at in (0, cr.NONE)
            assert cr.find([b], [a | kc.LOWER]) == at
    out = C.create_string_buffer(32)
    size, width = C.c_uint32(), C.c_uint32()
    texts = []
    for s in (b"ACGT", b"ACGU", b"acgt"):
        assert H.sina_host_cseq_op(s, 0, 0, 3, out, 32, C.byref(size), C.byref(width)) == 0
        texts.append(out.value.decode().upper())
    assert texts[0] == texts[1] == texts[2] and len(texts[0]) == 4


def test_plan_against_plain_arithmetic(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "contain_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "sina_amd", "csrc"), os.path.join(ROOT, "tests", "contain_plan_check.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert run.returncode == 0 and "contain_plan_check: ok" in run.stdout, run.stdout[-4000:]
    plan = open(os.path.join(ROOT, "sina_amd", "csrc", "contain_plan.h")).read()
    assert "#include <hip" not in plan and "hip_runtime" not in plan
    assert "kContainNone = 0xFFFFFFFFu" in plan and "kContainPairsPerWg = 4" in plan and "kContainMaxBases = 65535" in plan


def test_abi_additions():
    header = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    protos = {
        "sina_hip_find_bases": "int sina_hip_find_bases(sina_hip_ctx *ctx, const uint8_t *qmask, const uint64_t *q_off, uint32_t nq, "
                               "const uint32_t *cand_ids, const uint64_t *cand_off, uint32_t *out_at);",
        "sina_hip_find_bases_stats": "int sina_hip_find_bases_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *pairs, "
                                     "uint64_t *ref_bases, uint64_t *launches);",
    }
    stub = open(os.path.join(ROOT, "tools", "hoststub", "fake_hip.cpp")).read()
    L = capi.load()
    for sym, proto in protos.items():
        assert proto in flat, sym
        assert sym in capi.ABI_SYMBOLS and hasattr(L, sym)
        assert re.search(r"\bint %s\(" % sym, stub)
        assert getattr(L, sym).argtypes is not None
    for method in ("find_bases", "find_bases_stats"):
        assert callable(getattr(capi.Context, method))
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", header) and L.sina_hip_abi_version() == 5
    assert "} sina_hip_match_counts;" in header and "} sina_hip_stats;" in header      # no struct changed
    src = open(os.path.join(ROOT, "sina_amd", "csrc", "contain.hip")).read()
    assert "find_bases_kernel" in src and "__ballot" in src and "__ffsll" in src and "asm" not in src and "atomic" not in src.replace("No atomics", "")
    make = open(os.path.join(ROOT, "sina_amd", "csrc", "Makefile")).read()
    assert "$(B)/contain.o" in make and "fast-math" not in make and "-Ofast" not in make


def test_aligner_takes_device_copy():
    """The stage option, through the host library and without a device (before the feature: "unknown option")."""
    H = pipeline.load_host()
    H.sina_host_reset_options()
    try:
        assert H.sina_host_set_option(b"aligner", b"device-copy", b"1") == 0, H.sina_host_last_error()
        assert H.sina_host_set_option(b"aligner", b"device-copy", b"0") == 0
        assert H.sina_host_set_option(b"aligner", b"device-cpoy", b"1") != 0
        assert b"unknown option device-cpoy" in H.sina_host_last_error()
    finally:
        H.sina_host_reset_options()
    for sym in ("sina_host_store_copy_stats", "sina_host_find_bases_packed"):
        assert hasattr(H, sym)
    assert callable(pipeline.Store.copy_stats)
