"""CPU side of the in-place family identity (tests/test_gpu_identity.py runs it): the three added entries through every
layer that names them, the ABI version left as it was, identity_plan.h as a sanitized stand-alone program, and the
conditions on the GPU test's inputs -- checked here with the oracle, so that the GPU test cannot pass on inputs that
show nothing."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sina_amd import capi, pipeline
from tests import identity_cases as ic, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sina_hip_align_count_identity", "sina_hip_staged_identity", "sina_hip_identity_inplace_stats")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", text)
    assert re.search(r"\bint sina_hip_align_count_identity\(sina_hip_ctx \*ctx, int on\);", text)
    assert re.search(r"\bconst uint32_t \*sina_hip_staged_identity\(sina_hip_ctx \*ctx\);", text)
    assert re.search(r"\bint sina_hip_identity_inplace_stats\(sina_hip_ctx \*ctx, double \*kernel_ms, uint64_t \*sequences, "
                     r"uint64_t \*pairs,\s+uint64_t \*launches\);", text)
    assert "src/align.cpp:380-382" in text and "src/align.cpp:443-453" in text      # the reference lines they replace
    L = capi.load()
    assert L.sina_hip_abi_version() == 5
    for sym in NEW:
        assert sym in capi.ABI_SYMBOLS and hasattr(L, sym), sym
    assert L.sina_hip_align_count_identity.argtypes == [C.c_void_p, C.c_int]
    assert L.sina_hip_staged_identity.argtypes == [C.c_void_p]
    assert L.sina_hip_staged_identity.restype == C.POINTER(C.c_uint32)
    assert len(L.sina_hip_identity_inplace_stats.argtypes) == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "sina_amd", "libsina_hip.so")],
                        stdout=subprocess.PIPE, text=True, check=True).stdout
    for sym in NEW:
        assert re.search(r" T %s$" % sym, nm, re.M), sym
    # no struct of the header changes
    assert C.sizeof(capi.AlignOut) == 52 and C.sizeof(capi.AlignParams) == 48


def test_stub_documents_and_build_list_name_the_entries():
    stub = open(os.path.join(ROOT, "tools", "hoststub", "fake_hip.cpp")).read()
    docs = {n: open(os.path.join(ROOT, n)).read() for n in ("README.md", "DESIGN.md", "INTEGRATION.md")}
    for sym in NEW:
        assert re.search(r"\b%s\(sina_hip_ctx \*" % sym, stub), sym
        for n, doc in docs.items():
            assert sym in doc, (sym, n)
    for n, doc in docs.items():
        assert "device-idty" in doc, n
    assert "3.5c" in docs["DESIGN.md"]
    common = open(os.path.join(ROOT, "sina_amd", "csrc", "common.h")).read()
    assert "fam_chunk_q" in common and "fam_chunk_q" in docs["INTEGRATION.md"]
    assert "identity.o" in open(os.path.join(ROOT, "sina_amd", "csrc", "Makefile")).read()


def test_wrappers_and_option():
    for name in ("count_identity", "staged_identity", "identity_inplace_stats"):
        assert callable(getattr(capi.Context, name)), name
    assert callable(pipeline.Store.identity_inplace_stats)
    H = pipeline.load_host()
    assert hasattr(H, "sina_host_store_identity_inplace_stats")
    H.sina_host_reset_options()
    try:
        assert H.sina_host_set_option(b"aligner", b"device-idty", b"1") == 0
        assert H.sina_host_set_option(b"aligner", b"device-idty", b"0") == 0
        assert H.sina_host_set_option(b"aligner", b"device-idtz", b"1") != 0
    finally:
        H.sina_host_reset_options()


def test_null_context_is_refused_by_name():
    L = capi.load()
    assert L.sina_hip_align_count_identity(None, 1) != 0
    assert b"align_count_identity" in L.sina_hip_last_error()
    assert not L.sina_hip_staged_identity(None)
    assert b"staged_identity" in L.sina_hip_last_error()
    ms, a, b, c = C.c_double(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.sina_hip_identity_inplace_stats(None, C.byref(ms), C.byref(a), C.byref(b), C.byref(c)) != 0
    assert b"identity_inplace_stats" in L.sina_hip_last_error()


def test_identity_plan_check_program(tmp_path):
    """tests/identity_plan_check.cpp: LDS bytes, grid and the counting rule, sanitized, as its own process."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "identity_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "sina_amd", "csrc"),
                    os.path.join(ROOT, "tests", "identity_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert run.returncode == 0 and "identity_plan_check: ok" in run.stdout, run.stdout[-4000:]


@pytest.mark.parametrize("name", sorted(ic.GROUPS))
def test_inputs_are_worth_running(oracle, name):
    """Every launch: the expected scores of its queries are not all equal; some query's best member is not member 0
    (a kernel that looked at the first member alone would fail); 100 x the score is the oracle's own idty, bit for bit,
    on every query the device must assemble; oracle.align's finished sequence is backtrack()'s -- the one `must` was
    decided on -- with strictly ascending columns below the width."""
    for launch, ref in ic.group(name):
        assert len(ref) == len(launch.qmasks) == len(launch.fam_ids)
        must = [r for r in ref if r["must"]]
        assert must, launch.name
        for q, r in enumerate(ref):
            cols = (np.asarray(r["packed"], np.uint32) & 0xFFFFFF).astype(np.int64)
            assert np.array_equal(r["packed"], r["walk_packed"]), (launch.name, q)
            assert len(cols) <= len(launch.qmasks[q]), (launch.name, q)
            if not r["must"]:
                assert r["row"] == (0, 0)
                continue
            assert len(cols) >= 1 and (np.diff(cols) > 0).all() and cols[-1] < launch.width, (launch.name, q)
            score = np.array(r["row"][0], np.uint32).view(np.float32)
            assert util.f32_bits(np.float32(100) * score) == util.f32_bits(r["idty"]), (launch.name, q, score, r["idty"])
            assert 1 <= r["row"][1] <= len(launch.fam_ids[q])
        if len(must) > 1:
            assert len({r["row"][0] for r in must}) > 1, launch.name
        if any(len(f) > 1 for f in launch.fam_ids):
            assert any(r["first"] > 0 for r in must), launch.name
        # a member's score differs from the best somewhere: the maximum is a choice
        assert any(b is not None and b != r["row"][0] for r in must for b in r["member_bits"]) or \
            all(len(f) == 1 for f in launch.fam_ids), launch.name


def test_directed_conditions(oracle):
    # family_sizes: the sizes of the issue, in one launch
    (launch, ref), = ic.group("family_sizes")
    assert tuple(len(f) for f in launch.fam_ids) == (1, 3, 4, 5, 8, 9, 40, 128) and all(r["must"] for r in ref)
    # shared_family: 0 and 2 share a list, 1 has another, 3 has 0's in another order -- and 0's identity
    (launch, ref), = ic.group("shared_family")
    f = launch.fam_ids
    assert f[0] is f[2] and f[1] is not f[0] and f[3] != f[0] and sorted(f[3]) == sorted(f[0])
    assert ref[3]["row"] == ref[0]["row"] and ref[2]["row"] != ref[0]["row"]
    # member_outside: a member with denominator 0 -- wholly right of the query's last column
    (launch, ref), = ic.group("member_outside")
    for q, r in enumerate(ref):
        assert r["must"] and r["row"][1] == len(launch.fam_ids[q]) - 1 and r["member_bits"].count(None) == 1
        frag = launch.refs.seq(launch.fam_ids[q][r["member_bits"].index(None)])
        assert int(frag[0] & 0xFFFFFF) > int(r["packed"][-1] & 0xFFFFFF)
    # iupac_and_case: ambiguity codes and lower-case bases on both sides of the comparison
    launches = ic.group("iupac_and_case")
    for launch, ref in launches:
        for q, r in enumerate(ref):
            masks = (np.asarray(r["packed"], np.uint32) >> 24) & 0x1F
            amb = int(sum(bin(int(m) & 0xF).count("1") > 1 for m in masks))
            assert amb >= 20, (launch.name, q)
            mem = (launch.refs.seq(launch.fam_ids[q][0]) >> 24) & 0x1F
            assert int((mem & 0x10 != 0).sum()) >= 20 and int(sum(bin(int(m) & 0xF).count("1") > 1 for m in mem)) >= 20
    lower = [int((((np.asarray(r["packed"], np.uint32) >> 24) & 0x10) != 0).sum()) for _, ref in launches for r in ref]
    assert max(lower) >= 20      # (--lowercase=original keeps the case)
    # overhang: three different finished sequences per query, fewer words than bases under remove
    (la, ra), (lr, rr), (le, re_) = ic.group("overhang")
    assert (la.opts["overhang"], lr.opts["overhang"], le.opts["overhang"]) == (0, 1, 2)
    for q in range(len(ra)):
        words = [np.asarray(x[q]["packed"], np.uint32) for x in (ra, rr, re_)]
        assert len(words[1]) < len(la.qmasks[q]) and len(words[0]) == len(words[2]) == len(la.qmasks[q])
        assert not np.array_equal(words[0] & 0xFFFFFF, words[2] & 0xFFFFFF)
    # unassembled: both kinds
    (launch, ref), = ic.group("unassembled")
    assert sum(1 for r in ref if r["must"]) >= 2 and sum(1 for r in ref if not r["must"]) >= 2
    assert all(r["full_row"][1] > 0 for r in ref if not r["must"])      # (zeros there are the rule, not the score)
    # ranges: at least nine queries, a family shared across the chunk boundary of fam_chunk_q=4
    (launch, ref), = ic.group("ranges")
    assert len(ref) >= 9 and launch.fam_ids[3] is launch.fam_ids[4] and all(r["must"] for r in ref)
    assert any(k.get("fam_chunk_q") == 4 for k in ic.RANGES_KNOBS) and any(k.get("dp_range_q") == 3 for k in ic.RANGES_KNOBS)
    assert len({r["row"] for r in ref}) >= 6
    # widest
    (launch, ref), = ic.group("widest")
    assert launch.width == 524288 and ref[0]["must"] and int(launch.refs.seq(0)[-1] & 0xFFFFFF) == 524287
    # the other entries' launches
    assert ic.group("profiles")[0][0].opts == dict(fs_no_graph=1)
    (launch, ref), = ic.group("wsets")
    assert sorted(set(launch.sets.tolist())) == [0, 1]
