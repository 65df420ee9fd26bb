"""CPU side of the device identity filter (famfinder's --fs-msc-max on the GPU): the identity reduction the match-count
kernel rests on, checked with the plain walk on every case of tests/msc_cases.py and tests/compare_cases.py and against
the host stage's own comparator; the grid arithmetic of sina_amd/csrc/match_plan.h in a stand-alone program under the
address and undefined-behaviour sanitizers, and its Python mirror; the additions to the C ABI; the famfinder option;
and the precondition of tests/test_gpu_leaveout.py.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sina_amd import capi, pipeline
from tests import compare_cases as cc
from tests import compare_ref
from tests import msc_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_reduction(refs, qs, cand, rows):
    """match + mismatch + only_a + only_a_overhang == |A| whenever both sides have a base (else six zeros), and the
    match column is the set-arithmetic count."""
    at = 0
    for q, ids in zip(qs, cand):
        for i in ids:
            r = refs[int(i)]
            oa_over, ob_over, oa, ob, match, mismatch = (int(x) for x in rows[at])
            if len(q) and len(r):
                assert match + mismatch + oa + oa_over == len(q), (at, rows[at], len(q))
            else:
                assert (oa_over, ob_over, oa, ob, match, mismatch) == (0,) * 6
            assert match == mc.match_ref(q, r) <= min(len(q), 65535)
            at += 1
    assert at == len(rows)


@pytest.mark.parametrize("name", mc.NAMES)
def test_identity_reduction_msc_cases(name):
    """Building a case runs its builder's assertions."""
    width, refs, qs, cand = mc.case(name)
    _check_reduction(refs, qs, cand, mc.expected(name))


@pytest.mark.parametrize("name", cc.NAMES)
def test_identity_reduction_compare_cases(name):
    width, refs, qs, cand = cc.case(name)
    _check_reduction(refs, qs, cand, cc.expected(name)[0, False])


@pytest.mark.parametrize("seed", range(int(os.environ.get("SINA_FUZZ_SEEDS", "12"))))
def test_identity_reduction_fuzz(seed):
    width, refs, qs, cand = cc.fuzz_case(seed)
    _check_reduction(refs, qs, cand, cc.expected("fuzz", seed)[0, False])


def test_identity_equals_the_host_stages_score():
    """float32(match) / float32(|A|) is the score of the host stage's comparator (optimistic, no distance correction,
    cover query, no filter) -- bit for bit -- on every pair that can be written as two aligned strings; an empty side
    gives 0, not 0 / 0."""
    n = 0
    for name in mc.NAMES:
        width, refs, qs, cand = mc.case(name)
        if name.startswith("list_chunks") or name == "ragged":
            cand = [ids[:3] for ids in cand[:8]]            # (the same few sequences over and over)
            qs = qs[:8]
        rstr = [mc.aligned_text(r, width) for r in refs]
        for q, ids in zip(qs, cand):
            qstr = mc.aligned_text(q, width)
            for i in ids:
                if qstr is None or rstr[int(i)] is None or not len(q) or not len(refs[int(i)]):
                    continue
                score, counts = pipeline.host_compare(qstr, rstr[int(i)], 0, 0, 1, False)
                want = np.float32(mc.match_ref(q, refs[int(i)])) / np.float32(len(q))
                assert counts[4] == mc.match_ref(q, refs[int(i)])
                assert np.float32(score).tobytes() == np.float32(want).tobytes(), (name, score, want)
                n += 1
    assert n > 60


def test_match_plan_against_plain_arithmetic(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "match_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "sina_amd", "csrc"), os.path.join(ROOT, "tests", "match_plan_check.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert run.returncode == 0 and "match_plan_check: ok" in run.stdout, run.stdout[-4000:]
    # ... and the mirror the chunk cases are built with
    for nq, M, cu in ((1, 41000, 256), (3, 65, 256), (3, 65, 1), (512, 131, 256), (608, 131, 304), (1000, 41000, 256),
                      (5, 41, 256), (0x7FFFFFFF, 1000, 256), (0, 5, 256), (5, 0, 256), (16384, 128, 256)):
        out = subprocess.run([exe, str(nq), str(M), str(cu)], stdout=subprocess.PIPE, text=True, env=env, check=True).stdout
        assert tuple(int(x) for x in out.split()) == mc.plan(nq, M, cu), (nq, M, cu, out)
    plan = open(os.path.join(ROOT, "sina_amd", "csrc", "match_plan.h")).read()
    assert "kMatchChunkFloor = %d" % mc.CHUNK_FLOOR in plan and "kMatchWgPerCu = %d" % mc.WG_PER_CU in plan
    assert "#include <hip" not in plan and "hip_runtime" not in plan
    assert 4 * ((mc.MAX_WIDTH + 7) // 8) == 160 * 1024


def test_abi_additions():
    header = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    protos = {
        "sina_hip_match_count": "int sina_hip_match_count(sina_hip_ctx *ctx, const uint32_t *q_ab, const uint64_t *q_off, "
                                "uint32_t nq, const uint32_t *cand_ids, const uint64_t *cand_off, uint16_t *out_match);",
        "sina_hip_kmer_topk_match": "int sina_hip_kmer_topk_match(sina_hip_ctx *ctx, const uint32_t *q_ab, const uint64_t *q_off, "
                                    "uint32_t nq, uint32_t max, uint32_t *out_ids, float *out_scores, uint32_t *out_n, "
                                    "uint16_t *out_match);",
        "sina_hip_match_stats": "int sina_hip_match_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *pairs, "
                                "uint64_t *cand_bases, uint64_t *launches);",
    }
    stub = open(os.path.join(ROOT, "tools", "hoststub", "fake_hip.cpp")).read()
    L = capi.load()
    for sym, proto in protos.items():
        assert proto in flat, sym
        assert sym in capi.ABI_SYMBOLS and hasattr(L, sym)
        assert re.search(r"\bint %s\(" % sym, stub)
    for method in ("match_counts", "kmer_topk_match", "match_stats"):
        assert callable(getattr(capi.Context, method))
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", header) and L.sina_hip_abi_version() == 5
    # no struct changed: the counters' type is still there, and the new kernel is its own file with its own table
    assert "} sina_hip_match_counts;" in header
    src = open(os.path.join(ROOT, "sina_amd", "csrc", "match.hip")).read()
    assert "match_count_kernel" in src and "compare_kernel" not in src and "asm" not in src


def test_famfinder_takes_device_msc():
    H = pipeline.load_host()
    H.sina_host_reset_options()
    try:
        assert H.sina_host_set_option(b"famfinder", b"device-msc", b"1") == 0
        assert H.sina_host_set_option(b"famfinder", b"device-msc", b"0") == 0
        assert H.sina_host_set_option(b"famfinder", b"device-mcs", b"1") != 0
        assert b"unknown option device-mcs" in H.sina_host_last_error()
    finally:
        H.sina_host_reset_options()
    assert hasattr(H, "sina_host_pipeline_run_aligned") and hasattr(H, "sina_host_store_match_stats")
    assert callable(pipeline.Pipeline.run_aligned) and callable(pipeline.Store.match_stats)


def test_leaveout_world_escalates(oracle):
    """The precondition of tests/test_gpu_leaveout.py: two clades, identity above 0.9 inside and at most 0.9 across
    (every pair, by table look-up, pinned to the plain walk on a sample); the dense clade has more than 410 members;
    for every member query the top 41 and the top 410 by the oracle's k-mer score are all above 0.9 -- the cascade
    must widen to the whole store --, where at least fs-min long-enough candidates at or below 0.9 wait."""
    from tests import util
    refs, dense, clade = mc.leaveout_world()
    names, seqs, kinds = mc.leaveout_queries()
    sizes = np.diff(refs.off)
    assert (clade == 0).sum() > 411 and (clade == 1).sum() >= mc.LO_FS_MIN and (sizes >= mc.LO_FULL_LEN).all()
    for i in range(refs.n):
        ident = mc.identities(dense, refs.seq(i))
        same = clade == clade[i]
        assert (ident[same] > mc.LO_MSC_MAX).all() and (ident[~same] <= mc.LO_MSC_MAX).all(), i
    rng = np.random.default_rng(5)
    for a, b in rng.integers(0, refs.n, size=(40, 2)):
        got = mc.walk_identity(refs.seq(int(a)), refs.seq(int(b)))
        assert got.tobytes() == mc.identities(dense, refs.seq(int(a)))[int(b)].tobytes()
    cs = util.cseqs_from_refs(refs)
    idx = oracle.Index(cs, k=10)
    for name, q, kind in zip(names, seqs, kinds):
        if kind != "member":
            continue
        ident = mc.identities(dense, q)
        oq = oracle.Cseq.from_packed(name, q, refs.width)
        for top in (41, 410):
            ids, _ = idx.find(oq, top)
            assert len(ids) == top and (ident[ids] > mc.LO_MSC_MAX).all(), (name, top)
        assert ((ident <= mc.LO_MSC_MAX) & (sizes >= mc.LO_MIN_LEN)).sum() >= mc.LO_FS_MIN
    # the shifted copy matches next to nothing, its twin nearly everything of its clade
    assert mc.identities(dense, seqs[-1]).max() < 0.1 and kinds[-1] == "shifted"
