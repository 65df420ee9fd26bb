"""CPU side of the search stage's device ranking (search option device-rank): tests/rank_ref.py pinned to the host
stage's comparator (score bits, all nine cover rules) and to the reference's search (order, on the stage-level worlds,
through the oracle); the grid arithmetic of sina_amd/csrc/rank_plan.h in a stand-alone program under the address and
undefined-behaviour sanitizers, and its Python mirror; the additions to the C ABI; the stage option; and the
precondition of the GPU tests: the number of queries that must come back flagged, per world.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sina_amd import capi, pipeline
from tests import compare_cases as cc
from tests import msc_cases as mc
from tests import rank_cases as rc
from tests import rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cover_rules_are_the_abis():
    assert rank_ref.COVERS == capi.COVER_RULES
    header = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    for i, name in enumerate(rank_ref.COVERS):
        assert re.search(r"#define SINA_CMP_COVER_%s %d\b" % (name.upper(), i), header), name
    stages = open(os.path.join(ROOT, "sina_amd", "csrc", "host", "stages.h")).read()
    order = re.search(r"enum CMP_COVER_TYPE \{([^}]*)\}", stages).group(1)
    assert [x.strip() for x in order.split(",")] == ["CMP_COVER_" + n.upper() for n in rank_ref.COVERS]


@pytest.mark.parametrize("world", [n for n in cc.NAMES if n not in ("rank_top", "lds_wide", "lds_limit", "nq_600")])
def test_score_bits_equal_the_host_stages(world):
    """rank_ref.score is cseq_comparator::score, bit for bit, on every pair of compare_cases that can be written as two
    aligned strings, for all nine cover rules: the counters are the host's, and 0 / 0 is NaN there and None here."""
    width, refs, qs, cand = cc.case(world)
    rstr = [mc.aligned_text(r, width) for r in refs]
    rows = cc.expected(world)[0, False]
    at, n = 0, 0
    for q, ids in zip(qs, cand):
        qstr = mc.aligned_text(q, width)
        for i in ids:
            row = rows[at]
            at += 1
            if qstr is None or rstr[int(i)] is None or n >= 400:
                continue
            for cover in range(9):
                score, counts = pipeline.host_compare(qstr, rstr[int(i)], 0, 0, cover, False)
                assert tuple(counts) == tuple(int(x) for x in row)
                want = rank_ref.score(row, cover)
                if want is None:
                    assert np.isnan(score) and rank_ref.denom(row, cover) == 0 and row[4] == 0
                else:
                    assert np.float32(score).tobytes() == np.float32(want).tobytes(), (world, cover, score, want)
            n += 1


def test_score_is_pinned_on_enough_pairs():
    n = 0
    for world in ("ranges", "filter", "cand_lists", "nq_1"):
        width, refs, qs, cand = cc.case(world)
        rstr = [mc.aligned_text(r, width) for r in refs]
        n += sum(1 for q, ids in zip(qs, cand) for i in ids if mc.aligned_text(q, width) is not None and rstr[int(i)] is not None)
    assert n > 100


def test_order_and_key(oracle):
    """Non-negative float32 scores order like their bit patterns; the order is (score, name) descending; name_order is
    byte-wise."""
    xs = np.array([0.0, 1e-45, 1e-10, 0.5, 0.99999994, 1.0, 1.0000001, 2.0, 65535.0], np.float32)
    assert (np.diff(xs.view(np.uint32).astype(np.int64)) > 0).all() and rank_ref.bits(np.float32(0.0)) == 0
    names = ["ref2", "ref10", "Ref3", "ref1", "ref", "ref\xc3"]
    rank = rank_ref.name_order(names)
    assert [names[i] for i in np.argsort(rank)] == ["Ref3", "ref", "ref1", "ref10", "ref2", "ref\xc3"]
    rows = [(0, 0, 0, 0, 5, 5)] * 4 + [(0, 0, 0, 0, 6, 4), (0, 0, 0, 0, 0, 0)]
    ids, sb, flag = rank_ref.rank_query(rows, [0, 1, 2, 3, 4, 5], rank, "query", 3)
    assert ids == [4, 0, 1] and flag == 1 and sb[0] > sb[1] == sb[2]


@pytest.mark.parametrize("name", rc.NAMES)
def test_directed_cases_reach_their_edges(name):
    """Building a case runs its builder's assertions; the declared number of flagged queries is rank_ref's."""
    case = rc.case(name)
    ids, sb, n, flag = rc.expected(name)
    assert int(flag.sum()) == case["flagged"]
    lists = rc.lists_of(case)
    for q in range(len(lists)):
        left_out = sum(1 for r in cc.walk_all(case["refs"], [case["qs"][q]], [lists[q]], case["rule"], case["flc"])
                       if rank_ref.denom(r, case["cover"]) == 0)
        assert n[q] == min(case["n_best"], len(lists[q]) - left_out) and (left_out > 0) == bool(flag[q])
    if case["chunk"]:
        m = max(len(x) for x in lists)
        assert rc.plan(len(lists), m, 256, forced=case["chunk"])[1] > 1


@pytest.mark.parametrize("world", rc.CC_WORLDS)
def test_flagged_queries_of_the_compare_worlds(oracle, world):
    """The precondition of test_gpu_rank.py's matrix: per cover rule and setting, the queries rank_ref flags are those
    with a candidate whose score the reference's own cseq_comparator gives as NaN."""
    width, refs, qs, cand = cc.case(world)
    assert width >= 90
    total = 0
    for rule, flc in cc.SETTINGS:
        rows = cc.expected(world)[rule, flc]
        for cover in range(9):
            flag = rc.cc_expected(world, cover, rule, flc, 3)[3]
            at = 0
            for q, ids in enumerate(cand):
                nan = any(np.isnan(oracle.compare_score(rows[at + x], rank_ref.COVERS[cover])) for x in range(len(ids)))
                at += len(ids)
                assert bool(flag[q]) == nan, (world, rule, flc, cover, q)
            total += int(flag.sum())
    if world in ("filter", "ranges"):
        assert total > 0                     # (a side that the filter empties, ranges that do not meet)


@pytest.mark.parametrize("name", rc.STAGE_NAMES)
def test_stage_worlds_against_the_reference(oracle, name):
    """The precondition of test_gpu_rank_stage.py, and the pin of rank_ref's ORDER: on every stage-level world the
    reference's search (the oracle) returns rank_ref's rows from its own counters (asserted inside
    stage_reference_run); the cover rules that must run without a fallback have no NaN among any query's candidates,
    and the fragment worlds have some."""
    run = rc.stage_reference_run(name)
    searched = [r for r in run if r is not None]
    flagged = sum(1 for r in searched if r["nan"])
    assert len(searched) >= 10 and sum(len(r["ids"]) for r in searched) > 0
    if name.endswith("_fragments"):
        assert 0 < flagged
        assert name != "nogap_fragments" or flagged < len(searched)      # some queries stay on the device too
    else:
        assert flagged == 0


def test_repeat_pick_repeats_a_flagged_query(oracle):
    """The precondition of test_gpu_rank_stage.py's test of repeated queries: 30 trays, 12 distinct queries, and among
    the fragments' a query that the reference flags (a NaN among its candidates' scores) is picked more than once --
    so is one that it does not flag."""
    for kind, name in rc.REPEAT_STAGE.items():
        distinct, pick = rc.stage_repeat_pick(kind)
        assert len(pick) == 30 and len(distinct) == 12 and sorted(set(pick.tolist())) == distinct.tolist()
        run = rc.stage_reference_run(name)
        times = np.bincount(pick, minlength=len(run))
        assert all(run[q] is not None for q in distinct)
        flagged = [int(q) for q in distinct if run[q]["nan"]]
        if kind == "fragments":
            assert any(times[q] >= 2 for q in flagged)
            assert any(times[q] >= 2 for q in distinct if not run[q]["nan"])
        else:
            assert not flagged


def test_rank_plan_against_plain_arithmetic(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "rank_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "sina_amd", "csrc"), os.path.join(ROOT, "tests", "rank_plan_check.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert run.returncode == 0 and "rank_plan_check: ok" in run.stdout, run.stdout[-4000:]
    for nq, M, cu, forced in ((9216, 1000, 256, 0), (64, 100000, 256, 0), (1, 10, 256, 3), (2, 13, 256, 4), (600, 1, 256, 0),
                              (3, 257, 304, 0), (0x7FFFFFFF, 1000, 256, 3), (0, 5, 256, 0), (5, 0, 256, 0), (1, 11, 1, 4)):
        out = subprocess.run([exe, str(nq), str(M), str(cu), str(forced)], stdout=subprocess.PIPE, text=True, env=env,
                             check=True).stdout
        assert tuple(int(x) for x in out.split()) == rc.plan(nq, M, cu, forced=forced), (nq, M, cu, forced, out)
    plan = open(os.path.join(ROOT, "sina_amd", "csrc", "rank_plan.h")).read()
    assert "kRankChunkFloor = 128" in plan and "kRankWgPerCu = 4" in plan and "kRankMaxResult = %d" % rc.MAX_BEST in plan
    assert "#include <hip" not in plan and "hip_runtime" not in plan and capi.RANK_MAX_RESULT == rc.MAX_BEST


def test_abi_additions():
    header = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    protos = {
        "sina_hip_upload_name_order": "int sina_hip_upload_name_order(sina_hip_ctx *ctx, const uint32_t *rank, uint32_t n);",
        "sina_hip_compare_rank": "int sina_hip_compare_rank(sina_hip_ctx *ctx, const uint32_t *q_ab, const uint64_t *q_off, "
                                 "uint32_t nq, const uint32_t *cand_ids, const uint64_t *cand_off, int iupac_rule, "
                                 "int filter_lowercase, int cover_rule, uint32_t max_result, uint32_t *out_ids, "
                                 "float *out_scores, uint32_t *out_n, uint32_t *out_flag);",
        "sina_hip_kmer_topk_rank": "int sina_hip_kmer_topk_rank(sina_hip_ctx *ctx, const uint32_t *q_ab, const uint64_t *q_off, "
                                   "uint32_t nq, uint32_t kmer_candidates, int iupac_rule, int filter_lowercase, "
                                   "int cover_rule, uint32_t max_result, uint32_t *out_ids, float *out_scores, "
                                   "uint32_t *out_n, uint32_t *out_flag);",
        "sina_hip_rank_stats": "int sina_hip_rank_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *pairs, "
                               "uint64_t *cand_bases, uint64_t *launches);",
    }
    stub = open(os.path.join(ROOT, "tools", "hoststub", "fake_hip.cpp")).read()
    L = capi.load()
    for sym, proto in protos.items():
        assert proto in flat, sym
        assert sym in capi.ABI_SYMBOLS and hasattr(L, sym)
        assert re.search(r"\bint %s\(" % sym, stub)
        assert getattr(L, sym).argtypes is not None
    for method in ("upload_name_order", "compare_rank", "kmer_topk_rank", "rank_stats"):
        assert callable(getattr(capi.Context, method))
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", header) and L.sina_hip_abi_version() == 5
    # no struct changed; the new kernel is its own file, shares the tables with compare_kernel, and the build has no
    # fast-math flag (the score is one correctly rounded division)
    assert "} sina_hip_match_counts;" in header and "} sina_hip_stats;" in header
    src = open(os.path.join(ROOT, "sina_amd", "csrc", "rank.hip")).read()
    assert "rank_kernel" in src and "rank_merge_kernel" in src and "build_query_tables" in src and "asm" not in src
    assert "build_query_tables" in open(os.path.join(ROOT, "sina_amd", "csrc", "search.hip")).read()
    make = open(os.path.join(ROOT, "sina_amd", "csrc", "Makefile")).read()
    assert "$(B)/rank.o" in make and "fast-math" not in make and "-Ofast" not in make


def test_search_takes_device_rank():
    H = pipeline.load_host()
    H.sina_host_reset_options()
    try:
        assert H.sina_host_set_option(b"search", b"device-rank", b"1") == 0
        assert H.sina_host_set_option(b"search", b"device-rank", b"0") == 0
        assert H.sina_host_set_option(b"search", b"device-rnak", b"1") != 0
        assert b"unknown option device-rnak" in H.sina_host_last_error()
    finally:
        H.sina_host_reset_options()
    assert hasattr(H, "sina_host_store_rank_stats") and callable(pipeline.Store.rank_stats)
