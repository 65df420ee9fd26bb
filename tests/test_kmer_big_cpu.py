"""CPU side of the big select (more than 4096 candidates per query): tests/kmer_ref.py pinned to the oracle at such
sizes, every case of tests/kmer_big_cases.py built (which runs its builder's assertions) and asked again for the edge it
names, the search call's plan -- sina_amd/csrc/kmer_plan.h -- in a stand-alone program under the address and
undefined-behaviour sanitizers, the additions to the C ABI, and the precondition of tests/test_gpu_escalation.py.  No
GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sina_amd import capi, pipeline, synth
from tests import kmer_big_cases as kb
from tests import kmer_cases as kc
from tests import kmer_ref, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ref_equals_oracle_beyond_4096(oracle):
    """kmer_ref.topk against the oracle's Index.find on a natural world of 5000 references, at max values on both
    sides of 4096, the whole store and beyond it."""
    refs = synth.make_refs(5000, length=120, width=1200, seed=9001, n_clades=4, long_del_prob=0.0)
    idx = oracle.Index(util.cseqs_from_refs(refs), k=8)
    off, ids = idx.csr()
    qs = synth.make_queries(refs, 3, seed=9002, amb_rate=0.02)
    for qi in range(qs.n):
        q = util.query_cseq(qs, qi)
        s = kmer_ref.scores(off, ids, refs.n, qs.seq(qi), 8, True)
        assert (s == idx.scores(q)).all()
        for mx in (4096, 4097, 4999, 5000, 5001):
            gi, gs = kmer_ref.topk(s, mx)
            oi, os_ = idx.find(q, mx)
            assert len(gi) == min(mx, refs.n) and (gi == oi).all() and (gs == os_).all(), (qi, mx)


@pytest.mark.parametrize("name", sorted(kb.BIG_CASES))
def test_case_reaches_its_edge(name):
    """Building a case runs check_csr and the builder's assertions; its rows are kmer_ref's."""
    c = kb.case(name)
    assert len(c.expected) == len(c.qmasks) == len(c.labels)
    for m, e in zip(c.qmasks, c.expected):
        assert (e["scores"] == kmer_ref.scores(c.off, c.ids, c.n_refs, m, c.k, not c.nofast)).all()
        for mx in c.maxes:
            wi, ws = kmer_ref.topk(e["scores"], mx)
            assert (e["find"][mx][0] == wi).all() and (e["find"][mx][1] == ws).all() and len(wi) == min(mx, c.n_refs)


def test_every_edge_has_its_case():
    # the seam: 4096 the old kernel, 4097 .. the new one, clipped at n_refs
    c = kb.seam()
    assert c.n_refs == 5000 and c.maxes == (4096, 4097, 4999, 5000, 5001, 100000)
    assert [kb.big_queries(c, mx) for mx in c.maxes] == [0, 2, 2, 2, 2, 2]
    assert [len(c.expected[0]["find"][mx][0]) for mx in c.maxes] == [4096, 4097, 4999, 5000, 5000, 5000]
    assert kb.big_queries(kb.fewer_refs(), 5000) == 0
    # where the first taken tie sits, with M > 4096 and more than 4096 ties at the cut
    t = kb.tie_split()
    where = {name: kb.first_tie_taken(t, 0, mx) for name, mx in t.tie_maxes.items()}
    assert {name: w[1] for name, w in where.items()} == kc.TIE_FIRST
    assert all(w[0] == 2 and w[2] > 4096 for w in where.values()) and min(t.maxes) > 4096
    assert kc.TIE_FIRST["wave_range"] == 640 * 8 and (kc.TIE_FIRST["iteration_end"] + 1) % 512 == 0
    assert kc.TIE_FIRST["mid_vector"] % 8 not in (0, 7) and kc.TIE_FIRST["last_only"] == t.n_refs - 1
    # the short cut's exits at M > 4096, and the two ways it is not tried
    s = kb.shortcut_exits()
    assert [kc._models(s, qi, kb.SHORTCUT_M)["exit"] for qi in range(3)] == ["found", "fewer", "unusable"]
    assert kb.SHORTCUT_M > 4096
    r = kb.shortcut_not_tried_rows()
    assert r.n_refs == 16376 and (r.n_refs + 7) // 8 == 2047 and kc._models(r, 0, kb.SHORTCUT_M) is None
    w = kb.shortcut_not_tried_windows()
    assert all(len(m) - w.k >= 8192 for m in w.qmasks) and kc._models(w, 0, kb.SHORTCUT_M) is None
    assert kc._models(kb.zeros_fill(), 0, 4500)["exit"] == "unusable"
    # everything taken
    for n in (32769, 65537):
        e = kb.everything(n)
        assert e.maxes == (n,) and e.expected[0]["find"][n][1][-1] == 0
    # the long query: scores above 10 240 at the cut
    lq = kb.long_query()
    assert kb.first_tie_taken(lq, 1, 5000)[0] == kc.LONG_MAX - lq.k > 10240
    sc2 = lq.expected[2]["find"][5000][1]
    assert sc2[0] > 10240 > sc2[-1] > 0                      # (the two-block query: the cut falls between its groups)
    assert kb.big_queries(lq, 5000) == 3 and kb.launches_model(lq, 5000) == 2


def test_range_seams_of_the_mixed_batch():
    """How many ranges each big_sel_bytes setting of the range-seam test cuts the mixed batch into."""
    c = kb.mixed_batch()
    assert len(c.qmasks) == 4 and kb.launches_model(c, kb.MIXED_M) == 1
    for name, (budget, want) in kb.seam_budgets().items():
        per, n = kb.ranges_model(4, kb.MIXED_M, budget)
        assert [min(per, 4 - q0) for q0 in range(0, 4, per)] == want and n == len(want), name
        assert kb.launches_model(c, kb.MIXED_M, budget) == len(want)
    assert kb.seam_budgets()["after_first"][1][0] == 1 and kb.seam_budgets()["after_third"][1][0] == 3
    # the default budget (1 GiB, 24 bytes per candidate)
    assert kb.ranges_model(100000, 4100) == (10912, 10) and kb.ranges_model(512, 100000) == (447, 2)
    assert kb.ranges_model(1 << 20, 1 << 20)[0] == 42


@pytest.mark.parametrize("seed", kb.fuzz_seeds(int(os.environ.get("SINA_FUZZ_SEEDS", "12"))))
def test_fuzz_big_world(seed):
    c = kb.fuzz_big(seed)
    assert c.n_refs > 4097 and len(c.maxes) == 3 and all(4097 <= mx <= c.n_refs + 10 for mx in c.maxes)
    assert all(kb.is_big(c.n_refs, mx) for mx in c.maxes)
    for e, we in zip(c.expected, kc.fuzz_world(seed).expected):
        assert e["scores"] is we["scores"]
        for mx in c.maxes:
            assert len(e["find"][mx][0]) == min(mx, c.n_refs)


def test_fuzz_seeds_are_the_large_worlds():
    got = kb.fuzz_seeds(12)
    assert got == [s for s in range(12) if kc.fuzz_world(s).n_refs > 4097] and len(got) >= 3


def test_abi_additions():
    header = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    sym = "sina_hip_big_select_queries"
    assert re.search(r"\bint %s\(sina_hip_ctx \*ctx, uint64_t \*n\);" % sym, header)
    assert sym in capi.ABI_SYMBOLS and hasattr(capi.load(), sym)
    assert callable(capi.Context.big_select_queries)
    assert hasattr(pipeline.load_host(), "sina_host_store_big_select_queries")
    assert callable(pipeline.Store.big_select_queries)
    stub = open(os.path.join(ROOT, "tools", "hoststub", "fake_hip.cpp")).read()
    assert re.search(r"\bint %s\(" % sym, stub)
    for unit in ("kmer.hip", "kmer_launch.hip"):                       # (the kernels' unit, the search call's driver)
        assert "not supported by the LDS select kernel" not in open(os.path.join(ROOT, "sina_amd", "csrc", unit)).read()
    plan = open(os.path.join(ROOT, "sina_amd", "csrc", "kmer_plan.h")).read()
    assert "kBigSelBudget = 1ull << 30" in plan and kb.BIG_BUDGET == 1 << 30
    assert "kBigSelBytesPerCand = %d" % kb.BIG_BYTES_PER_CAND in plan


def test_kmer_plan_against_plain_arithmetic(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "kmer_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "sina_amd", "csrc"), os.path.join(ROOT, "tests", "kmer_plan_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert run.returncode == 0 and "kmer_plan_check: ok" in run.stdout, run.stdout[-4000:]


def test_escalation_world_escalates(oracle):
    """The precondition of tests/test_gpu_escalation.py: for at least half of its sixteen queries neither the top 410
    nor the top 4100 by k-mer score hold the full-length relative famfinder asks for -- they go on to the whole store,
    through the big select --, the others are satisfied at once, and the oracle's famfinder finds a family for all."""
    refs, _, _ = kb.escalation_world()
    qs = kb.escalation_queries()
    assert refs.n == 6010 > 4100 and qs.n == 16
    sizes = np.diff(refs.off)
    cs = util.cseqs_from_refs(refs)
    idx = oracle.Index(cs, k=10)
    must = []
    for qi in range(qs.n):
        q = util.query_cseq(qs, qi, upper=False)
        s = idx.scores(q).astype(np.int64)
        at = [kb.satisfied_by_top(s, sizes, n) for n in (41, 410, 4100, refs.n)]
        assert at[3] and at == sorted(at)
        must.append(not at[2])
        ids, sc, log = idx.famfinder(q, oracle.ff_opts(**kb.ESC_FF))
        assert len(ids) >= 40 and "unable" not in log, (qi, log)            # no query fails softly
        assert (sizes[ids] >= 240).sum() >= 1
        if must[-1]:
            assert (s[ids[sizes[ids] >= 240]] == 0).all() and ids[sizes[ids] >= 240].max() == refs.n - 1
    assert sum(must) == 10 and must == [True] * 10 + [False] * 6
