"""CPU side of the in-place ranking (tests/test_gpu_search_inplace.py runs it): the three added entries through every
layer that names them, the ABI version left as it was, align_plan.h's plan_search_inplace as a sanitized stand-alone
program, and the conditions on the GPU test's inputs -- checked here with the oracle, so that the GPU test cannot pass
on inputs that show nothing."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from sina_amd import capi, pipeline
from tests import identity_cases as ic, rank_cases as rc, rank_ref, search_inplace_cases as sic, shift_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sina_hip_align_rank", "sina_hip_staged_rank", "sina_hip_rank_inplace_stats")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", text)
    assert re.search(r"\bint sina_hip_align_rank\(sina_hip_ctx \*ctx, int on, unsigned k, int nofast, uint32_t kmer_candidates, "
                     r"int iupac_rule,\s+int filter_lowercase, int cover_rule, uint32_t max_result\);", text)
    assert re.search(r"\bconst uint32_t \*sina_hip_staged_rank\(sina_hip_ctx \*ctx\);", text)
    assert re.search(r"\bint sina_hip_rank_inplace_stats\(sina_hip_ctx \*ctx, double \*kernel_ms, uint64_t \*sequences, "
                     r"uint64_t \*pairs,\s+uint64_t \*launches\);", text)
    L = capi.load()
    assert L.sina_hip_abi_version() == 5
    for sym in NEW:
        assert sym in capi.ABI_SYMBOLS and hasattr(L, sym), sym
    assert len(L.sina_hip_align_rank.argtypes) == 9
    assert L.sina_hip_staged_rank.argtypes == [C.c_void_p] and L.sina_hip_staged_rank.restype == C.POINTER(C.c_uint32)
    assert len(L.sina_hip_rank_inplace_stats.argtypes) == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "sina_amd", "libsina_hip.so")],
                        stdout=subprocess.PIPE, text=True, check=True).stdout
    for sym in NEW:
        assert re.search(r" T %s$" % sym, nm, re.M), sym
    assert C.sizeof(capi.AlignOut) == 52 and C.sizeof(capi.AlignParams) == 48      # no struct of the header changes
    assert capi.RANK_ROW_WORDS == sic.ROW_WORDS == 2 + 2 * sic.MAX_BEST


def test_stub_documents_and_plan_name_the_entries():
    stub = open(os.path.join(ROOT, "tools", "hoststub", "fake_hip.cpp")).read()
    docs = {n: open(os.path.join(ROOT, n)).read() for n in ("README.md", "DESIGN.md", "INTEGRATION.md")}
    for sym in NEW:
        assert re.search(r"\b%s\(sina_hip_ctx \*" % sym, stub), sym
        for n, doc in docs.items():
            assert sym in doc, (sym, n)
    for n, doc in docs.items():
        assert "device-search" in doc, n
    assert "3.5d" in docs["DESIGN.md"]
    plan = open(os.path.join(ROOT, "sina_amd", "csrc", "host", "align_plan.h")).read()
    assert "plan_search_inplace" in plan
    # plan_counting's signature stays: tests/align_plan_check.cpp compiles unchanged
    assert "plan_counting(const align_switches &s, align_route route, bool batch_driver, bool has_pair_map, bool assembles)" in plan


def test_wrappers_and_option():
    for name in ("rank_assembled", "staged_rank", "rank_inplace_stats"):
        assert callable(getattr(capi.Context, name)), name
    assert callable(pipeline.Store.search_inplace_stats)
    H = pipeline.load_host()
    assert hasattr(H, "sina_host_store_search_inplace_stats")
    H.sina_host_reset_options()
    try:
        assert H.sina_host_set_option(b"aligner", b"device-search", b"1") == 0
        assert H.sina_host_set_option(b"aligner", b"device-search", b"0") == 0
        assert H.sina_host_set_option(b"aligner", b"device-serch", b"1") != 0
    finally:
        H.sina_host_reset_options()


def test_null_context_is_refused_by_name():
    L = capi.load()
    assert L.sina_hip_align_rank(None, 1, 10, 0, 1000, 0, 0, 1, 10) != 0
    assert b"align_rank" in L.sina_hip_last_error()
    assert not L.sina_hip_staged_rank(None)
    assert b"staged_rank" in L.sina_hip_last_error()
    ms, a, b, c = C.c_double(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.sina_hip_rank_inplace_stats(None, C.byref(ms), C.byref(a), C.byref(b), C.byref(c)) != 0
    assert b"rank_inplace_stats" in L.sina_hip_last_error()


def test_search_plan_check_program(tmp_path):
    """tests/search_plan_check.cpp: every precondition of plan_search_inplace, sanitized, as its own process."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "search_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "sina_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "search_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert run.returncode == 0 and "search_plan_check: ok" in run.stdout, run.stdout[-4000:]


@pytest.mark.parametrize("name", sorted(sic.GROUPS))
def test_inputs_are_worth_running(oracle, name):
    """Every launch: a ranked query's finished sequence has every input base in strictly ascending columns below the
    width; its row has min(N, candidates) entries, best first by (score bits, name rank), with ids among its
    candidates; rows differ between queries; an unranked query's row is zero although it would have had rows."""
    for launch, ref in sic.group(name):
        s = launch.search
        name_rank = rank_ref.name_order(launch.names)
        assert len(ref) == len(launch.qmasks) == len(launch.fam_ids) and launch.stride >= 1
        for q, r in enumerate(ref):
            assert r["ranked"] == (r["must"] and r["kept"]), (launch.name, q)
            assert len(r["cand"]) == launch.stride and len(set(r["cand"].tolist())) == launch.stride, (launch.name, q)
            full = r["full"]
            n = int(full[0])
            assert n <= s["n_best"] and (full[2 + n:2 + sic.MAX_BEST] == 0).all() and (full[2 + sic.MAX_BEST + n:] == 0).all()
            if not full[1] & sic.NAN:
                assert n == min(s["n_best"], launch.stride), (launch.name, q)
            ids, bits = full[2:2 + n].tolist(), full[2 + sic.MAX_BEST:2 + sic.MAX_BEST + n].tolist()
            assert set(ids) <= set(r["cand"].tolist())
            keys = [(b, int(name_rank[i])) for i, b in zip(ids, bits)]
            assert keys == sorted(keys, reverse=True), (launch.name, q)
            if not r["ranked"]:
                assert not r["row"].any() and n > 0, (launch.name, q)
                continue
            cols = (np.asarray(r["packed"], np.uint32) & 0xFFFFFF).astype(np.int64)
            assert len(cols) == len(launch.qmasks[q]) and (np.diff(cols) > 0).all() and cols[-1] < launch.width, (launch.name, q)
            assert np.array_equal(r["row"], full)
        ranked = [r for r in ref if r["ranked"]]
        if len(ranked) > 1:
            assert len({r["row"].tobytes() for r in ranked}) > 1, launch.name


def test_directed_conditions(oracle):
    # cands: the counts of the issue around N = 10 and the four waves, and a max beyond the store that clamps
    launches = sic.group("cands")
    assert [l.search["cands"] for l, _ in launches] == [1, 3, 4, 5, 9, 10, 11, 1000] and all(l.search["n_best"] == 10 for l, _ in launches)
    assert [l.stride for l, _ in launches] == [1, 3, 4, 5, 9, 10, 11, launches[0][0].refs.n]
    assert rc.WAVES == 4 and sum(1 for r in launches[0][1] if r["ranked"]) >= 3
    # (with one more candidate than N the one left out is not simply the last of the k-mer search's list)
    (l11, r11) = launches[6]
    assert any(r["ranked"] and int(r["cand"][-1]) in r["full"][2:12].tolist() for r in r11)
    # n_best: 1, 10 and 64 rows out of 160 candidates
    assert [(l.search["n_best"], int(ref[0]["full"][0])) for l, ref in sic.group("n_best")] == [(1, 1), (10, 10), (64, 64)]
    # covers: each rule once, all three iupac rules and the lower-case filter among them; the rules order differently
    launches = sic.group("covers")
    assert [l.search["cover"] for l, _ in launches] == list(rank_ref.COVERS)
    assert {l.search["rule"] for l, _ in launches} == {0, 1, 2} and {l.search["flc"] for l, _ in launches} == {False, True}
    assert len({ref[0]["row"][2:12].tobytes() for _, ref in launches}) >= 3
    # no_hit: not one reference shares a 10-mer with the query -- its candidates are the store's last references
    (launch, ref), = sic.group("no_hit")
    cs, idx = sic._index(launch.refs, 10)
    assert not idx.scores(ic._cseq("q", launch.qmasks[0])).any() and idx.scores(ic._cseq("q", launch.qmasks[1])).any()
    n = launch.refs.n
    assert ref[0]["ranked"] and sorted(ref[0]["cand"].tolist()) == list(range(n - launch.stride, n))
    # tie: eight equal scores straddle place N, the name decides, and the name order is not the id order
    (launch, ref), = sic.group("tie")
    full, N = ref[0]["full"], launch.search["n_best"]
    ids, bits = full[2:2 + N].tolist(), full[2 + sic.MAX_BEST:2 + sic.MAX_BEST + N].tolist()
    assert ref[0]["ranked"] and int(full[0]) == N and len(set(bits[-3:])) == 1 and (N == 3 or bits[-4] != bits[-3])
    assert ids[-3:] == [7, 166, 165] and launch.names[7].encode() > launch.names[166].encode()
    assert sorted([7] + list(range(160, 167)), reverse=True)[:3] != ids[-3:]
    # nan: a k-mer candidate without a score sets bit 0, and the row still carries the others
    (launch, ref), = sic.group("nan")
    for q, r in enumerate(ref):
        assert r["ranked"] and int(r["row"][1]) == sic.RANKED | sic.NAN and launch.refs.n - 2 + q in r["cand"].tolist()
        assert launch.refs.n - 2 + q not in r["row"][2:12].tolist()
    # overhang_remove: bases are dropped, and the aligned sequence's k-mers are not the input's
    (launch, ref), = sic.group("overhang_remove")
    assert launch.opts["overhang"] == 1
    for q, r in enumerate(ref):
        L = len(launch.qmasks[q])
        assert r["must"] and not r["kept"] and not r["ranked"] and len(r["packed"]) < L
        q_in = np.arange(L, dtype=np.uint32) | (launch.qmasks[q].astype(np.uint32) << 24)
        k_in, k_al = po.kmers(q_in, 10), po.kmers(np.asarray(r["packed"], np.uint32), 10)
        assert len(k_al) < len(k_in) and sorted(k_in.tolist()) != sorted(k_al.tolist())
    # unassembled: both kinds in one launch; shifted: assemble = 2 over a world whose queries have shifted runs
    (launch, ref), = sic.group("unassembled")
    assert sum(1 for r in ref if r["ranked"]) >= 2 and sum(1 for r in ref if not r["must"]) >= 2
    launches = sic.group("shifted")
    assert [l.assemble for l, _ in launches] == [2, 2] and [l.search["flc"] for l, _ in launches] == [False, True]
    w = sc.dp_world()
    assert sum(1 for x in w["want"] if sc.log_events(x["log"])) * 2 >= len(w["want"])
    for q, (a, b) in enumerate(zip(launches[0][1], launches[1][1])):
        assert np.array_equal(a["packed"], w["want"][q]["packed"]) and a["ranked"] and b["ranked"]
    lower = [int((((np.asarray(r["packed"], np.uint32) >> 24) & 0x10) != 0).sum()) for r in launches[0][1]]
    assert sum(1 for x in lower if x > 0) >= 4                      # (--lowercase unaligned lower-cases the shifted bases)
    assert any(not np.array_equal(a["row"], b["row"]) for a, b in zip(launches[0][1], launches[1][1]))
    # ranges: ten ranked queries, several launch ranges and several chunks (the merge launch) out of 160 candidates
    launches = sic.group("ranges")
    assert len(launches[0][1]) == 10 and all(r["ranked"] for r in launches[0][1]) and launches[0][0].knobs == {}
    assert [l.knobs for l, _ in launches[1:]] == list(sic.RANGES_KNOBS)
    assert rc.plan(10, 160, 256, forced=16) == (16, 10) and rc.plan(3, 160, 256, forced=16)[1] == 10 and rc.plan(10, 160, 256)[1] > 1
    for l, ref in launches[1:]:
        assert np.array_equal(sic.rows(ref), sic.rows(launches[0][1]))
    # the other entries' launches
    assert sic.group("profiles")[0][0].opts == dict(fs_no_graph=1)
    assert sorted(set(sic.group("wsets")[0][0].sets.tolist())) == [0, 1]


def test_stage_worlds_have_dp_trays_to_rank(oracle):
    """The stage worlds of tests/rank_cases.py: at least ten queries per world that the oracle aligns by DP (not the
    copy shortcut) and searches -- the trays the device must assemble and rank in place."""
    from tests import util
    for kind, n_refs in (("full", 300), ("fragments", 300), ("full", 150)):
        refs, qs = rc.stage_refs(n_refs), rc.stage_queries(kind, n_refs)
        cs = util.cseqs_from_refs(refs)
        idx = po.Index(cs, k=10)
        dp = 0
        for qi in range(qs.n):
            q = util.query_cseq(qs, qi, upper=False)
            ids, _, _ = idx.famfinder(q, po.ff_opts(fs_min_len=100, fs_full_len=250))
            al = po.align([cs[i] for i in ids], q, po.align_opts(realign=1)) if len(ids) else None
            dp += al is not None and al["status"] == 0 and len(al["packed"]) >= 20
        assert dp >= 10, (kind, n_refs, dp)
