"""CPU side of the device family cascade (famfinder's device-cascade): the additions to the C ABI and to the host
library; every predicate of tests/cascade_cases.py; the plain loop of tests/cascade_ref.py against the oracle's
famfinder on seeded random stores and option sets and on the leave-out world of tests/msc_cases.py, and against
msc_cases.leaveout_cascade; the two facts the kernel rests on (the family is bounded, the scan may stop early);
sina_amd/csrc/family_plan.h in a stand-alone program under the address sanitizer, and its Python mirror.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sina_amd import capi, pipeline, synth
from tests import cascade_cases as kc
from tests import cascade_ref as cr
from tests import msc_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = int(os.environ.get("SINA_FUZZ_SEEDS", "200"))


def test_abi_additions():
    header = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    protos = {
        "sina_hip_family_row_words": "int sina_hip_family_row_words(const sina_hip_family_rule *r, uint32_t *words);",
        "sina_hip_family_cascade": "int sina_hip_family_cascade(sina_hip_ctx *ctx, const uint32_t *cand_ids, const float *cand_scores, "
                                   "const uint16_t *cand_match, const uint64_t *cand_off, const uint32_t *q_bases, uint32_t nq, "
                                   "const sina_hip_family_rule *r, const uint32_t *self_ids, const uint64_t *self_off, uint32_t *out_rows);",
        "sina_hip_kmer_topk_family": "int sina_hip_kmer_topk_family(sina_hip_ctx *ctx, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, "
                                     "uint32_t max, const sina_hip_family_rule *r, const uint32_t *self_ids, const uint64_t *self_off, "
                                     "uint32_t *out_rows);",
        "sina_hip_family_stats": "int sina_hip_family_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *queries, "
                                 "uint64_t *candidates_listed, uint64_t *candidates_scanned, uint64_t *launches);",
    }
    stub = open(os.path.join(ROOT, "tools", "hoststub", "fake_hip.cpp")).read()
    L = capi.load()
    for sym, proto in protos.items():
        assert proto in flat, sym
        assert sym in capi.ABI_SYMBOLS and hasattr(L, sym)
        assert re.search(r"\bint %s\(" % sym, stub)
    assert ("typedef struct sina_hip_family_rule { uint32_t fs_min, fs_max, fs_req_full, fs_full_len, fs_min_len, fs_cover_gene; "
            "float fs_msc, fs_msc_max; } sina_hip_family_rule;") in flat
    assert C.sizeof(capi.FamilyRule) == 32
    for method in ("family_cascade", "kmer_topk_family", "family_row_words", "family_stats"):
        assert callable(getattr(capi.Context, method))
    # no existing struct changed
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", header) and L.sina_hip_abi_version() == 5
    # the kernel is its own unit with its own plan header, plain C++
    src = open(os.path.join(ROOT, "sina_amd", "csrc", "family.hip")).read()
    assert "family_cascade_kernel" in src and "family_meta_kernel" in src and "asm" not in src
    plan = open(os.path.join(ROOT, "sina_amd", "csrc", "family_plan.h")).read()
    assert "#include <hip" not in plan and "hip_runtime" not in plan and "kFamilyCascadeMaxK = %d" % cr.MAX_K in plan
    assert capi.FAMILY_MAX_K == cr.MAX_K


def test_host_library_takes_device_cascade():
    H = pipeline.load_host()
    H.sina_host_reset_options()
    try:
        assert H.sina_host_set_option(b"famfinder", b"device-cascade", b"1") == 0
        assert H.sina_host_set_option(b"famfinder", b"device-cascade", b"0") == 0
        assert H.sina_host_set_option(b"famfinder", b"device-cascades", b"1") != 0
        assert b"unknown option device-cascades" in H.sina_host_last_error()
    finally:
        H.sina_host_reset_options()
    assert hasattr(H, "sina_host_store_family_stats") and callable(pipeline.Store.family_stats)


@pytest.mark.parametrize("name", kc.NAMES)
def test_case_predicate(name):
    """Building a case runs its builder's assertions; its row has the bound's width and leaving early keeps it."""
    c = kc.case(name)
    row = kc.expected(name)
    assert row.dtype == np.uint32 and len(row) == cr.row_words(c.rule) and row[0] <= cr.bound(c.rule)
    assert kc.run(c, early_exit=True).kept == kc.run(c).kept
    assert bool(row[1] & cr.FLAG_EMPTY) == (len(c.ids) == 0) and not (row[1] >> 2)
    assert kc.scanned(c) <= len(c.ids)


def test_cases_cover_the_edges():
    names = set(kc.NAMES)
    assert {"len_%d" % n for n in (0, 1, 63, 64, 65, 128, 129)} <= names
    assert {"%s_at_%d" % (w, m) for w in ("min", "max") for m in (63, 64, 65)} <= names
    lens = [len(kc.case(n).ids) for n in kc.groups()[kc.case("len_0").rule]]
    assert min(lens) == 0 and max(lens) == 129                      # rows below the stride share a call with the longest
    assert kc.case("identity_limit").match is not None and kc.case("msc_max_1").match is None
    assert kc.expected("full_behind_max")[0] == cr.bound(kc.case("full_behind_max").rule)


def _random_rule(rng, sizes, scores, msc_max=2.0):
    pick = lambda a: int(a[int(rng.integers(len(a)))]) if len(a) else 0
    return cr.Rule(fs_min=int(rng.integers(0, 9)), fs_max=int(rng.integers(1, 9)), fs_req_full=int(rng.integers(0, 3)),
                   fs_full_len=pick(sizes) + int(rng.integers(0, 2)), fs_min_len=int(rng.integers(0, 2)) * pick(sizes),
                   fs_cover_gene=int(rng.integers(0, 3)), fs_msc=float(pick(scores)) + 0.5 if rng.integers(2) else 0.7, fs_msc_max=msc_max)


def _random_store(seed):
    """A small store of cut references (some without bases, some starting in column 0) and a query drawn from it."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(20, 70))
    refs = synth.make_refs(n, length=70, width=260, seed=1000 + seed, n_clades=2, clade_div=0.1, sub_lo=0.01, sub_hi=0.1)
    seqs = []
    for i in range(n):
        s = refs.seq(i)
        cut = int(rng.integers(4))
        if cut == 0:
            s = s[:0] if rng.integers(3) == 0 else s[:int(rng.integers(1, 12))]
        elif cut == 1:
            s = s[int(rng.integers(0, 30)):]
        if len(s) and rng.integers(3) == 0:
            s = s - (s[0] & np.uint32(0xFFFFFF))                    # first base in column 0
        seqs.append(np.ascontiguousarray(s, np.uint32))
    q = refs.seq(int(rng.integers(n)))
    return rng, refs.width, seqs, np.ascontiguousarray(q, np.uint32)


@pytest.mark.parametrize("block", range(8))
def test_plain_loop_equals_oracle_famfinder(oracle, block):
    """cascade_ref with its escalation loop gives the oracle's famfinder (so_famfinder) its family, ids and scores, on
    random stores and option sets -- leave-out included; the oracle takes no identity limit."""
    for seed in range(block, SEEDS, 8):
        rng, width, seqs, q = _random_store(seed)
        names = ["ref%d" % i for i in range(len(seqs))]
        cs = [oracle.Cseq.from_packed(nm, s, width) for nm, s in zip(names, seqs)]
        idx = oracle.Index(cs, k=6)
        meta = cr.meta_of(seqs)
        leave_out = bool(rng.integers(2))
        qname = names[int(rng.integers(len(names)))] if rng.integers(3) else "other"
        oq = oracle.Cseq.from_packed(qname, q, width)
        _, all_scores = idx.find(oq, len(seqs))
        rule = _random_rule(rng, meta[:, 0], all_scores)
        selfs = [names.index(qname)] if leave_out and qname in names else []
        ids, scores, rounds = cr.escalate(lambda M: idx.find(oq, M), len(seqs), rule,
                                          lambda i, s: cr.candidates(meta, i, s, None, len(q), selfs))
        want_ids, want_scores, _ = idx.famfinder(oq, oracle.ff_opts(
            fs_min=rule.fs_min, fs_max=rule.fs_max, fs_msc=rule.fs_msc, fs_msc_max=2.0, fs_leave_query_out=int(leave_out), fs_req=0,
            fs_req_full=rule.fs_req_full, fs_full_len=rule.fs_full_len, fs_req_gaps=0, fs_min_len=rule.fs_min_len,
            fs_cover_gene=rule.fs_cover_gene))
        assert ids.tolist() == want_ids.tolist() and scores.tobytes() == want_scores.tobytes(), (seed, rule, rounds)
        assert len(ids) <= cr.bound(rule)


def test_bound_and_early_exit_over_random_sets():
    """have <= K, and no candidate is kept behind the first point at which `saturated` holds: over random option sets
    and lists, identity limits and self entries included."""
    rng = np.random.default_rng(77)
    for _ in range(20 * SEEDS):
        n = int(rng.integers(0, 150))
        sizes = rng.integers(0, 6, size=n)
        cands = [(int(sizes[x]), int(rng.integers(0, 2)), 9, np.float32(rng.integers(0, 4)), np.float32(rng.integers(0, 11)) / np.float32(10),
                  bool(rng.integers(8) == 0)) for x in range(n)]
        rule = cr.Rule(fs_min=int(rng.integers(0, 9)), fs_max=int(rng.integers(0, 9)), fs_req_full=int(rng.integers(0, 3)),
                       fs_full_len=int(rng.integers(0, 6)), fs_min_len=int(rng.integers(0, 4)), fs_cover_gene=int(rng.integers(0, 3)),
                       fs_msc=float(rng.integers(0, 4)) + 0.5, fs_msc_max=float(rng.choice([0.5, 0.9, 1.0, 2.0])))
        full, early = cr.cascade(cands, rule), cr.cascade(cands, rule, early_exit=True)
        assert full.have == len(full.kept) <= cr.bound(rule)
        assert early[:6] == full[:6] and early.stop <= full.stop == n
        assert all(x < early.stop for x in full.kept)


def _leaveout_setup(oracle):
    from tests import util
    refs, dense, clade = mc.leaveout_world()
    names, seqs, kinds = mc.leaveout_queries()
    idx = oracle.Index(util.cseqs_from_refs(refs), k=10)
    meta = cr.meta_of([refs.seq(i) for i in range(refs.n)])
    return refs, dense, names, seqs, kinds, idx, meta


def test_plain_loop_on_the_leaveout_world(oracle):
    """On the leave-out world: cascade_ref equals msc_cases.leaveout_cascade under the leave-out options (identity
    limit 0.9), and the oracle's famfinder under the same options without the limit; a member's rounds are 41, 410 and
    the whole store."""
    refs, dense, names, seqs, kinds, idx, meta = _leaveout_setup(oracle)
    sizes = np.diff(refs.off)
    rule = cr.Rule(fs_min=mc.LO_FS_MIN, fs_max=mc.LO_FS_MAX, fs_req_full=1, fs_full_len=mc.LO_FULL_LEN, fs_min_len=mc.LO_MIN_LEN,
                   fs_cover_gene=0, fs_msc=mc.LO_FS_MSC, fs_msc_max=float(mc.LO_MSC_MAX))
    assert np.float32(rule.fs_msc_max) == mc.LO_MSC_MAX
    for name, q, kind in list(zip(names, seqs, kinds))[::3] + [(names[-1], seqs[-1], kinds[-1])]:
        if kind == "equal_columns":
            continue
        oq = oracle.Cseq.from_packed(name, q, refs.width)
        ident = mc.identities(dense, q)
        self_id = int(name[3:]) if name.startswith("ref") else -1
        lists = lambda M: idx.find(oq, M)
        view = lambda ids, sc: [(int(meta[i, 0]), int(meta[i, 1]), int(meta[i, 2]), s, ident[int(i)], int(i) == self_id) for i, s in zip(ids, sc)]
        ids, _, rounds = cr.escalate(lists, refs.n, rule, view)
        assert ids.tolist() == mc.leaveout_cascade(lists, sizes, ident, self_id, refs.n), name
        if kind == "member":
            assert rounds == [41, 410, refs.n] and len(ids) == mc.LO_FS_MAX
        # ... and without the limit, the oracle's own
        free = rule._replace(fs_msc_max=2.0)
        ids, scores, _ = cr.escalate(lists, refs.n, free, view)
        want_ids, want_scores, _ = idx.famfinder(oq, oracle.ff_opts(fs_leave_query_out=1, fs_min_len=mc.LO_MIN_LEN, fs_full_len=mc.LO_FULL_LEN,
                                                                    fs_req=0, fs_req_gaps=0))
        assert ids.tolist() == want_ids.tolist() and scores.tobytes() == want_scores.tobytes(), name


def test_family_plan_against_plain_arithmetic(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "family_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address", "-I" + os.path.join(ROOT, "sina_amd", "csrc"),
                    os.path.join(ROOT, "tests", "family_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "family_plan_check: ok" in run.stdout, run.stdout[-4000:]
    # ... and the Python mirrors of K and the row width, against the plan and against the library's own entry
    L = capi.load()
    for fs_min, fs_max, full, cover, nq in ((40, 40, 1, 0, 1000), (0, 0, 0, 0, 0), (10, 4, 2, 3, 5), (1024, 0, 0, 0, 1), (1021, 5, 1, 1, 7),
                                           (1024, 0, 1, 0, 1), (0, 1023, 0, 1, 1), (2 ** 32 - 1, 7, 2 ** 32 - 1, 2 ** 32 - 1, 3)):
        out = subprocess.run([exe] + [str(x) for x in (fs_min, fs_max, full, cover, nq)], stdout=subprocess.PIPE, text=True, check=True).stdout
        ok, K, words, grid = (int(x) for x in out.split())
        rule = cr.Rule(fs_min=fs_min, fs_max=fs_max, fs_req_full=full, fs_cover_gene=cover)
        assert bool(ok) == (cr.bound(rule) <= cr.MAX_K)
        crule = capi.FamilyRule(fs_min=fs_min, fs_max=fs_max, fs_req_full=full, fs_cover_gene=cover)
        w = C.c_uint32(12345)
        rc = L.sina_hip_family_row_words(C.byref(crule), C.byref(w))
        if ok:
            assert (K, words, grid) == (cr.bound(rule), cr.row_words(rule), -(-nq // 4))
            assert rc == 0 and w.value == words == crule.row_words and crule.K == K
        else:
            assert rc != 0 and w.value == 12345 and L.sina_hip_last_error_is_limit() == 1
            assert b"1024" in L.sina_hip_last_error()
