"""CPU side of the in-place helix base-pair count (tests/test_gpu_bps_inplace.py runs it): the three added entries
through every layer that names them, the structs and the ABI version left as they were, and the conditions on the GPU
test's inputs -- checked here with the oracle, so that the GPU test cannot pass on inputs that show nothing."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from sina_amd import capi, pipeline, synth
from tests import bps_ref as br, test_gpu_bps_inplace as gi, util, walk_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sina_hip_align_count_pairs", "sina_hip_staged_pair_counts", "sina_hip_pair_inplace_stats")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", text)
    assert re.search(r"\bint sina_hip_align_count_pairs\(sina_hip_ctx \*ctx, int on\);", text)
    assert re.search(r"\bconst uint32_t \*sina_hip_staged_pair_counts\(sina_hip_ctx \*ctx\);", text)
    assert re.search(r"\bint sina_hip_pair_inplace_stats\(sina_hip_ctx \*ctx, double \*kernel_ms, uint64_t \*sequences, "
                     r"uint64_t \*launches\);", text)
    L = capi.load()
    assert L.sina_hip_abi_version() == 5
    for sym in NEW:
        assert sym in capi.ABI_SYMBOLS and hasattr(L, sym), sym
    assert L.sina_hip_align_count_pairs.argtypes == [C.c_void_p, C.c_int]
    assert L.sina_hip_staged_pair_counts.argtypes == [C.c_void_p]
    assert L.sina_hip_staged_pair_counts.restype == C.POINTER(C.c_uint32)
    assert len(L.sina_hip_pair_inplace_stats.argtypes) == 4
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "sina_amd", "libsina_hip.so")],
                        stdout=subprocess.PIPE, text=True, check=True).stdout
    for sym in NEW:
        assert re.search(r" T %s$" % sym, nm, re.M), sym


def test_structs_are_what_they_were():
    """No struct of the header changes: the sizes of the parent commit, as literals, and the typedefs' closing lines."""
    assert C.sizeof(capi.AlignOut) == 52 and capi.ALIGN_OUT_DTYPE.itemsize == 52
    assert C.sizeof(capi.AlignParams) == 48
    text = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    assert text.count("} sina_hip_align_out;") == 1 and text.count("} sina_hip_align_params;") == 1
    # ... and of the header itself, by the compiler
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc:
        prog = ('#include "sina_hip.h"\n_Static_assert(sizeof(sina_hip_align_out) == 52, "align_out");\n'
                '_Static_assert(sizeof(sina_hip_align_params) == 48, "align_params");\n'
                '_Static_assert(SINA_HIP_ABI_VERSION == 5, "abi");\n')
        run = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-x", "c", "-"], input=prog,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert run.returncode == 0, run.stdout


def test_stub_and_documents_name_the_entries():
    stub = open(os.path.join(ROOT, "tools", "hoststub", "fake_hip.cpp")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in NEW:
        assert re.search(r"\b%s\(sina_hip_ctx \*" % sym, stub), sym
        assert sym in doc, sym
    assert "device-bps" in doc and "dp_range_q" in open(os.path.join(ROOT, "sina_amd", "csrc", "common.h")).read()


def test_wrappers_and_option():
    for name in ("count_pairs", "staged_pair_counts", "pair_inplace_stats"):
        assert callable(getattr(capi.Context, name)), name
    assert callable(pipeline.Store.pair_inplace_stats)
    H = pipeline.load_host()
    assert hasattr(H, "sina_host_store_pair_inplace_stats")
    H.sina_host_reset_options()
    try:
        assert H.sina_host_set_option(b"aligner", b"device-bps", b"1") == 0
        assert H.sina_host_set_option(b"aligner", b"device-bps", b"0") == 0
        assert H.sina_host_set_option(b"aligner", b"device-bpz", b"1") != 0
    finally:
        H.sina_host_reset_options()


def test_null_context_is_refused_by_name():
    L = capi.load()
    assert L.sina_hip_align_count_pairs(None, 1) != 0
    assert b"align_count_pairs" in L.sina_hip_last_error()
    assert not L.sina_hip_staged_pair_counts(None)
    assert b"staged_pair_counts" in L.sina_hip_last_error()
    ms, a, b = C.c_double(), C.c_uint64(), C.c_uint64()
    assert L.sina_hip_pair_inplace_stats(None, C.byref(ms), C.byref(a), C.byref(b)) != 0
    assert b"pair_inplace_stats" in L.sina_hip_last_error()


def test_helix_map_generator():
    for n in gi.ENTRY_COUNTS + (2, 3):
        m = gi.helix_map(3000, n, seed=n, occupied=np.arange(100, 400))
        idx = np.flatnonzero(m)
        assert len(idx) == n and m[0] == 0 and idx.min() >= 1 and int(m.max()) < 3000
        assert (m[idx] != idx).all()
        # nested: of two entries that open (partner to the right), the later one closes first
        opens = [(int(i), int(m[i])) for i in idx if m[i] > i]
        for (i0, p0), (i1, p1) in zip(opens, opens[1:]):
            assert i0 < i1 < p1 < p0
    assert (gi.helix_map(3000, 64, 5) == gi.helix_map(3000, 64, 5)).all()
    assert (gi.helix_map(3000, 64, 5) != gi.helix_map(3000, 64, 6)).any()


@pytest.mark.parametrize("group", gi.GROUPS)
def test_inputs_are_worth_running(oracle, group):
    """What pair_count_assembled_kernel relies on, and what makes its test say something: every query the device must
    assemble has strictly ascending columns (the kernel has no check of its own); under the test's maps the expected
    counters are not trivial -- over the group's (query, map) combinations at least half have num > 0, and every map
    size has one at least."""
    n_must = n_rest = combos = nontrivial = 0                     # (the groups together: the next test)
    by_size = {n: 0 for n in gi.ENTRY_COUNTS}
    for case, ref, per in gi.expected(group):
        for q, r in enumerate(ref):
            if not r["must"]:
                n_rest += 1
                assert all((rows[q] == 0).all() for _, rows in per.values())
                continue
            n_must += 1
            cols = (np.asarray(r["orc"]["packed"], np.uint32) & 0xFFFFFF).astype(np.int64)
            assert len(cols) >= 1 and (np.diff(cols) > 0).all() and cols[-1] < case.width, (case.name, q)
            for n, (m, rows) in per.items():
                combos += 1
                nontrivial += rows[q][0] > 0
                by_size[n] += rows[q][0] > 0
                assert rows[q][0] <= n and rows[q][1:].sum() <= rows[q][0]
    print(group, "must", n_must, "rest", n_rest, "nontrivial", nontrivial, "of", combos, by_size)
    assert 2 * nontrivial >= combos, (group, nontrivial, combos)
    assert n_must == 0 or all(v >= 1 for v in by_size.values()), (group, by_size)  # (insertion_scan: nothing is assembled)


def test_groups_hold_assembled_and_unassembled_queries(oracle):
    must = [r["must"] for g in gi.GROUPS for _, ref in wc.group(g) for r in ref]
    assert sum(1 for x in must if x) >= 20 and sum(1 for x in must if not x) >= 3
    # the lowercase modes matter: a lower-case base weighs nothing, and the matrix has finished sequences with some
    lower = sum(int(((np.asarray(r["orc"]["packed"], np.uint32) >> 28) & 1).sum())
                for _, ref in wc.group("matrix") for r in ref if r["must"])
    assert lower > 0


def test_stage_world_assembles_most_queries(oracle):
    """The world of the stages test: at least half of its queries are assembled on the device (in-place trays >= half of
    the DP's there) -- the aligner's families from the oracle's famfinder, must_assemble from the plain walk."""
    refs, mask, off, helix = gi.stage_world()
    cs = util.cseqs_from_refs(refs)
    idx = po.Index(cs, k=10)
    fams, qms = [], []
    for q in range(len(off) - 1):
        m = mask[int(off[q]):int(off[q + 1])]
        cq = po.Cseq.from_packed("q%d" % q, np.arange(len(m), dtype=np.uint32) | ((m & 0x0f).astype(np.uint32) << 24), len(m))
        ids, _, _ = idx.famfinder(cq, po.ff_opts(fs_min_len=100, fs_full_len=250))
        if len(ids):
            fams.append([cs[i] for i in ids])
            qms.append(m)
    assert len(fams) >= 60
    ref = wc.reference(wc.Case("stage-world", refs.width, fams, qms))
    n_must = sum(1 for r in ref if r["must"])
    nonzero = sum(1 for r in ref if r["must"] and br.counts(r["orc"]["packed"], helix)[0] > 0)
    print("stage world: %d of %d queries assembled on the device, %d with num > 0" % (n_must, len(ref), nonzero))
    assert 4 * n_must >= 3 * len(ref) and 2 * nonzero >= len(ref)
