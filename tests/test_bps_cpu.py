"""CPU side of the helix base-pair score (align_bp_score_slv): the host walk (cseq_base::calcPairScore) and
pair_score_from_counts against the plain restatement of tests/bps_ref.py on every case of tests/bps_cases.py and on
seeded random sequences -- counters equal, score bits equal; the score table's worked examples; the dot-bracket
reader; the planning code of sina_amd/csrc/pair_plan.h in a stand-alone program under the address and
undefined-behaviour sanitizers; the additions to the C ABI; Log::printer with and without a helix map.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sina_amd import capi, pairs, pipeline, synth
from tests import bps_cases as bc
from tests import bps_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_host(q_ab, q_off, m, what):
    for i, s in enumerate(bc.sequences(q_ab, q_off)):
        want = br.counts(s, m)
        score, got = pipeline.host_pair_score(s, m)
        assert [int(x) for x in got] == want, (what, i, got, want)
        assert br.bits(score) == br.bits(br.score(want)), (what, i, score, br.score(want))
        again, attr = pipeline.pair_score_from_counts(want)
        assert br.bits(again) == br.bits(score) and attr == br.attr(br.score(want)), (what, i)


@pytest.mark.parametrize("name", bc.NAMES)
def test_host_walk_on_cases(name):
    q_ab, q_off, m = bc.case(name)
    _check_host(q_ab, q_off, m, name)


@pytest.mark.parametrize("symmetric", [True, False])
def test_host_walk_on_random_sequences(symmetric):
    q_ab, q_off, m = bc.random_batch(0, n=200, symmetric=symmetric)
    assert len(q_off) == 201
    _check_host(q_ab, q_off, m, "random")


def test_score_table():
    """The worked examples: width 12, columns 1..4 paired with 10..7 both ways."""
    for text, (num, ag, au, cg, gg, gu, attr) in zip(bc.TABLE_SEQS, bc.TABLE_EXPECT):
        score, counts = pipeline.host_pair_score(text, bc.TABLE_MAP)     # (the aligned string itself)
        assert tuple(int(x) for x in counts) == (num, ag, au, cg, gg, gu), text
        assert br.attr(score) == attr and pipeline.pair_score_from_counts(counts)[1] == attr, text
        assert br.counts(bc.words_of(text), bc.TABLE_MAP) == [num, ag, au, cg, gg, gu]
    assert pipeline.host_pair_score(bc.TABLE_SEQS[0], bc.TABLE_MAP)[0] == np.float32(1.25)
    assert pipeline.host_pair_score(bc.TABLE_SEQS[1], bc.TABLE_MAP)[0] == np.float32(0.875)
    assert br.bits(pipeline.host_pair_score(bc.TABLE_SEQS[2], bc.TABLE_MAP)[0]) == br.bits(np.float32(0.65))
    assert br.bits(pipeline.host_pair_score(bc.TABLE_SEQS[3], bc.TABLE_MAP)[0]) == br.bits(np.float32(0))


def test_score_arithmetic():
    """The double sum is rounded once, the division is a float32 one; num == 0 gives 0 and attribute 0."""
    rng = np.random.default_rng(5)
    for _ in range(2000):
        c = rng.integers(0, 2000, size=6)
        c[0] = max(int(c[0]), 1) if rng.random() < 0.9 else 0
        got, attr = pipeline.pair_score_from_counts(c)
        want = br.score([int(x) for x in c])
        assert br.bits(got) == br.bits(want) and attr == br.attr(want), c
    assert pipeline.pair_score_from_counts([0, 5, 5, 5, 5, 5]) == (np.float32(0), 0)


def test_pairs_from_brackets():
    m = pairs.pairs_from_brackets(".((..))")
    assert m.dtype == np.uint32 and m.tolist() == [0, 6, 5, 0, 0, 2, 1]
    # kinds nest on stacks of their own: a pseudoknot written with a second kind crosses the first
    m = pairs.pairs_from_brackets(".(<[{)>]}.")
    assert m.tolist() == [0, 5, 6, 7, 8, 1, 2, 3, 4, 0]
    m = pairs.pairs_from_brackets("-:<<_AAa>>,~x")
    assert m.tolist() == [0, 0, 9, 8, 0, 0, 0, 0, 3, 2, 0, 0, 0]
    assert pairs.pairs_from_brackets("").tolist() == [] and pairs.pairs_from_brackets("....").tolist() == [0] * 4
    for bad in (".(()", ".())", ".(]", ".>", ".{"):
        with pytest.raises(ValueError):
            pairs.pairs_from_brackets(bad)
    for bad in ("(.)", "<..>", "[]", "{}"):          # a bracket at column 0: partner 0 means unpaired
        with pytest.raises(ValueError):
            pairs.pairs_from_brackets(bad)
    # the table's map
    assert pairs.pairs_from_brackets(".((((..)))).").tolist() == bc.TABLE_MAP.tolist()


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", text)
    for sym in ("sina_hip_upload_pairs", "sina_hip_pair_counts", "sina_hip_pair_stats"):
        assert re.search(r"\bint %s\(sina_hip_ctx \*ctx" % sym, text), sym
        assert sym in capi.ABI_SYMBOLS
    assert "src/cseq.cpp:651-733" in text and "src/log.cpp:383-385" in text
    L = capi.load()
    assert L.sina_hip_abi_version() == 5
    for sym in ("sina_hip_upload_pairs", "sina_hip_pair_counts", "sina_hip_pair_stats"):
        assert hasattr(L, sym), sym


def test_pair_plan_check_program(tmp_path):
    """tests/pair_plan_check.cpp: the compaction and the launch ranges, sanitized, as its own process."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "pair_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "sina_amd", "csrc"),
                    os.path.join(ROOT, "tests", "pair_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert run.returncode == 0 and "pair_plan_check: ok" in run.stdout, run.stdout[-4000:]


def _attr_lines(text):
    return [int(v) for v in re.findall(r"^align_bp_score_slv: (-?\d+)$", text, re.M)]


def test_log_printer_without_a_map():
    """Today's output: no helix map, attribute 0 for every sequence and avg_bps 0."""
    refs = synth.make_refs(4, length=40, width=100, seed=1)
    st = pipeline.Store(":mem:bps-nomap", refs, device=0)
    try:
        H = pipeline.load_host()
        H.sina_host_reset_options()
        pipeline._set_options(H, "aligner", {"db": st.key})
        text, avg = pipeline.log_reports(bc.TABLE_SEQS)
        assert _attr_lines(text) == [0, 0, 0, 0]
        assert avg == 0.0
        H.sina_host_reset_options()                         # ... and with no store named at all
        text, avg = pipeline.log_reports(bc.TABLE_SEQS[:2])
        assert _attr_lines(text) == [0, 0] and avg == 0.0
    finally:
        st.close()


def test_log_printer_with_a_map():
    """A tray that no batch step has scored takes the host walk; the totals add the float scores as doubles, in order."""
    refs = synth.make_refs(4, length=40, width=100, seed=1)
    st = pipeline.Store(":mem:bps-map", refs, device=0)
    try:
        H = pipeline.load_host()
        H.sina_host_reset_options()
        pipeline._set_options(H, "aligner", {"db": st.key})
        st.set_pairs(bc.TABLE_MAP)
        text, avg = pipeline.log_reports(bc.TABLE_SEQS)
        assert _attr_lines(text) == [e[6] for e in bc.TABLE_EXPECT]
        total = 0.0
        for s in bc.TABLE_SEQS:
            total += float(br.score(br.counts(bc.words_of(s), bc.TABLE_MAP)))
        assert avg == total / 4
        st.set_pairs(np.zeros(12, np.uint32))               # an all-zero map removes it
        text, avg = pipeline.log_reports(bc.TABLE_SEQS)
        assert _attr_lines(text) == [0, 0, 0, 0] and avg == 0.0
        st.set_pairs(bc.TABLE_MAP)
        st.set_pairs(np.zeros(0, np.uint32))                # ... and so does an empty one
        assert _attr_lines(pipeline.log_reports(bc.TABLE_SEQS)[0]) == [0, 0, 0, 0]
    finally:
        st.close()
