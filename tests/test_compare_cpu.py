"""Pins tests/compare_ref.py -- the plain lock-step walk the GPU comparison tests compare against -- to the oracle's
traverse() and, where the sequences fit its string interface, to the host stage's cseq_comparator::counts, on every named
case of tests/compare_cases.py (whose builders assert the edge each case exists for) and on every fuzz seed, under
three IUPAC rules x two filter settings.  No GPU."""
import os

import pytest

from oracle import pyoracle as po
from sina_amd import pipeline, synth
from tests import compare_cases as cc, compare_ref

HOST_MAX_WIDTH = 8224     # (a gapped string per sequence: the wide cases are left to the oracle)


def _pin(width, refs, qs, cand, exp):
    rc = [po.Cseq.from_packed("r%d" % i, r, width) for i, r in enumerate(refs)]
    qc = [po.Cseq.from_packed("q%d" % i, q, width) for i, q in enumerate(qs)]
    n_pairs = sum(len(ids) for ids in cand)
    on_host = width <= HOST_MAX_WIDTH and n_pairs <= 1000 and \
        all(((cc.masks(s) & 15) != 0).all() for s in list(refs) + list(qs))
    if on_host:
        rs = [synth.aligned_string(r, width) for r in refs]
        qstr = [synth.aligned_string(q, width) for q in qs]
    for (rule, flc), rows in exp.items():
        assert rows.shape == (n_pairs, 6)
        at = 0
        seen = {}
        for qi, ids in enumerate(cand):
            for rid in ids:
                rid = int(rid)
                want = tuple(int(x) for x in rows[at])
                at += 1
                if (qi, rid) in seen:       # (an id listed twice is one comparison)
                    assert seen[qi, rid] == want
                    continue
                seen[qi, rid] = want
                assert po.compare_counts(qc[qi], rc[rid], compare_ref.RULES[rule], flc) == want, (rule, flc, qi, rid)
                if on_host:
                    _, got = pipeline.host_compare(qstr[qi], rs[rid], rule, 0, 4, flc)
                    assert got == want, ("host", rule, flc, qi, rid)
    return on_host


@pytest.mark.parametrize("name", cc.NAMES)
def test_plain_walk_equals_oracle_traverse(oracle, name):
    width, refs, qs, cand = cc.case(name)
    on_host = _pin(width, refs, qs, cand, cc.expected(name))
    assert on_host or width > HOST_MAX_WIDTH or name in ("mask_table", "mask_table_lc")


def test_every_gap_has_its_case():
    """The widths, word counts and sizes the matrix is meant to hold are there (each builder asserts its own edge)."""
    assert {"width_%d" % w for w in (1, 31, 32, 33, 64, 65, 2500)} <= set(cc.NAMES)
    assert {"nwords_%d" % n for n in (255, 256, 257, 511, 512, 513, 1563)} <= set(cc.NAMES)
    assert cc.case("rank_top")[0] >= 65535 and max(len(q) for q in cc.case("rank_top")[2]) == 65535
    assert cc.case("lds_wide")[0] == 524288 and cc.case("nq_1")[2].__len__() == 1 and len(cc.case("nq_600")[2]) == 600
    assert cc.LIMIT_LA == 55261 and len(cc.case("lds_limit")[2][0]) == cc.LIMIT_LA
    # the walk tells the three rules apart on the mask table, and the filter changes every case it is meant to change
    e = cc.expected("mask_table")
    assert len({tuple(e[r, False][0]) for r in (0, 1, 2)}) == 3
    for name in ("filter", "mask_table_lc"):
        e = cc.expected(name)
        assert (e[0, False] != e[0, True]).any()
    e = cc.expected("filter")
    assert (e[0, True] == 0).all(axis=1).any() and not (e[0, False] == 0).all(axis=1).any()


def test_mask_table_by_hand():
    """The 16 x 16 table's counts follow from the three rules' definitions, counted here without any walk."""
    pairs = [(a, b) for a in range(16) for b in range(16)]
    opt = sum(1 for a, b in pairs if a & b)
    pes = sum(1 for a, b in pairs if a == b and bin(a).count("1") <= 1)
    exa = sum(1 for a, b in pairs if a == b)
    assert (opt, pes, exa) == (175, 5, 16)
    e = cc.expected("mask_table")
    for rule, n in ((0, opt), (1, pes), (2, exa)):
        assert tuple(e[rule, False][0]) == (0, 0, 0, 0, n, 256 - n)


@pytest.mark.parametrize("seed", range(int(os.environ.get("SINA_FUZZ_SEEDS", "12"))))
def test_fuzz_generator_reaches_every_counter(oracle, seed):
    """The coverage condition of test_compare_fuzz holds on the plain walk alone: per setting every counter is nonzero
    for some pair and some pair has a side without a remaining base; the walk of every pair is pinned on the way."""
    width, refs, qs, cand = cc.fuzz_case(seed)
    assert width in cc.FUZZ_WIDTHS and all(len(ids) <= 40 for ids in cand)
    cc.fuzz_coverage(seed)
    _pin(width, refs, qs, cand, cc.expected("fuzz", seed))


def test_fuzz_generator_spreads_over_its_ranges():
    widths = {cc.fuzz_case(s)[0] for s in range(12)}
    assert len(widths) >= 4
    sizes = [len(ids) for s in range(12) for ids in cc.fuzz_case(s)[3]]
    assert min(sizes) == 0 and max(sizes) >= 35
