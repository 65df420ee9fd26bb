"""Pins tests/walk_ref.py -- the plain walk the GPU trace-back tests compare against -- to the oracle's backtrack(), and
asserts that every directed input of tests/walk_cases.py still reaches the edge it was built for.  No GPU: a case that
silently stops reaching its edge fails here, on any machine."""
import os

import numpy as np
import pytest

from tests import util, walk_cases as wc, walk_ref


def _pin(case, ref):
    """walk_ref.walk + the container steps == oracle.backtrack: packed bases, head, tail, score bits, fix-up log."""
    for i, r in enumerate(ref):
        wk, orc, tag = r["walk"], r["orc"], (case.name, i)
        packed, log = util.finish_alignment(r["oracle_masks"], wk, wk["cols"], case.width,
                                            lowercase_unaligned=(case.opts["lowercase"] == 2), want_packed=True)
        assert packed is not None and (packed == orc["packed"]).all(), tag
        assert (wk["cutoff_head"], wk["cutoff_tail"]) == (orc["head"], orc["tail"]), tag
        assert util.f32_bits(np.float32(wk["raw"]) / np.float32(wk["sum_weight"])) == util.f32_bits(orc["score"]), tag
        assert orc["log"].startswith(log) and orc["log"][len(log):].startswith("scoring: "), tag
        assert "aligned-bases=%d," % wk["aligned_bases"] in orc["log"], tag
        # the masks in append order are what the walk's columns belong to
        m = walk_ref.out_masks(r["oracle_masks"], wk, case.opts["overhang"], case.opts["lowercase"] == 2)
        assert len(m) == wk["n_out"] == len(wk["cols"]), tag
        f = r["facts"]
        if f["fits"] and not f["beyond"]:   # (a run that does not fit makes its neighbours move: they count too)
            assert (f["nast_total"], f["nast_longest"], f["nast_last_run"]) == wc.nast_numbers(orc["log"]), tag
            # ... and the finished sequence is the append rule's columns, mirrored, with every run right-aligned
            # in its gap
            colm = f["colm"].copy()
            for i0, n in f["runs"]:
                nxt = case.width - 1 - int(colm[i0 - 1]) if i0 > 0 else case.width
                colm[i0:i0 + n] = case.width - nxt + np.arange(n)
            assert ((orc["packed"] & 0xFFFFFF) == (case.width - 1 - colm)[::-1]).all(), tag
        else:
            assert "shifting bases to fit" in orc["log"] or f["beyond"], tag
        assert r["must"] == (wk["n_out"] <= 4096 and f["fits"] and not f["beyond"])


@pytest.mark.parametrize("name", ["matrix"] + sorted(wc.DIRECTED))
def test_plain_walk_equals_oracle_backtrack(oracle, name):
    """All three overhang modes, all three lowercase modes, shift and forbid, the simple, weighted and profile schemes
    (matrix), and the inputs of every directed GPU test."""
    for case, ref in wc.group(name):
        _pin(case, ref)


def _stats(name, pick=None):
    return [(c, r, r["walk"]["stats"]) for c, ref in wc.group(name) if pick is None or pick(c) for r in ref]


def test_insertion_scan_leaves_the_window():
    for case, ref in wc.group("insertion_scan"):
        long_runs = [r for r in ref if r["walk"]["stats"]["longest_ins_run"] >= 65]
        assert long_runs, case.name
        assert all(not r["must"] and not r["facts"]["fits"] for r in long_runs), case.name
        assert case.opts["insertion"] == 0     # (type-code cells: the start of the insertion is found by scanning)


def test_insertion_run_reaches_column_0():
    """Reached by the type-code cells' case (observed: queries 0 and 2 of `ins-col0`).  Under --insertion=forbid the
    same inputs take other paths; the 32-bit cells store value_sidx, so nothing scans there anyway."""
    hits = [s["ins_reaches_col0"] for c, r, s in _stats("insertion_col0", lambda c: c.opts["insertion"] == 0)]
    assert sum(hits) >= 1


def test_row_jump_beyond_the_window():
    for case, ref in wc.group("row_jump"):
        st = [r["walk"]["stats"] for r in ref]
        assert max(s["max_row_jump"] for s in st) >= 65, case.name
        assert any(s["max_row_jump"] >= 65 and s["far_deletions"] >= 1 for s in st), case.name
    assert {c.opts["insertion"] for c, _ in wc.group("row_jump")} == {0, 1}


def test_predecessor_ordinals_outside_the_cached_four():
    for ins in (0, 1):
        st = [s for c, r, s in _stats("many_predecessors", lambda c: c.opts["insertion"] == ins)]
        assert any(s["ord_ge4"] >= 10 and s["max_npred"] >= 9 for s in st)
    assert {len(c.fams[0]) for c, _ in wc.group("many_predecessors")} == {40, 128}


def test_load_alignment_end_columns():
    for ins in (0, 1):
        ragged = [c for c, _ in wc.group("load_alignment") if c.name == "load-align-ragged-ins%d" % ins]
        assert len(ragged) == 1 and tuple(len(m) for m in ragged[0].qmasks) == wc.ALIGN_LENGTHS
        alone = [(c, ref) for c, ref in wc.group("load_alignment") if c.opts["insertion"] == ins and len(ref) == 1]
        assert tuple(len(c.qmasks[0]) for c, _ in alone) == wc.ALIGN_LENGTHS
        ends = [ref[0]["walk"]["end_s"] for _, ref in alone]
        assert {e % 8 for e in ends} == set(range(8)) and {e % 4 for e in ends} == set(range(4))
        assert any(ref[0]["walk"]["cutoff_tail"] > 0 for _, ref in alone)
        assert min(wc.ALIGN_LENGTHS) < 32
        # alone or in the ragged launch, a query is the same query
        rr = [ref for c, ref in wc.group("load_alignment") if c is ragged[0]][0]
        assert [r["walk"]["end_s"] for r in rr] == ends


def test_overhang_clamps():
    by_name = {c.name: (c, ref) for c, ref in wc.group("overhang_clamps")}
    case, ref = by_name["overhang-clamps-attach"]
    tail_clamped = head_clamped = reaches_edge = False
    for r in ref:
        wk = r["walk"]
        cols, t, h = wk["cols"], wk["cutoff_tail"], wk["cutoff_head"]
        # more overhanging bases than columns left: the first tail entries sit on column 0, the last head entries on
        # width - 1, several each
        tail_clamped |= t >= 2 and (cols[:2] == 0).all()
        head_clamped |= h >= 2 and (cols[-2:] == case.width - 1).all()
        reaches_edge |= h == 0 and cols.max() == case.width - 1 and r["must"]
    assert tail_clamped and head_clamped and reaches_edge
    assert {c.opts["overhang"] for c, _ in wc.group("overhang_clamps")} == {0, 1, 2}
    for r in by_name["overhang-clamps-remove"][1]:
        assert r["walk"]["n_out"] == r["walk"]["aligned_bases"] <= len(r["oracle_masks"])


def test_assembly_capacity():
    (case, ref), = wc.group("capacity")
    assert case.opts["overhang"] == 0
    assert [r["walk"]["n_out"] for r in ref][:3] == [4095, 4096, 4097]
    assert [r["must"] for r in ref] == [True, True, False, True, True]
    assert ref[2]["facts"]["fits"] and not ref[2]["facts"]["beyond"]   # (only its length keeps it from the device)


def test_grid_tail_sizes():
    assert [len(ref) for _, ref in wc.group("grid_tail")] == [65, 130]


def test_ends_and_starts_inside_the_dag():
    st = [s for c, r, s in _stats("partial")]
    for key in ("end_last_col_nonsink", "end_inner_sink", "stop_col0", "stop_source_inner"):
        assert any(s[key] for s in st), key


def test_fuzz_generator_reaches_both_outcomes():
    """Conditions on the generator over the default 12 seeds.  Observed: 64 queries, must_assemble true for 51 and false
    for 13; 9 launches with 16-bit cells, 3 with 32-bit ones; seeds 3, 7 and 11 profile batches.  The walk of every
    query is pinned to the oracle on the way."""
    n = n_must = 0
    formats = set()
    for seed in range(12):
        case = wc.fuzz_case(seed)
        ref = wc.reference(case)
        _pin(case, ref)
        assert 3 <= len(ref) <= 8
        n += len(ref)
        n_must += sum(r["must"] for r in ref)
        formats.add(case.opts["insertion"] == 1)
        assert bool(case.opts["fs_no_graph"]) == (seed % 4 == 3)
    assert 4 * n_must >= n and n - n_must >= 3
    assert formats == {False, True}
