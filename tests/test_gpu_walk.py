"""The trace-back stage against a plain walk: the four device walks (one wave / one lane per query x 16-bit / 32-bit
cells) and assemble_kernel, through sina_hip_align_graphs, compared field for field and column for column with
tests/walk_ref.py on the oracle's planes (tests/test_walk_cpu.py pins that walk to the oracle's backtrack() and asserts
that the directed inputs below reach their edges).

The matrix: every launch runs four ways -- bt_lanes 0 / 1 x assemble 0 / 1 -- and
  1. assemble = 0: every field of sina_hip_align_out equals the plain walk (raw and sum_weight by their bits), and
     out_pos holds the plain walk's appended columns, entry for entry;
  2. assemble = 1: `assembled` equals walk_ref.must_assemble() exactly (include/sina_hip.h: at most 4096 bases, no column
     beyond the alignment, every insertion fits its gap).  An assembled query's out_pos is the oracle's finished
     sequence word for word, case bit included, its nast_* the container's facts; a query left alone is byte for byte
     what the launch without the switch gave;
  3. the two walks give the same bytes.
"""
import os

import numpy as np
import pytest

from sina_amd import capi
from tests import util, walk_cases as wc

pytestmark = pytest.mark.gpu

_WALK_FIELDS = ("end_m", "end_s", "cutoff_head", "cutoff_tail", "aligned_bases", "n_out")
_ASM_FIELDS = ("assembled", "nast_total", "nast_longest", "nast_last_run")


def _launches(ctx, monkeypatch, case, ref):
    """{(bt_lanes, assemble): (out, per-query out_pos[:n_out])} of one launch run four ways."""
    graphs = [r["graph"] for r in ref]
    tabs = dict(node_score16=np.concatenate([r["score16"] for r in ref]), self_score16=ref[0]["self16"]) \
        if case.opts["fs_no_graph"] else {}
    gb = ctx.graph_batch(graphs, case.width, **tabs)
    qoff = np.zeros(len(ref) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(m) for m in case.qmasks])
    qmask = np.concatenate(case.qmasks)
    popts = {k: v for k, v in case.opts.items() if k not in ("fs_no_graph", "weights")}
    got = {}
    for lanes in (0, 1):
        util.set_knobs(monkeypatch, bt_lanes=lanes)
        for asm in (0, 1):
            out, pos = ctx.align_graphs(gb, qmask, qoff, ctx.params(weights=case.opts["weights"], assemble=asm, **popts))
            got[lanes, asm] = (out.copy(), [pos[int(qoff[q]):int(qoff[q]) + int(out[q]["n_out"])].copy()
                                            for q in range(len(ref))])
    return got


def _check(case, ref, got):
    for lanes in (0, 1):
        plain, plain_pos = got[lanes, 0]
        asm, asm_pos = got[lanes, 1]
        for q, r in enumerate(ref):
            wk, tag = r["walk"], (case.name, "bt_lanes=%d" % lanes, "query %d" % q)
            o = plain[q]
            # 1. the walk alone
            assert o["status"] == 0, tag
            for f in _WALK_FIELDS:
                assert int(o[f]) == int(wk[f]), tag + (f, int(o[f]), int(wk[f]))
            assert util.f32_bits(o["raw"]) == util.f32_bits(wk["raw"]), tag + ("raw", o["raw"], wk["raw"])
            assert util.f32_bits(o["sum_weight"]) == util.f32_bits(wk["sum_weight"]), \
                tag + ("sum_weight", o["sum_weight"], wk["sum_weight"])
            assert all(int(o[f]) == 0 for f in _ASM_FIELDS), tag
            bad = np.flatnonzero(plain_pos[q].astype(np.int64) != wk["cols"])
            assert len(bad) == 0, tag + ("out_pos differs first at append %d of %d" % (bad[0], wk["n_out"]),)
            # 2. the assembly
            a = asm[q]
            assert int(a["assembled"]) == int(r["must"]), \
                tag + ("assembled", int(a["assembled"]), "must", r["must"], "fits", r["facts"]["fits"])
            if a["assembled"]:
                f = r["facts"]
                assert (int(a["nast_total"]), int(a["nast_longest"]), int(a["nast_last_run"])) == \
                    (f["nast_total"], f["nast_longest"], f["nast_last_run"]), tag
                assert (f["nast_total"], f["nast_longest"], f["nast_last_run"]) == wc.nast_numbers(r["orc"]["log"]), tag
                bad = np.flatnonzero(asm_pos[q] != r["orc"]["packed"])
                assert len(bad) == 0, tag + ("assembled sequence differs first at base %d" % bad[0],)
                assert all(a[n].tobytes() == o[n].tobytes() for n in a.dtype.names if n not in _ASM_FIELDS), tag
            else:
                assert a.tobytes() == o.tobytes() and (asm_pos[q] == plain_pos[q]).all(), tag
    # 3. one wave per query == one lane per query
    for asm in (0, 1):
        assert got[0, asm][0].tobytes() == got[1, asm][0].tobytes(), (case.name, "assemble=%d" % asm)
        for q in range(len(ref)):
            assert (got[0, asm][1][q] == got[1, asm][1][q]).all(), (case.name, "assemble=%d" % asm, q)


def _matrix(monkeypatch, case, ref, after_launch=None):
    for knobs in case.variants:
        util.set_knobs(monkeypatch, geom=None, rho=None, lds_kb=None)
        util.set_knobs(monkeypatch, **knobs)
        ctx = capi.Context(0)   # (a context of its own: the LDS budget is read when it is created)
        try:
            got = _launches(ctx, monkeypatch, case, ref)
            if after_launch:
                after_launch(ctx, case, ref, knobs)
        finally:
            ctx.close()
        _check(case, ref, got)


@pytest.mark.parametrize("which", range(len(wc.MATRIX_NAMES)), ids=wc.MATRIX_NAMES)
def test_walk_matrix(oracle, monkeypatch, which):
    """`small` under every overhang and lowercase mode, shift and forbid, simple, weighted and profile scheme."""
    case, ref = wc.group("matrix")[which]
    _matrix(monkeypatch, case, ref)


def _directed(monkeypatch, name):
    for case, ref in wc.group(name):
        _matrix(monkeypatch, case, ref)


def test_insertion_scan_leaves_the_window(oracle, monkeypatch):
    """Insertions of 68 to 129 bases: the type-code cells' leftward scan for the insertion's start crosses window
    refills, and the insertion does not fit its gap (assembled == 0)."""
    _directed(monkeypatch, "insertion_scan")


def test_insertion_run_reaches_column_0(oracle, monkeypatch):
    _directed(monkeypatch, "insertion_col0")


def test_row_jump_beyond_the_window(oracle, monkeypatch):
    """Deletions of 60 to 150 bases: consecutive path cells up to 365 rows apart, through gap-extending cells."""
    _directed(monkeypatch, "row_jump")


def test_predecessor_ordinals_outside_the_cached_four(oracle, monkeypatch):
    """Nodes with up to 15 predecessors, 60 path steps per query to the fifth and later: both cell formats."""
    _directed(monkeypatch, "many_predecessors")


def test_load_alignment_of_the_window(oracle, monkeypatch):
    """Query lengths 1 .. 257 in one ragged launch and each alone; end columns of every residue modulo 8."""
    _directed(monkeypatch, "load_alignment")


def test_overhang_clamps(oracle, monkeypatch):
    _directed(monkeypatch, "overhang_clamps")


def test_assembly_capacity(oracle, monkeypatch):
    """4095 and 4096 bases are assembled on the device, 4097 are not."""
    _directed(monkeypatch, "capacity")


def test_lane_grid_tail(oracle, monkeypatch):
    _directed(monkeypatch, "grid_tail")


def test_walk_over_a_pruned_plane(oracle, monkeypatch):
    """Two-strip and three-strip geometries with the row skip on: the walk runs beside rows nobody swept."""
    for case, ref in wc.group("pruned_plane"):
        skipping = []

        def look(ctx, case, ref, knobs):
            b = int(knobs["geom"].split(",")[1])
            for q, r in enumerate(ref):
                info = ctx.dp_info(q)
                assert info["attempts"] >= 1, (case.name, knobs, q)
                strips = (len(case.qmasks[q]) - 1) // (64 * b) + 1
                skipping.append(info["rows_swept"] < strips * r["graph"]["n"] * info["attempts"])
        _matrix(monkeypatch, case, ref, after_launch=look)
        assert any(skipping), case.name


def test_ends_and_starts_inside_the_dag(oracle, monkeypatch):
    _directed(monkeypatch, "partial")


@pytest.mark.parametrize("seed", range(int(os.environ.get("SINA_FUZZ_SEEDS", "12"))))
def test_walk_fuzz(oracle, monkeypatch, seed):
    """The plane fuzz's worlds, families, scoring and geometry draws with 3 to 8 queries per launch (pieces of members,
    mutated, runs spliced in and cut out, some lower case), random overhang and lowercase modes, every fourth seed a
    profile batch: the matrix above."""
    case = wc.fuzz_case(seed)
    _matrix(monkeypatch, case, wc.reference(case))
