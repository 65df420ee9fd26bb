"""The trace-back walk that fetches a row's cell, record and first four predecessor ids (pred4, sina_amd/csrc/common.h)
together, against the plain walk (tests/walk_ref.py on the oracle's planes):

  1. the lane walk forced (bt_lanes=1) over the directed inputs of tests/walk_cases.py that reach what the combined
     fetch changed: predecessor ordinals 0-3 and >= 4, Ext chains and long deletions, the one-step deletion skip at a
     row whose record differs from the skipped row's, insertion scans to column 0, a plane with unswept rows;
  2. every producer of the table -- the device DAG build, the host-built DAG, a caller-supplied DAG, the device and the
     host profile build -- once with the wave walk and once with the lane walk: a producer that leaves the table out
     fails here.

The conditions "the input reaches its edge" are asserted on the CPU (the first two tests; tests/test_walk_cpu.py holds
the others of walk_cases.py)."""
import numpy as np
import pytest

from oracle import pyoracle as po
from sina_amd import capi, pipeline
from tests import util, walk_cases as wc, walk_ref

gpu = pytest.mark.gpu

_WALK_FIELDS = ("end_m", "end_s", "cutoff_head", "cutoff_tail", "aligned_bases", "n_out")


# ---------------------------------------------------------------- the edges, on the CPU

def skip_steps(g, cells):
    """[(skipped row, row taken instead)] of the one-step deletion skips (mesh.h:653-655) on the path of one query."""
    vmid, vsid = cells["value_midx"], cells["value_sidx"]
    srcs = set(int(x) for x in g["src"])
    m, s = walk_ref.end_cell(g, cells["value"])
    out = []
    while s != 0 and m not in srcs:
        snew, m = int(vsid[m, s]), int(vmid[m, s])
        if snew != 0 and int(vsid[m, snew]) == snew:
            m2 = int(vmid[m, snew])
            out.append((m, m2))
            m = m2
        s = snew
    return out


def test_deletion_skip_lands_on_a_row_with_another_record(oracle):
    """row-jump-small: the walk issues the record of the row it reaches first and takes the skip afterwards; the row it
    ends on has another column and another weight, so the skipped row's record in its place would show in out_pos
    and in sum_weight."""
    case = next(c for c, _ in wc.group("row_jump") if c.name == "row-jump-small")
    hits = 0
    for i, (fam, qm) in enumerate(zip(case.fams, case.qmasks)):
        g = util.graph_dict(fam, case.opts["fs_weight"])
        cells = po.backtrack(fam, wc._cseq("q%d" % i, case.oracle_masks(i)), case.oracle_opts())["cells"]
        for m, m2 in skip_steps(g, cells):
            hits += int(g["pos"][m] != g["pos"][m2] and util.f32_bits(g["weight"][m]) != util.f32_bits(g["weight"][m2]))
    assert hits >= 1


def test_directed_inputs_reach_the_near_and_the_far_ordinals():
    """many_predecessors: path steps to predecessors 0-3 (the table) AND to the fifth and later (the list)."""
    for case, ref in wc.group("many_predecessors"):
        st = [r["walk"]["stats"] for r in ref]
        steps = sum(len(r["walk"]["rows"]) - 1 for r in ref)
        assert sum(s["ord_ge4"] for s in st) >= 10 and steps - sum(s["ord_ge4"] for s in st) >= 10, case.name
    assert any(s["far_deletions"] >= 1 for _, ref in wc.group("row_jump") for s in [r["walk"]["stats"] for r in ref])
    assert any(r["walk"]["stats"]["ins_reaches_col0"] for _, ref in wc.group("insertion_col0") for r in ref)


# ---------------------------------------------------------------- 1. the lane walk over the directed inputs

def _same_walk(out, pos, qoff, ref, tag):
    for q, r in enumerate(ref):
        wk, o, t = r["walk"], out[q], tag + ("query %d" % q,)
        assert o["status"] == 0, t
        for f in _WALK_FIELDS:
            assert int(o[f]) == int(wk[f]), t + (f, int(o[f]), int(wk[f]))
        assert util.f32_bits(o["raw"]) == util.f32_bits(wk["raw"]), t + ("raw",)
        assert util.f32_bits(o["sum_weight"]) == util.f32_bits(wk["sum_weight"]), t + ("sum_weight", o["sum_weight"], wk["sum_weight"])
        got = pos[int(qoff[q]):int(qoff[q]) + int(o["n_out"])].astype(np.int64)
        bad = np.flatnonzero(got != wk["cols"])
        assert len(bad) == 0, t + ("out_pos differs first at append %d of %d" % (bad[0], wk["n_out"]),)


def _qarrays(case):
    qoff = np.zeros(len(case.qmasks) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(m) for m in case.qmasks])
    return np.concatenate(case.qmasks), qoff


def _params(ctx, case, **kw):
    popts = {k: v for k, v in case.opts.items() if k not in ("fs_no_graph", "weights")}
    popts.update(kw)
    return ctx.params(weights=case.opts["weights"], assemble=0, **popts)


def _lanes_over(monkeypatch, name):
    for case, ref in wc.group(name):
        qmask, qoff = _qarrays(case)
        for knobs in case.variants:
            util.set_knobs(monkeypatch, geom=None, rho=None, lds_kb=None)
            util.set_knobs(monkeypatch, bt_lanes=1, **knobs)
            ctx = capi.Context(0)   # (a context of its own: the LDS budget is read when it is created)
            try:
                gb = ctx.graph_batch([r["graph"] for r in ref], case.width)
                out, pos = ctx.align_graphs(gb, qmask, qoff, _params(ctx, case))
            finally:
                ctx.close()
            _same_walk(out, pos, qoff, ref, (case.name, str(knobs)))


@gpu
def test_lanes_predecessor_ordinals_in_and_outside_the_table(oracle, monkeypatch):
    _lanes_over(monkeypatch, "many_predecessors")


@gpu
def test_lanes_ext_chains_and_long_deletions(oracle, monkeypatch):
    """Deletions of 60 to 150 rows through gap-extending cells (several gapm_idx hops each), and the deletion skip of
    test_deletion_skip_lands_on_a_row_with_another_record."""
    _lanes_over(monkeypatch, "row_jump")


@gpu
def test_lanes_insertion_scan_to_column_0(oracle, monkeypatch):
    _lanes_over(monkeypatch, "insertion_col0")


@gpu
def test_lanes_walk_beside_unswept_rows(oracle, monkeypatch):
    _lanes_over(monkeypatch, "pruned_plane")


# ---------------------------------------------------------------- 2. every producer of the table, both walks

def _small():
    """`small` with the families as reference ids: (case of the simple scheme, its reference, ids per query)."""
    w = wc.world_small()
    refs, qs, cs, idx = w
    ids = [np.asarray(idx.famfinder(util.query_cseq(qs, qi))[0], np.uint32) for qi in range(6)]
    case = wc.Case("producers", refs.width, [[cs[i] for i in f] for f in ids], [qs.seq(qi) for qi in range(6)])
    return refs, case, ids


@pytest.fixture(scope="module")
def small_graphs(oracle):
    refs, case, ids = _small()
    return refs, case, wc.reference(case), ids


@pytest.fixture(scope="module")
def small_profiles(oracle):
    refs, case, ids = _small()
    case = wc.Case("producers-profile", refs.width, case.fams, case.qmasks, fs_no_graph=1)
    return refs, case, wc.reference(case), ids


def _fam_arrays(ids):
    foff = np.zeros(len(ids) + 1, np.uint64)
    foff[1:] = np.cumsum([len(f) for f in ids])
    return np.concatenate(ids), foff


@gpu
@pytest.mark.parametrize("lanes", (0, 1), ids=("waves", "lanes"))
def test_producer_device_dag_build(small_graphs, monkeypatch, lanes):
    refs, case, ref, ids = small_graphs
    qmask, qoff = _qarrays(case)
    util.set_knobs(monkeypatch, bt_lanes=lanes)
    ctx = capi.Context(0)
    try:
        ctx.upload_refs(refs.ab, refs.off, refs.width)
        fam, foff = _fam_arrays(ids)
        out, pos = ctx.align_families(fam, foff, qmask, qoff, _params(ctx, case))
    finally:
        ctx.close()
    _same_walk(out, pos, qoff, ref, ("device DAG build", lanes))


@gpu
@pytest.mark.parametrize("lanes", (0, 1), ids=("waves", "lanes"))
def test_producer_host_built_dag(small_graphs, monkeypatch, lanes):
    """build_family_graph (host/family_graph.cpp): what the aligner hands to sina_hip_align_graphs with device-graph off."""
    refs, case, ref, ids = small_graphs
    qmask, qoff = _qarrays(case)
    st = pipeline.Store(":mem:onetrip-host", refs)
    try:
        graphs = [st.build_graph(f, case.opts["fs_weight"]) for f in ids]
    finally:
        st.close()
    util.set_knobs(monkeypatch, bt_lanes=lanes)
    ctx = capi.Context(0)
    try:
        out, pos = ctx.align_graphs(ctx.graph_batch(graphs, case.width), qmask, qoff, _params(ctx, case))
    finally:
        ctx.close()
    _same_walk(out, pos, qoff, ref, ("host-built DAG", lanes))


@gpu
@pytest.mark.parametrize("lanes", (0, 1), ids=("waves", "lanes"))
def test_producer_caller_supplied_dag(small_graphs, monkeypatch, lanes):
    """The oracle's DAGs through sina_hip_align_graphs, in two launch ranges: the second range's tables are filled
    again from entry 0."""
    refs, case, ref, ids = small_graphs
    qmask, qoff = _qarrays(case)
    util.set_knobs(monkeypatch, bt_lanes=lanes, dp_range_q=4)
    ctx = capi.Context(0)
    try:
        gb = ctx.graph_batch([r["graph"] for r in ref], case.width)
        out, pos = ctx.align_graphs(gb, qmask, qoff, _params(ctx, case))
    finally:
        ctx.close()
    _same_walk(out, pos, qoff, ref, ("caller-supplied DAG", lanes))


@gpu
@pytest.mark.parametrize("lanes", (0, 1), ids=("waves", "lanes"))
def test_producer_profile_route(small_profiles, monkeypatch, lanes):
    """--fs-no-graph: the profile built on the device (sina_hip_align_profiles) and the host's tables through
    sina_hip_align_graphs."""
    refs, case, ref, ids = small_profiles
    qmask, qoff = _qarrays(case)
    util.set_knobs(monkeypatch, bt_lanes=lanes)
    ctx = capi.Context(0)
    try:
        ctx.upload_refs(refs.ab, refs.off, refs.width)
        fam, foff = _fam_arrays(ids)
        out, pos = ctx.align_profiles(fam, foff, qmask, qoff, _params(ctx, case))
        gb = ctx.graph_batch([r["graph"] for r in ref], case.width,
                             node_score16=np.concatenate([r["score16"] for r in ref]), self_score16=ref[0]["self16"])
        out2, pos2 = ctx.align_graphs(gb, qmask, qoff, _params(ctx, case))
    finally:
        ctx.close()
    _same_walk(out, pos, qoff, ref, ("device profile build", lanes))
    _same_walk(out2, pos2, qoff, ref, ("host profile tables", lanes))
