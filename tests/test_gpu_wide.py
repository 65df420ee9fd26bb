"""The wide DP path on the GPU: sina_hip_align_graphs_any, sina_hip_debug_mesh_wide and the aligner's wide-fallback
option, against the oracle's planes and the plain walk of tests/walk_ref.py on hand-built DAGs the fast kernel refuses
(tests/wide_cases.py; tests/test_wide_cpu.py asserts that each reaches its edge)."""
import numpy as np
import pytest

from sina_amd import capi, pipeline, synth
from tests import util, walk_cases as wc, walk_ref, wide_cases as wd
from tests.util import check_trays

pytestmark = pytest.mark.gpu

_WALK_FIELDS = ("end_m", "end_s", "cutoff_head", "cutoff_tail", "aligned_bases", "n_out")
_ASM_FIELDS = ("assembled", "nast_total", "nast_longest", "nast_last_run")


@pytest.fixture
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _qoff(qmasks):
    off = np.zeros(len(qmasks) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in qmasks])
    return off


def _same_as_walk(o, pos, wk, tag):
    """Check 1 of tests/test_gpu_walk.py: every field, raw and sum_weight by their bits, out_pos entry for entry."""
    assert o["status"] == 0, tag
    for f in _WALK_FIELDS:
        assert int(o[f]) == int(wk[f]), tag + (f, int(o[f]), int(wk[f]))
    assert util.f32_bits(o["raw"]) == util.f32_bits(wk["raw"]), tag + ("raw", o["raw"], wk["raw"])
    assert util.f32_bits(o["sum_weight"]) == util.f32_bits(wk["sum_weight"]), tag + ("sum_weight", o["sum_weight"], wk["sum_weight"])
    assert all(int(o[f]) == 0 for f in _ASM_FIELDS), tag
    bad = np.flatnonzero(pos[:int(o["n_out"])].astype(np.int64) != wk["cols"])
    assert len(bad) == 0, tag + ("out_pos differs first at append %d of %d" % (bad[0], wk["n_out"]),)


# ---------------------------------------------------------------- planes

_PLANE_IDS = [(c.name, qi, v) for c in wd.plane_cases() for qi in range(len(c.qmasks))
              for v in ("simple", "weighted", "forbid", "weighted-forbid")]


@pytest.mark.parametrize("name,qi,variant", _PLANE_IDS, ids=["%s-q%d-%s" % t for t in _PLANE_IDS])
def test_planes_equal_the_oracle(oracle, ctx, name, qi, variant):
    case = wd.by_name(name)
    kw = dict(wd.variants(case.width, max(len(m) for m in case.qmasks)))[variant]
    planes, _ = wd.reference(name, qi, variant)
    gb = ctx.graph_batch([case.graph], case.width)
    vm, vs, val = ctx.debug_mesh_wide(gb, case.qmasks[qi], ctx.params(**kw))
    assert (util.f32_bits(val) == util.f32_bits(planes["value"])).all()
    assert (vm == planes["value_midx"]).all() and (vs == planes["value_sidx"]).all()


@pytest.mark.parametrize("insertion", [0, 1])
def test_profile_planes_equal_the_oracle(oracle, ctx, insertion):
    case, _ = wc.group("matrix")[wc.MATRIX_NAMES.index("matrix-profile")]
    g, tab, self16 = wc.profile_tables(case.fams[0], case.opts)
    qm = case.oracle_masks(0)
    planes = wd.oracle_planes(g, qm, oracle.align_opts(fs_no_graph=1, insertion=insertion), prof=g["prof"])
    gb = ctx.graph_batch([g], case.width, node_score16=tab, self_score16=self16)
    vm, vs, val = ctx.debug_mesh_wide(gb, qm, ctx.params(insertion=insertion))
    assert (util.f32_bits(val) == util.f32_bits(planes["value"])).all()
    assert (vm == planes["value_midx"]).all() and (vs == planes["value_sidx"]).all()


# ---------------------------------------------------------------- shapes over the fast path's limits

@pytest.mark.parametrize("name", ["fan-in", "long-chain", "far-edges", "long-query"])
def test_over_limit_shapes(oracle, ctx, name):
    case = wd.by_name(name)
    gb = ctx.graph_batch([case.graph] * len(case.qmasks), case.width)
    qoff, qmask = _qoff(case.qmasks), np.concatenate(case.qmasks)
    with pytest.raises(capi.SinaHipError):       # (existing behaviour: the shape IS over the limit)
        ctx.align_graphs(gb, qmask, qoff)
    assert ctx.last_error_is_limit()
    before = ctx.wide_queries()
    out, pos = ctx.align_graphs_any(gb, qmask, qoff)
    assert ctx.wide_queries() - before == len(case.qmasks)
    for q in range(len(case.qmasks)):
        _same_as_walk(out[q], pos[int(qoff[q]):], wd.reference(name, q)[1], (name, q))


def test_mixed_batch_routes_per_query(oracle, ctx):
    """Fitting queries of `small` interleaved with over-limit ones: the fitting ones give the bytes align_graphs gives
    for them alone, wide_queries counts only the others; once with out_pos == NULL, read from the staged buffer.
    far-edges passes the cheap limits and fails the spill-row limit in the MIDDLE of a fast run, two fitting queries
    before it and one behind: the run is split there."""
    case, ref = wc.group("matrix")[0]
    width = 40000     # (one width per batch: wide enough for every DAG of the mix; it only mirrors the columns)
    assert width >= case.width
    fit = [(ref[q]["graph"], case.qmasks[q]) for q in range(4)]
    over = [(c.graph, c.qmasks[0]) for c in (wd.fan_in(), wd.long_query(), wd.far_edges())]
    mixed = [fit[0], over[0], over[1], fit[1], fit[2], over[2], fit[3]]
    is_over = [False, True, True, False, False, True, False]
    p = ctx.params(overhang=case.opts["overhang"], lowercase=case.opts["lowercase"], insertion=0)
    gb_fit = ctx.graph_batch([g for g, _ in fit], width)
    alone, alone_pos = ctx.align_graphs(gb_fit, np.concatenate([m for _, m in fit]), _qoff([m for _, m in fit]), p)
    alone_off = _qoff([m for _, m in fit])
    gb = ctx.graph_batch([g for g, _ in mixed], width)
    qoff, qmask = _qoff([m for _, m in mixed]), np.concatenate([m for _, m in mixed])
    for staged in (False, True):
        before = ctx.wide_queries()
        out, pos = ctx.align_graphs_any(gb, qmask, qoff, p, staged=staged)
        assert ctx.wide_queries() - before == sum(is_over)
        k = 0
        for q, (g, m) in enumerate(mixed):
            got = pos[int(qoff[q]):int(qoff[q + 1])]
            if is_over[q]:
                planes = wd.oracle_planes(g, m)
                wk = walk_ref.walk(g, planes, m, width, walk_ref.opts_dict(overhang=case.opts["overhang"]))
                _same_as_walk(out[q], got, wk, ("mixed", staged, q))
            else:
                assert out[q].tobytes() == alone[k].tobytes(), ("mixed", staged, q)
                n = int(out[q]["n_out"])
                assert (got[:n] == alone_pos[int(alone_off[k]):int(alone_off[k]) + n]).all(), ("mixed", staged, q)
                k += 1


# ---------------------------------------------------------------- wide = 1 over the existing walk cases

def _run_any(ctx, case, ref, **kw):
    graphs = [r["graph"] for r in ref]
    tabs = dict(node_score16=np.concatenate([r["score16"] for r in ref]), self_score16=ref[0]["self16"]) \
        if case.opts["fs_no_graph"] else {}
    gb = ctx.graph_batch(graphs, case.width, **tabs)
    qoff, qmask = _qoff(case.qmasks), np.concatenate(case.qmasks)
    popts = {k: v for k, v in case.opts.items() if k not in ("fs_no_graph", "weights")}
    out, pos = ctx.align_graphs_any(gb, qmask, qoff, ctx.params(weights=case.opts["weights"], **popts), **kw)
    return out, pos, qoff


@pytest.mark.parametrize("group", ["matrix", "insertion_col0", "overhang_clamps", "many_predecessors"])
def test_every_query_wide_over_the_walk_cases(oracle, ctx, monkeypatch, group):
    util.set_knobs(monkeypatch, wide=1)
    for case, ref in wc.group(group):
        before = ctx.wide_queries()
        out, pos, qoff = _run_any(ctx, case, ref)
        assert ctx.wide_queries() - before == len(ref)
        for q, r in enumerate(ref):
            _same_as_walk(out[q], pos[int(qoff[q]):], r["walk"], (case.name, q))


# ---------------------------------------------------------------- the budget

def _mesh_cells(n, L):
    return (n + L - 1) * min(n, L)


def test_wide_cells_splits_a_launch_and_refuses_a_query_beyond_it(oracle, ctx, monkeypatch):
    case, ref = wc.group("matrix")[0]
    case5 = wc.Case("five", case.width, case.fams[:5], case.qmasks[:5], **case.opts)
    ref5 = ref[:5]
    cells = [_mesh_cells(r["graph"]["n"], len(m)) for r, m in zip(ref5, case5.qmasks)]
    util.set_knobs(monkeypatch, wide=1)
    whole, whole_pos, _ = _run_any(ctx, case5, ref5)
    launches = ctx.stats()["dp_launches"]
    util.set_knobs(monkeypatch, wide_cells=max(cells) + min(cells) // 2)     # at most one query and a half per launch
    split, split_pos, _ = _run_any(ctx, case5, ref5)
    assert ctx.stats()["dp_launches"] - launches >= 3
    assert split.tobytes() == whole.tobytes() and (split_pos == whole_pos).all()
    util.set_knobs(monkeypatch, wide_cells=max(cells) - 1)
    with pytest.raises(capi.SinaHipError) as err:
        _run_any(ctx, case5, ref5)
    assert str(max(cells) * 28) in str(err.value), str(err.value)
    assert not ctx.last_error_is_limit()


def test_malformed_graph_is_still_rejected(ctx):
    g = dict(pos=[0, 1], mask=[1, 2], weight=[1.0, 1.0], pred_off=[0, 0, 1], pred=[1])     # node 1 its own predecessor
    gb = ctx.graph_batch([g], 4)
    with pytest.raises(capi.SinaHipError, match="predecessor ids"):
        ctx.align_graphs_any(gb, np.array([1, 2], np.uint8), _qoff([[1, 2]]))
    assert not ctx.last_error_is_limit()


# ---------------------------------------------------------------- the aligner stage with wide-fallback on

def _packed(cols, masks):
    return (np.asarray(cols, np.uint32) | (np.asarray(masks, np.uint32) << 24)).astype(np.uint32)


def _world_with(special, width, seed):
    """400 ordinary references of 320 bases with the hand-built `special` ones (packed aligned sequences) behind them."""
    refs = synth.make_refs(400, length=320, width=width, seed=seed, amb_rate=0.01)
    seqs = [refs.seq(i) for i in range(refs.n)] + special
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return refs, synth.RefSet(ab=np.concatenate(seqs), off=off, width=width)


def _stage_run(oracle, allrefs, ordinary, special_q, ff, off_ff, name):
    cs = util.cseqs_from_refs(allrefs)
    idx = oracle.Index(cs, k=10)
    qs = synth.make_queries(ordinary, 5, seed=97)
    masks = [qs.seq(i) for i in range(3)] + [special_q] + [qs.seq(i) for i in range(3, 5)]
    off = np.zeros(len(masks) + 1, np.int64)
    off[1:] = np.cumsum([len(m) for m in masks])
    batch = synth.QuerySet(mask=np.concatenate(masks), off=off, src=np.zeros(len(masks), np.int64))
    # the special query's family as the oracle picks it, and its DAG
    ids, _, _ = idx.famfinder(util.query_cseq(batch, 3, upper=False), oracle.ff_opts(**off_ff))
    g = util.graph_dict([cs[i] for i in ids])
    st = pipeline.Store(":mem:gpu-wide-" + name, allrefs)
    try:
        pl = pipeline.Pipeline(st, famfinder=ff, aligner={"wide-fallback": True})
        pl.run(batch.mask, batch.off, batch=len(masks), inflight=1)
        n_dp = check_trays(oracle, batch, pl, cs, idx, off_ff)
        assert n_dp >= len(masks) - 1 and pl.result(3)["status"] == 0
        pl.close()
    finally:
        st.close()
    return g, ids


def test_stage_family_of_300(oracle):
    """300 members, each one base in a column of its own and a shared 160-base tail: the family's DAG has a node with
    300 predecessors.  A family of more than 128 takes the host-graph route, with wide-fallback through
    sina_hip_align_graphs_any."""
    rng = np.random.default_rng(951)
    width = 3200
    tail = rng.choice(wd.BASES, size=160)
    special = [_packed(np.concatenate([[i], 1000 + np.arange(160)]), np.concatenate([[wd.BASES[i % 4]], tail])) for i in range(300)]
    ordinary, allrefs = _world_with(special, width, seed=952)
    q = np.concatenate([[4], tail]).astype(np.uint8)
    q[[40, 90, 130]] = [wd.BASES[(list(wd.BASES).index(b) + 1) % 4] for b in q[[40, 90, 130]]]   # (not a member's substring)
    ff = {"fs-min-len": 50, "fs-full-len": 100, "fs-min": 300, "fs-max": 300}
    g, ids = _stage_run(oracle, allrefs, ordinary, q, ff, dict(fs_min_len=50, fs_full_len=100, fs_min=300, fs_max=300), "fam300")
    assert len(ids) == 300 and (np.asarray(ids) >= 400).all()
    assert g["n"] == 460 and np.diff(g["pred_off"].astype(np.int64)).max() == 300


def test_stage_family_the_device_build_refuses(oracle):
    """40 members of 1900 bases in disjoint column ranges: a DAG of more than 65535 nodes.  sina_hip_align_families
    refuses it as over its limits; with wide-fallback the group is redone over host-built graphs."""
    rng = np.random.default_rng(953)
    n_mem, length = 40, 1900
    width = n_mem * length + 4000
    special = [_packed(4000 + m * length + np.arange(length), rng.choice(wd.BASES, size=length)) for m in range(n_mem)]
    ordinary, allrefs = _world_with(special, width, seed=954)
    q = (special[0][700:910] >> 24).astype(np.uint8)
    mut = [20, 75, 140, 190]
    q[mut] = [wd.BASES[(list(wd.BASES).index(b) + 1) % 4] for b in q[mut]]
    g, ids = _stage_run(oracle, allrefs, ordinary, q, {"fs-min-len": 100, "fs-full-len": 250}, dict(fs_min_len=100, fs_full_len=250), "fam66k")
    assert len(ids) <= 128 and g["n"] > 65535
