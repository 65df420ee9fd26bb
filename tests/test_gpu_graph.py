"""The device DAG build (family_graph_kernel) on the named families of tests/graph_cases.py against the plain build of
tests/graph_ref.py: the DAG, the raw words the DP kernel is handed (sina_hip_debug_family_graph_words), the first
member's chain; every case of a store in ONE sina_hip_align_families launch against sina_hip_align_graphs on the plain
DAGs; the cheap cases through the profile kernel against the oracle's pseq; the refusal of a family without a base.
Everything is compared bit for bit."""
import numpy as np
import pytest

from sina_amd import capi
from tests import graph_cases as gc, graph_ref as gr, util

pytestmark = pytest.mark.gpu

SCORES = (-1.7, 0.9, 3.3, 0.7)   # a scheme whose terms are not representable (test_gpu_profile_device.py)


@pytest.fixture(scope="module")
def stores():
    """Per alignment width: a context with the cases' members uploaded as one store, and each case's family ids."""
    out, ctxs = {}, []
    for width, cases in gc.by_width():
        refs, fams = gc.refset(cases)
        ctx = capi.Context(0)
        ctxs.append(ctx)
        ctx.upload_refs(refs.ab, refs.off, refs.width)
        for case, ids in zip(cases, fams):
            out[case.name] = (ctx, ids, refs)
    yield out
    for ctx in ctxs:
        ctx.close()


@pytest.mark.parametrize("case", gc.CASES, ids=[c.name for c in gc.CASES])
def test_single_family_build_equals_the_plain_build(stores, case):
    """... for every ring depth and fs-weight: the DAG, where each row is kept, the chain of the first member, and the
    row records' z / w, the predecessor entries and the size words as they are."""
    ctx, ids, _ = stores[case.name]
    for fsw in gc.FS_WEIGHTS:
        o = case.graph(fsw)
        for ring in gc.RINGS:
            what = (case.name, fsw, ring)
            want = case.words(ring)
            g = ctx.debug_family_graph(ids, fsw, ring)
            chain = ctx.chain_rows()
            assert g["n"] == o["n"], what
            assert (g["pos"] == o["pos"]).all() and (g["mask"] == o["mask"]).all(), what
            assert (util.f32_bits(g["weight"]) == util.f32_bits(o["weight"])).all(), what
            assert (g["pred_off"] == o["pred_off"]).all() and (g["pred"] == o["pred"]).all(), what
            assert (g["succ_minpos"] == o["succ_minpos"]).all() and (g["sink"] == o["sink"]).all(), what
            assert (g["spill"] == want["store"]).all(), what
            assert len(chain) == len(o["chain"]) and (chain == o["chain"]).all(), what
            w = ctx.debug_family_graph_words(ids, fsw, ring)
            assert (w["n"], w["status"], w["n_spill"], w["first_sink"], w["chain_len"]) == \
                (want["n"], 0, want["n_spill"], want["first_sink"], want["chain_len"]), what
            assert len(w["z"]) == o["n"] and (w["z"] == want["z"]).all() and (w["store"] == want["store"]).all(), what
            assert len(w["pred"]) == len(want["pred"]) and (w["pred"] == want["pred"]).all(), what


def _pack(arrays, dt):
    off = np.zeros(len(arrays) + 1, np.uint64)
    off[1:] = np.cumsum([len(a) for a in arrays])
    return np.concatenate([np.asarray(a, dt) for a in arrays]), off


@pytest.mark.parametrize("width", [w for w, _ in gc.by_width()])
def test_mixed_launch_equals_align_graphs_on_the_plain_dags(stores, width):
    """All cases of a store in one sina_hip_align_families launch -- families of 1 and of 128 side by side, DAGs of 1 and of
    15 000 nodes, every family's predecessor area at its own offset -- against sina_hip_align_graphs handed the plain DAGs;
    with --insertion=forbid the kernel's successor minima are read too."""
    cases = dict(gc.by_width())[width]
    ctx = stores[cases[0].name][0]
    fam_ids, foff = _pack([stores[c.name][1] for c in cases], np.uint32)
    qm, qoff = _pack([gc.query_of(c) for c in cases], np.uint8)
    for ins, fsw in ((0, 1.0), (1, 2.5)):
        p = ctx.params(insertion=ins, fs_weight=fsw)
        o1, p1 = ctx.align_graphs(ctx.graph_batch([c.graph(fsw) for c in cases], width), qm, qoff, p)
        o2, p2 = ctx.align_families(fam_ids, foff, qm, qoff, p)
        assert (o1["status"] == 0).all()
        bad = [c.name for i, c in enumerate(cases)
               if o1[i].tobytes() != o2[i].tobytes() or (p1[int(qoff[i]):int(qoff[i + 1])] != p2[int(qoff[i]):int(qoff[i + 1])]).any()]
        assert not bad, (ins, fsw, bad)
        assert o1.tobytes() == o2.tobytes() and p1.tobytes() == p2.tobytes()


@pytest.mark.parametrize("case", [c for c in gc.CASES if c.profile], ids=[c.name for c in gc.CASES if c.profile])
def test_profile_kernel_on_the_cheap_cases(oracle, stores, case):
    """family_profile_kernel on the same families (members without a base, single bases, 128 members, bases without a
    base bit) against the oracle's pseq + base_profile::comp."""
    ctx, ids, refs = stores[case.name]
    cs = {int(i): oracle.Cseq.from_packed("m%d" % i, refs.seq(int(i)), refs.width) for i in set(ids.tolist())}
    assert util.check_profile_hook(oracle, ctx, cs, ids, SCORES) >= len(np.unique(case.graph()["pos"]))


def test_a_family_without_a_base_is_refused_before_any_launch():
    """No base, no node: sina_hip_align_families refuses (a plain error, not a limit) where the families' bases are added
    up, in front of every copy and launch -- alone, and beside a family that has bases.  (The profile of such a family
    still has the node of column 0: sina_hip_align_profiles has nothing to refuse.)"""
    seqs = [gc.mem([]), gc.mem([]), gc.mem(range(40))]
    refs, _ = gc.refset([gc.Case("no-base", seqs, None)])
    ctx = capi.Context(0)
    try:
        ctx.upload_refs(refs.ab, refs.off, refs.width)
        q = np.full(20, gc.A, np.uint8)
        launches_before = ctx.stats()["graph_launches"]
        for fams in ([[0]], [[0, 1]], [[2], [1, 0]]):
            ids, foff = _pack(fams, np.uint32)
            qm, qoff = _pack([q] * len(fams), np.uint8)
            with pytest.raises(capi.SinaHipError, match="align_families: a family without a single base"):
                ctx.align_families(ids, foff, qm, qoff, ctx.params())
            assert not ctx.last_error_is_limit()
        assert ctx.stats()["graph_launches"] == launches_before
        # the debug entries, which align nothing, show the DAG of no node -- as the plain build has it
        for fam in gc.NO_BASE_FAMILIES:
            ids = np.arange(len(fam), dtype=np.uint32) % 2
            want = gr.dp_words(gr.build(fam), 4)
            g, w = ctx.debug_family_graph(ids), ctx.debug_family_graph_words(ids)
            assert g["n"] == 0 and len(g["pred"]) == 0 and len(ctx.chain_rows()) == 0
            assert (w["n"], w["status"], w["n_spill"], w["first_sink"], w["chain_len"], len(w["z"]), len(w["pred"])) == \
                (0, 0, 0, want["first_sink"], 0, 0, 0)
        # ... and the same context goes on working
        o = gr.build([seqs[2]])
        g = ctx.debug_family_graph(np.array([2], np.uint32))
        assert g["n"] == 40 and (g["pos"] == o["pos"]).all()
        out, _ = ctx.align_families(np.array([2], np.uint32), np.array([0, 1], np.uint64), q, np.array([0, 20], np.uint64))
        assert out[0]["status"] == 0
    finally:
        ctx.close()
