"""The passes behind the device DAG build's tile loop (family_graph_kernel steps 6-9) on the families of
tests/graph_rowpass_cases.py against the plain build of tests/graph_ref.py, bit for bit: the DAG, where every row is
kept, the row records' words, the predecessor entries, the size words, the chain, the row-skip bound -- for DAGs whose
rows' codes the kernel keeps in LDS with the column maxima beside them, in LDS alone, and in global memory; and whole
launches of such families through sina_hip_align_families against sina_hip_align_graphs on the plain DAGs, with and
without the successor minima (--insertion=forbid) and with and without the row-skip bound (one strip: none)."""
import numpy as np
import pytest

from sina_amd import capi
from tests import graph_cases as gc, graph_rowpass_cases as rc, util

pytestmark = pytest.mark.gpu

KAPPA64 = np.float32(64.0) * np.float32(1.0001) * np.float32(2.0)   # the debug entry's bound: the default scoring's


@pytest.fixture(scope="module")
def store():
    refs, fams = gc.refset(rc.CASES)
    ctx = capi.Context(0)
    ctx.upload_refs(refs.ab, refs.off, refs.width)
    yield ctx, dict(zip((c.name for c in rc.CASES), fams)), refs
    ctx.close()


@pytest.mark.parametrize("case", rc.CASES, ids=[c.name for c in rc.CASES])
def test_row_passes_equal_the_plain_build(store, case):
    ctx, fams, _ = store
    ids = fams[case.name]
    o = case.graph()
    want_r, want_c, want_gmin = rc.bound_of(o, KAPPA64)
    for ring in rc.rings_of(case):
        what = (case.name, ring, rc.fit(o["n"], len(ids)))
        want = case.words(ring)
        g = ctx.debug_family_graph(ids, 1.0, ring)
        chain = ctx.chain_rows()
        r, c = ctx.rgain(g["n"])
        assert g["n"] == o["n"], what
        assert (g["pos"] == o["pos"]).all() and (g["mask"] == o["mask"]).all(), what
        assert (util.f32_bits(g["weight"]) == util.f32_bits(o["weight"])).all(), what
        assert (g["pred_off"] == o["pred_off"]).all() and (g["pred"] == o["pred"]).all(), what
        assert (g["succ_minpos"] == o["succ_minpos"]).all() and (g["sink"] == o["sink"]).all(), what
        assert (g["spill"] == want["store"]).all(), what
        assert len(chain) == len(o["chain"]) and (chain == o["chain"]).all(), what
        assert (r == want_r).all() and (c == want_c).all(), what
        w = ctx.debug_family_graph_words(ids, 1.0, ring)
        assert (w["n"], w["status"], w["n_spill"], w["first_sink"], w["chain_len"], w["gmin"]) == \
            (want["n"], 0, want["n_spill"], want["first_sink"], want["chain_len"], want_gmin), what
        assert len(w["z"]) == o["n"] and (w["z"] == want["z"]).all() and (w["store"] == want["store"]).all(), what
        assert len(w["pred"]) == len(want["pred"]) and (w["pred"] == want["pred"]).all(), what


def _pack(arrays, dt):
    off = np.zeros(len(arrays) + 1, np.uint64)
    off[1:] = np.cumsum([len(a) for a in arrays])
    return np.concatenate([np.asarray(a, dt) for a in arrays]), off


@pytest.mark.parametrize("strips", ["one-strip", "two-strips"])
@pytest.mark.parametrize("group", sorted(rc.GROUPS))
def test_launches_equal_align_graphs_on_the_plain_dags(store, monkeypatch, group, strips):
    """Families of one size whose codes are kept in every place, in one launch: with two strips the build emits the
    row-skip bound, with one it does not; --insertion=forbid reads the build's successor minima."""
    _, fams, refs = store
    cases = [rc.BY_NAME[n] for n in rc.GROUPS[group]]
    if strips == "two-strips":
        util.set_knobs(monkeypatch, geom="128,4")     # (a 300-base query takes two strips)
    ctx = capi.Context(0)                             # (a context of its own: the geometry is read when it is created)
    try:
        ctx.upload_refs(refs.ab, refs.off, refs.width)
        fam_ids, foff = _pack([fams[c.name] for c in cases], np.uint32)
        qm, qoff = _pack([rc.query_of(c, 300 if strips == "two-strips" else 60) for c in cases], np.uint8)
        for ins in (0, 1):
            p = ctx.params(insertion=ins)
            o1, p1 = ctx.align_graphs(ctx.graph_batch([c.graph() for c in cases], refs.width), qm, qoff, p)
            o2, p2 = ctx.align_families(fam_ids, foff, qm, qoff, p)
            if strips == "one-strip" or ins == 0:
                assert (ctx.dp_info(0)["prune_step"] > 0) == (strips == "two-strips")
            assert (o1["status"] == 0).all()
            bad = [c.name for i, c in enumerate(cases)
                   if o1[i].tobytes() != o2[i].tobytes() or (p1[int(qoff[i]):int(qoff[i + 1])] != p2[int(qoff[i]):int(qoff[i + 1])]).any()]
            assert not bad, (ins, bad)
    finally:
        ctx.close()
