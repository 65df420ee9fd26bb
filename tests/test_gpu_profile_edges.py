"""The device profile build (family_profile_kernel) on the named families of tests/profile_cases.py against the plain
build of tests/profile_ref.py, under every tile size a case names (SINA_HIP_TEST=profile_tile): the nodes' columns,
the table of match terms, the self terms (sina_hip_debug_family_profile) and the chain the DP kernel is handed, as it is
(sina_hip_debug_family_profile_words); the seeded fuzz families the same way; the host loop's capacity and counters
on the real numbers; cases of every family size, an all-empty family, a duplicate and a family above the first capacity
in ONE sina_hip_align_profiles launch against sina_hip_align_graphs on the plain tables and against the oracle.
Everything is compared bit for bit."""
import os

import numpy as np
import pytest

from sina_amd import capi
from tests import profile_cases as pc, profile_ref as pr, util

pytestmark = pytest.mark.gpu

DEFAULT_SCORES = (-2.0, 1.0, 5.0, 2.0)   # the scheme's arguments under the default options


def _uploaded(refs):
    ctx = capi.Context(0)
    ctx.upload_refs(refs.ab, refs.off, refs.width)
    return ctx


@pytest.fixture(scope="module")
def stores():
    """Per alignment width of the small cases: a context with the cases' members uploaded as one store, and each case's
    family ids."""
    out, ctxs = {}, []
    for width, cases in pc.by_width():
        refs, fams = pc.refset(cases)
        ctxs.append(_uploaded(refs))
        for case, ids in zip(cases, fams):
            out[case.name] = (ctxs[-1], ids)
    yield out
    for ctx in ctxs:
        ctx.close()


def _where(node, tile):
    """A node by its tile and its offset there (every store of the cases has room for the full tile)."""
    T = tile or pc.TILE_MAX
    return "node %d = tile %d (of %d nodes) + %d" % (node, node // T, T, node % T)


def _check(ctx, ids, case, tile, scores=pc.SCORES):
    """Both debug hooks on the family `ids` against the case's plain build."""
    b, (tab, own), w = case.build(), case.tables(scores), case.words()
    what = (case.name, tile)
    pos, sc, self16 = ctx.debug_family_profile(ids, *scores)
    assert len(pos) == b["n"], what
    bad = np.flatnonzero(pos != b["pos"])
    assert len(bad) == 0, (what, "columns: first difference at " + _where(int(bad[0]), tile))
    assert np.isposinf(sc[:, 0]).all(), what
    bad = np.argwhere(util.f32_bits(sc[:, 1:]) != util.f32_bits(tab[:, 1:]))
    assert len(bad) == 0, (what, "table: first difference at %s, mask %d: %r for %r; points %s" % (
        _where(int(bad[0][0]), tile), bad[0][1] + 1, sc[bad[0][0], bad[0][1] + 1], tab[bad[0][0], bad[0][1] + 1],
        b["points"][bad[0][0]].tolist()), "%d entries differ" % len(bad))
    assert (util.f32_bits(self16[1:]) == util.f32_bits(own[1:])).all() and self16[0] == 0, what
    g = ctx.debug_family_profile_words(ids)
    assert g["n"] == b["n"] and list(g["sizes"][:6]) == list(w["sizes"]), (what, g["sizes"])
    for key in ("rec", "succ_min", "pred"):
        assert g[key].shape == w[key].shape, (what, key)
        bad = np.argwhere(g[key] != w[key])
        assert len(bad) == 0, (what, "%s: first difference at %s: %r for %r" % (
            key, _where(int(bad[0][0]), tile), g[key][tuple(bad[0])], w[key][tuple(bad[0])]))


_SMALL = [(c, t) for c in pc.CASES if not c.fresh for t in c.tiles]


@pytest.mark.parametrize("case,tile", _SMALL, ids=["%s-%s" % (c.name, t or "host") for c, t in _SMALL])
def test_named_case_equals_the_plain_build(stores, monkeypatch, case, tile):
    ctx, ids = stores[case.name]
    util.set_knobs(monkeypatch, profile_tile=tile)
    _check(ctx, ids, case, tile)


_REAL = [c for c in pc.CASES if c.fresh]


@pytest.mark.parametrize("case", _REAL, ids=[c.name for c in _REAL])
def test_case_on_the_real_numbers_equals_the_plain_build(monkeypatch, case):
    """4096 and 4097 nodes on the first capacity, 6144 / 6145 / 12 288 / 12 289 on the full tile: a context of its own,
    no knob; one launch in the counters however often the kernel came."""
    util.set_knobs(monkeypatch, profile_tile=None)
    refs, (ids,) = pc.refset([case])
    ctx = _uploaded(refs)
    try:
        s0 = ctx.stats()
        _check(ctx, ids, case, None)
        s1 = ctx.stats()
        assert s1["graph_launches"] - s0["graph_launches"] == 2       # (the two hooks: a build each)
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", range(int(os.environ.get("SINA_FUZZ_SEEDS", "12"))))
def test_fuzz_family_equals_the_plain_build(monkeypatch, seed):
    case = pc.fuzz_case(seed)
    refs, (ids,) = pc.refset([case])
    ctx = _uploaded(refs)
    try:
        for tile in case.tiles:
            util.set_knobs(monkeypatch, profile_tile=tile)
            _check(ctx, ids, case, tile)
    finally:
        ctx.close()


# ---------------------------------------------------------------- the host loop

def _pack(arrays, dt):
    off = np.zeros(len(arrays) + 1, np.uint64)
    off[1:] = np.cumsum([len(a) for a in arrays])
    return np.concatenate([np.asarray(a, dt) for a in arrays]), off


def _both_routes(ctx, cases, fams, queries, width, **opts):
    """(out, pos) of align_graphs on the plain builds' chains and tables and of align_profiles on the ids, one launch each
    (test_gpu_profile_device._both_routes)."""
    tabs = [c.tables(DEFAULT_SCORES) for c in cases]
    gb = ctx.graph_batch([pr.chain_graph(c.build()["pos"]) for c in cases], width,
                         node_score16=np.concatenate([t[0] for t in tabs]), self_score16=tabs[0][1])
    qm, qoff = _pack(queries, np.uint8)
    ids, foff = _pack(fams, np.uint32)
    want = ctx.align_graphs(gb, qm, qoff, ctx.params(**opts))
    got = ctx.align_profiles(ids, foff, qm, qoff, ctx.params(**opts))
    return want, got, qoff


def _same_alignments(cases, want, got, qoff, what):
    (wout, wpos), (gout, gpos) = want, got
    bad = [c.name for i, c in enumerate(cases) if wout[i].tobytes() != gout[i].tobytes() or
           (wpos[int(qoff[i]):int(qoff[i + 1])] != gpos[int(qoff[i]):int(qoff[i + 1])]).any()]
    assert not bad, (what, bad)
    assert wout.tobytes() == gout.tobytes() and wpos.tobytes() == gpos.tobytes(), what


def test_capacity_grows_once_and_stays_grown(monkeypatch):
    """A fresh context: 4096 nodes fit the first arrays, 4097 have the kernel come again -- one launch and one profile in
    the counters per call either way -- and a short family after them is built in the arrays as they have grown."""
    util.set_knobs(monkeypatch, profile_tile=None)
    by_name = {c.name: c for c in pc.CASES}
    short = pc.widened(by_name["tile-cursor-hand-over"], 12800)
    cases = [by_name["host-4096-nodes"], by_name["host-4097-nodes"], short]
    refs, fams = pc.refset(cases)
    ctx = _uploaded(refs)
    try:
        for case, ids in zip(cases, fams):
            s0 = ctx.stats()
            want, got, qoff = _both_routes(ctx, [case], [ids], [pc.query_of(case)], refs.width)
            s1 = ctx.stats()
            assert (got[0]["status"] == 0).all(), case.name
            _same_alignments([case], want, got, qoff, case.name)
            assert s1["graph_launches"] - s0["graph_launches"] == 1 and s1["dags_built"] - s0["dags_built"] == 1, case.name
            assert s1["dags_used"] - s0["dags_used"] == 1 and s1["graph_ms"] > s0["graph_ms"], case.name
        for case, ids in zip(cases[::-1], fams[::-1]):
            _check(ctx, ids, case, None)
    finally:
        ctx.close()


_MIXED = ("chain-one-node", "chain-two-nodes", "members-8-one-per-wave", "count-128-same-base", "count-127-gaps-open",
          "count-128-gaps-extend", "host-4097-nodes", "tile-cursor-hand-over", "bitless-walk-back-across-a-tile",
          "tile-open-on-next-tiles-first-node", "tile-stretch-clamped-to-n0", "length-257", "same-reference-twice")


@pytest.mark.parametrize("tile", [None, 64], ids=["host", "64"])
def test_several_families_in_one_launch(oracle, monkeypatch, tile):
    """Families of 1, 2, 3, 8 and 128 members, of 1 node and of 4097 (more than the first arrays hold, in a fresh
    context: the whole launch comes again for the one family), a family without a base and one family twice, in ONE
    sina_hip_align_profiles launch -- max_f lays out the LDS for all of them -- against sina_hip_align_graphs on the plain
    builds; --insertion shift and forbid (the kernel's successor columns are read), assemble 0 and 1."""
    util.set_knobs(monkeypatch, profile_tile=tile)
    by_name = {c.name: c for c in pc.CASES}
    cases = [pc.widened(by_name[n], 12800) for n in _MIXED]
    refs, fams = pc.refset(cases)
    cases.append(cases[2])            # (the same ordered family again, with another query: one profile for both)
    fams.append(fams[2])
    queries = [pc.query_of(c, salt=i % 3) for i, c in enumerate(cases)]
    assert sorted({len(f) for f in fams}) == [1, 2, 3, 8, 128] and len(cases[0].family()[0]) == 0
    assert sorted(c.build()["n"] for c in cases)[::len(cases) - 1] == [1, 4097]
    ctx = _uploaded(refs)
    try:
        res = {}
        for n_call, (ins, asm) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            s0 = ctx.stats()
            want, got, qoff = _both_routes(ctx, cases, fams, queries, refs.width, insertion=ins, assemble=asm)
            s1 = ctx.stats()
            _same_alignments(cases, want, got, qoff, (tile, ins, asm))
            assert (got[0]["status"][[len(q) >= 20 for q in queries]] == 0).all(), (tile, ins, asm)
            assert s1["graph_launches"] - s0["graph_launches"] == 1, n_call
            assert s1["dags_built"] - s0["dags_built"] == len(cases) - 1 and s1["dags_used"] - s0["dags_used"] == len(cases)
            res[ins, asm] = got
    finally:
        ctx.close()
    # ... and the oracle's alignment for a few of them (test_gpu_profile_device.py)
    n_asm = 0
    for ins in (0, 1):
        (plain, ppos), (fin, fpos) = res[ins, 0], res[ins, 1]
        for q in (2, 6, 12, len(cases) - 1):   # (two of them along the whole profile, two that keep one base)
            qm = queries[q]
            qc = oracle.Cseq.from_packed("q%d" % q, np.arange(len(qm), dtype=np.uint32) | (qm.astype(np.uint32) << 24), len(qm))
            fam = [oracle.Cseq.from_packed("m%d" % i, m, refs.width) for i, m in enumerate(cases[q].family())]
            want = oracle.align(fam, qc, oracle.align_opts(realign=1, fs_no_graph=1, insertion=ins))
            assert want["status"] == 0, (q, want["log"])
            o, lo = plain[q], int(qoff[q])
            assert (o["cutoff_head"], o["cutoff_tail"]) == (want["head"], want["tail"])
            assert util.f32_bits(np.float32(o["raw"]) / np.float32(o["sum_weight"])) == util.f32_bits(want["score"])
            packed, _ = util.finish_alignment(qm, o, ppos[lo:lo + int(o["n_out"])], refs.width, want_packed=True)
            assert packed is not None and (packed == want["packed"]).all(), (ins, q)
            if fin[q]["assembled"]:
                n_asm += 1
                assert (fpos[lo:lo + int(fin[q]["n_out"])] == want["packed"]).all(), (ins, q)
    assert n_asm > 0
