"""GPU tests of the scout pass inside the DP wave (mesh_dp.hip chain_scout_wave) and of the chain the DAG
build hands it (graph_build.hip, GraphArgs::chain_rows).  Every query's DP wave first aligns the query, in a band of
64 columns on a fixed diagonal, against the chain of its family's first member; the cost found is the first attempt's
bound U.  So: (a) the results never depend on it, (b) the value is the cost of a path that exists -- never below the
optimum -- and good enough that a lightly mutated query passes its first certificate, (c) against a family of ONE the
chain is the DAG and the value is the optimum, (d) the band's edges, (e) the chain is member 0's nodes.

Shapes: two strips at 8 columns per lane need L > 512, so references of 600 - 1100 bases, a few hundred of them,
8 - 32 queries per launch.  "The oracle's optimum" is the launch's own end value once its score has been checked
against the oracle's bit for bit (score = raw / sum_weight, both the launch's)."""
import math

import numpy as np
import pytest

from sina_amd import synth
from tests import util

pytestmark = pytest.mark.gpu


def _cseq(name, m):
    m = np.asarray(m, np.uint8)
    return util.po.Cseq.from_packed(name, np.arange(len(m), dtype=np.uint32) | (m.astype(np.uint32) << 24), len(m))


def _bases(refs, r):
    return ((refs.seq(int(r)) >> 24) & 0x0f).astype(np.uint8)


def _mutate(rng, m, sub=0.02, indels=0):
    """Substitutions at rate sub, and `indels` short (1 - 6 bases) insertions / deletions."""
    m = m.copy()
    hit = rng.random(len(m)) < sub
    m[hit] = rng.choice([1, 2, 4, 8], size=int(hit.sum()))
    for x in range(indels):
        at = int(rng.integers(20, len(m) - 20))
        n = int(rng.integers(1, 7))
        if x % 2:
            m = np.concatenate([m[:at], m[at + n:]])
        else:
            m = np.concatenate([m[:at], rng.choice([1, 2, 4, 8], size=n).astype(np.uint8), m[at:]])
    return m


@pytest.fixture(scope="module")
def world():
    refs = synth.make_refs(240, length=1100, width=8000, seed=71, n_clades=6, amb_rate=0.01)
    # three fragments of reference 0 as members of their own: chains of 40, and of 127 / 128 / 129 occupied columns
    frag = [refs.seq(0)[:n] for n in (40, 127, 128, 129)]
    ab = np.concatenate([refs.ab] + frag)
    off = np.concatenate([refs.off, refs.off[-1] + np.cumsum([len(f) for f in frag])])
    refs = synth.RefSet(ab=ab, off=off, width=refs.width)
    return refs, util.cseqs_from_refs(refs)


@pytest.fixture(scope="module")
def store(gpu_ctx, world):
    refs, cs = world
    gpu_ctx.upload_refs(refs.ab, refs.off, refs.width)
    gpu_ctx.build_index(10, False)
    return gpu_ctx


def _families(ctx, first, masks, n=6):
    """Per query: `first[i]` (the member whose chain the scout walks), then the query's nearest references."""
    qoff = np.zeros(len(masks) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(m) for m in masks])
    ids, _, cnt = ctx.kmer_topk(np.concatenate(masks), qoff, n)
    fams = []
    for i, r in enumerate(first):
        rest = [int(x) for x in ids[i, :cnt[i]] if int(x) != int(r) and int(x) < 240]
        fams.append(np.array([int(r)] + rest[:n - 1], np.uint32))
    return fams


def _launch(ctx, oracle, world, fams, masks):
    """One align_families launch, every tray against the oracle; returns per query (dp_info, optimum)."""
    refs, cs = world
    qoff = np.zeros(len(masks) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(m) for m in masks])
    foff = np.zeros(len(fams) + 1, np.uint64)
    foff[1:] = np.cumsum([len(f) for f in fams])
    out, pos = ctx.align_families(np.concatenate(fams), foff, np.concatenate(masks), qoff, ctx.params())
    res = []
    for i, (fam, m) in enumerate(zip(fams, masks)):
        want = oracle.align([cs[int(j)] for j in fam], _cseq("q%d" % i, m), oracle.align_opts(realign=1))
        o = out[i]
        assert want["status"] == 0 and o["status"] == 0, (i, want["log"])
        assert util.f32_bits(np.float32(o["raw"]) / np.float32(o["sum_weight"])) == util.f32_bits(want["score"]), i
        aligned, _ = util.finish_alignment(m, o, pos[int(qoff[i]):int(qoff[i + 1])], refs.width)
        assert aligned == want["aligned"], i
        res.append((ctx.dp_info(i), float(o["raw"])))
    return res


def _queries(world, seed, n, sub=0.02, indels=2, cut=None):
    refs, _ = world
    rng = np.random.default_rng(seed)
    first = [int(x) for x in rng.choice(240, size=n, replace=False)]
    masks = [_mutate(rng, _bases(refs, r)[:cut], sub, indels) for r in first]
    return first, masks


@pytest.mark.parametrize("mode", ["on", "off", "bold", "loose", "set"])
def test_results_do_not_depend_on_the_scout(oracle, store, world, monkeypatch, mode):
    """The preamble left alone, switched off, forced 300 units too bold and 400 too loose, and replaced by the
    optimum itself (scout_set: one value per launch, so one query per launch there)."""
    util.set_knobs(monkeypatch, geom="128,8")
    first, masks = _queries(world, 72, 12, cut=1000)
    fams = _families(store, first, masks)
    s0 = store.stats()["scout_launches"]
    if mode == "set":
        for i in range(3):
            util.set_knobs(monkeypatch, scout_set=None)
            (_, opt), = _launch(store, oracle, world, fams[i:i + 1], masks[i:i + 1])
            util.set_knobs(monkeypatch, scout_set=repr(opt))
            (info, opt2), = _launch(store, oracle, world, fams[i:i + 1], masks[i:i + 1])
            assert opt2 == opt and info["attempts"] == 1 and info["scout"] == np.float32(opt)
        return
    knobs = {"on": {}, "off": {"scout": "0"}, "bold": {"scout_add": "-300"}, "loose": {"scout_add": "400"}}[mode]
    util.set_knobs(monkeypatch, **knobs)
    res = _launch(store, oracle, world, fams, masks)
    ran = store.stats()["scout_launches"] - s0
    if mode == "off":
        assert ran == 0 and all(math.isnan(info["scout"]) for info, _ in res)
    else:
        assert ran == 1 and all(info["scout"] >= opt for info, opt in res)
    if mode == "bold":      # every certificate fails: second attempts under what the first found
        assert sum(info["attempts"] >= 2 for info, _ in res) >= len(res) - 1


def test_scout_is_a_real_paths_cost(oracle, store, world, monkeypatch):
    """Never below the optimum; lightly mutated queries pass their first certificate under it."""
    util.set_knobs(monkeypatch, geom="128,8")
    first, masks = _queries(world, 73, 24, sub=0.01, indels=1, cut=1000)
    res = _launch(store, oracle, world, _families(store, first, masks), masks)
    for i, (info, opt) in enumerate(res):
        print("query %d: scout %.3f optimum %.3f attempts %d" % (i, info["scout"], opt, info["attempts"]))
    for info, opt in res:
        assert info["scout"] >= opt
        assert info["attempts"] == 1


def test_family_of_one_scout_is_the_optimum(oracle, store, world, monkeypatch):
    """fs-min = fs-max = 1: the DAG is the chain.  Indels of up to six bases stay inside the band, so the value
    rounded up to a unit (1/64) is the optimum rounded up to a unit."""
    util.set_knobs(monkeypatch, geom="128,8")
    first, masks = _queries(world, 74, 8, sub=0.03, indels=4, cut=1000)
    res = _launch(store, oracle, world, [np.array([r], np.uint32) for r in first], masks)
    for i, (info, opt) in enumerate(res):
        print("query %d: scout %.4f optimum %.4f" % (i, info["scout"], opt))
    for info, opt in res:
        assert info["scout"] >= opt
        assert math.ceil(float(info["scout"]) * 64.0) == math.ceil(opt * 64.0)


EDGES = ["L513", "L1024", "L1025_three_strips", "longer", "shorter", "gap100", "short_chain", "column0", "iupac"]


@pytest.mark.parametrize("edge", EDGES)
def test_band_edges(oracle, store, world, monkeypatch, edge):
    refs, cs = world
    rng = np.random.default_rng(75 + EDGES.index(edge))
    long_enough = [r for r in range(240) if len(refs.seq(r)) >= 1030]
    r = int(long_enough[int(rng.integers(len(long_enough)))])
    src = _bases(refs, r)
    rnd = lambda n: rng.choice([1, 2, 4, 8], size=n).astype(np.uint8)  # noqa: E731
    first = r
    if edge in ("L513", "L1024", "L1025_three_strips"):
        m = _mutate(rng, src[:int(edge[1:].split("_")[0])], 0.02)
    elif edge == "longer":       # 45 bases more than its relative at either end: the band runs past the chain's ends
        m = np.concatenate([rnd(45), _mutate(rng, src, 0.02), rnd(45)])
    elif edge == "shorter":      # ... and 50 fewer
        m = _mutate(rng, src[50:len(src) - 50], 0.02)
    elif edge == "gap100":       # the relative has a 100-column gap the query does not share: the band loses the query
        m = np.concatenate([_mutate(rng, src[:400], 0.02), rnd(100), _mutate(rng, src[400:900], 0.02)])
    elif edge == "short_chain":  # the first member is a fragment of 40 bases: a chain shorter than a block of rows
        first = 240
        m = _mutate(rng, _bases(refs, 0)[:700], 0.02)
    elif edge == "column0":      # query and relative start together: column 0 sits in the band's middle at row 0
        m = _mutate(rng, src[:800], 0.0)
        m[5] ^= 3 if m[5] in (1, 2) else 12
    else:                        # rows with IUPAC masks: the relative's own ambiguity codes, and some in the query
        amb = [x for x in long_enough if (_bases(refs, x)[:1000] & (_bases(refs, x)[:1000] - 1)).any()]
        first = r = int(amb[0])
        m = _mutate(rng, _bases(refs, r)[:1000], 0.02)
        m[rng.random(len(m)) < 0.01] = 15
    # (two strips of 512 columns; three for the queries past 1024 bases)
    util.set_knobs(monkeypatch, geom="192,8" if len(m) > 1024 else "128,8")
    fams = _families(store, [first], [m])
    (info, opt), = _launch(store, oracle, world, fams, [m])
    print("%s: L %d scout %.3f optimum %.3f attempts %d" % (edge, len(m), info["scout"], opt, info["attempts"]))
    assert info["attempts"] >= 1 and not math.isnan(info["scout"])      # the skipping kernel, with the preamble
    assert info["scout"] >= opt


@pytest.mark.parametrize("fam", [[3, 50, 97, 140, 188, 230], [241, 7], [242, 7], [243, 7], [242], [5]])
def test_chain_rows_are_member_zeros_nodes(oracle, store, world, fam):
    """The DAG build's chain against the oracle's DAG: members from six clades (several characters per column), and
    first members of 127, 128 and 129 bases (the build's tile is 128 occupied columns; with reference 7 behind them the
    family's columns run on across the boundary)."""
    refs, cs = world
    g = util.graph_dict([cs[i] for i in fam])
    got = store.debug_family_graph(np.array(fam, np.uint32))
    assert got["n"] == g["n"] and (got["pos"] == g["pos"]).all() and (got["mask"] == g["mask"]).all()
    chain = store.chain_rows()
    ab = refs.seq(fam[0])
    node_of = {(int(p), int(k)): i for i, (p, k) in enumerate(zip(g["pos"], g["mask"]))}
    want = np.array([node_of[(int(x & 0xFFFFFF), int((x >> 24) & 31))] for x in ab], np.uint16)
    assert len(chain) == len(ab)
    assert (chain == want).all()
