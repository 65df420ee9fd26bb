"""The inputs of the wide-path tests, shared by tests/test_wide_cpu.py (which asserts that every case reaches the edge it
is there for) and tests/test_gpu_wide.py (which runs them through sina_hip_align_graphs_any / sina_hip_debug_mesh_wide).
The DAGs are hand-built numpy arrays -- shapes the fast DP kernel refuses --, handed to the oracle's so_mesh_compute as
a pyoracle.Graph; tests/walk_ref.walk walks its planes.  Everything here is CPU work."""
import ctypes as C
import functools

import numpy as np

from oracle import pyoracle as po
from tests import walk_ref

BASES = np.array([1, 2, 4, 8], np.uint8)


def make_graph(preds, mask, pos=None, weight=None, width=None):
    """A DAG in the layout of util.graph_dict from per-node predecessor lists (ascending ids, all smaller than the
    node's): pos (default: the node id), mask, weight (default 1), pred / succ CSR, sources, sinks, succ_minpos."""
    n = len(preds)
    pos = np.arange(n, dtype=np.uint32) if pos is None else np.asarray(pos, np.uint32)
    pred_off = np.zeros(n + 1, np.uint32)
    pred_off[1:] = np.cumsum([len(p) for p in preds])
    pred = np.concatenate([np.asarray(p, np.uint32) for p in preds]) if pred_off[-1] else np.zeros(0, np.uint32)
    node = np.repeat(np.arange(n, dtype=np.uint32), np.diff(pred_off))
    assert (pred < node).all()
    order = np.lexsort((node, pred))            # successors of a node, ascending
    succ = node[order]
    succ_off = np.zeros(n + 1, np.uint32)
    succ_off[1:] = np.cumsum(np.bincount(pred, minlength=n))
    succ_min = np.full(n, 1000000, np.uint32)
    np.minimum.at(succ_min, pred, pos[node])
    return dict(n=n, width=int(width if width is not None else pos.max() + 1), pos=pos, mask=np.asarray(mask, np.uint8),
                weight=np.ones(n, np.float32) if weight is None else np.asarray(weight, np.float32),
                pred_off=pred_off, pred=pred, succ_off=succ_off, succ=succ.astype(np.uint32),
                src=np.flatnonzero(np.diff(pred_off) == 0).astype(np.uint32),
                snk=np.flatnonzero(np.diff(succ_off) == 0).astype(np.uint32), succ_minpos=succ_min)


def chain_preds(n):
    return [[]] + [[m - 1] for m in range(1, n)]


def oracle_planes(g, qmask, opts=None, prof=None):
    """The oracle's cell planes [N, L] of a hand-built DAG (prof: [n, 6] profile columns of a --fs-no-graph case)."""
    u32p, u8p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    keep = {k: np.ascontiguousarray(g[k]) for k in ("pos", "mask", "weight", "pred_off", "pred", "succ_off", "succ", "src", "snk")}
    ptr = lambda k, t: keep[k].ctypes.data_as(t)  # noqa: E731
    G = po.Graph()
    G.n, G.width = g["n"], g["width"]
    G.pos, G.mask, G.weight = ptr("pos", u32p), ptr("mask", u8p), ptr("weight", f32p)
    G.pred_off, G.pred, G.succ_off, G.succ = ptr("pred_off", u32p), ptr("pred", u32p), ptr("succ_off", u32p), ptr("succ", u32p)
    G.n_src, G.src, G.n_snk, G.snk = len(keep["src"]), ptr("src", u32p), len(keep["snk"]), ptr("snk", u32p)
    if prof is not None:
        keep["prof"] = np.ascontiguousarray(prof, np.float32)
        G.prof = keep["prof"].ctypes.data_as(f32p)
    qm = np.asarray(qmask, np.uint8)
    q = np.ascontiguousarray(np.arange(len(qm), dtype=np.uint32) | (qm.astype(np.uint32) << 24))
    cells = np.zeros((g["n"], len(qm)), po.CELL_DTYPE)
    opts = opts or po.align_opts()
    po.lib().so_mesh_compute(C.byref(G), q.ctypes.data_as(u32p), len(q), C.byref(opts), cells.ctypes.data_as(C.c_void_p))
    return cells


class WideCase:
    """One DAG with its queries.  limit: the fast path's limit every query of the case exceeds (None: it fits);
    plane_check: small enough to compare whole planes."""

    def __init__(self, name, graph, qmasks, limit=None, plane_check=True):
        self.name, self.graph, self.limit, self.plane_check = name, graph, limit, plane_check
        self.qmasks = [np.asarray(m, np.uint8) for m in qmasks]
        self.width = graph["width"]


# the scoring variants the planes are compared under: simple, weighted, forbid, weighted + forbid
def variants(width, max_len):
    w = np.random.default_rng(77).uniform(0.2, 1.5, size=width + max_len + 8).astype(np.float32)
    return [("simple", dict()), ("weighted", dict(weights=w)), ("forbid", dict(insertion=1)),
            ("weighted-forbid", dict(weights=w, insertion=1))]


FAN_SINGLES, FAN_VIA = 300, 280


@functools.lru_cache(maxsize=None)
def fan_in():
    """300 single nodes feed one node, a 20-node chain follows.  The singles hang off one root: rows without
    predecessors are 1 in every column, so 300 SOURCES would tie and the first would always win -- behind a root
    their rows differ by their masks.  Node 0 the root, 1..300 the singles, 301 the node with 300 predecessors,
    302..321 the chain.  Only single 280 (ordinal 279 of node 301) carries the query's second base."""
    rng = np.random.default_rng(901)
    n = 1 + FAN_SINGLES + 1 + 20
    preds = [[]] + [[0]] * FAN_SINGLES + [list(range(1, FAN_SINGLES + 1))] + [[m - 1] for m in range(FAN_SINGLES + 2, n)]
    mask = np.empty(n, np.uint8)
    mask[0] = 1
    mask[1:FAN_SINGLES + 1] = 2
    mask[FAN_VIA] = 8
    mask[FAN_SINGLES + 1:] = rng.choice(BASES, size=21)
    pos = np.concatenate([[0], 1 + np.arange(FAN_SINGLES), FAN_SINGLES + 1 + np.arange(21)]).astype(np.uint32)
    g = make_graph(preds, mask, pos=pos)
    q = np.concatenate([[1, 8], mask[FAN_SINGLES + 1:]]).astype(np.uint8)
    return WideCase("fan-in", g, [q], limit="predecessors")


CHAIN_N, CHAIN_END = 66000, 65791


@functools.lru_cache(maxsize=None)
def long_chain():
    """66 000 nodes in a chain, a 12-base query that is the chain's nodes 65780 .. 65791."""
    rng = np.random.default_rng(902)
    mask = rng.choice(BASES, size=CHAIN_N)
    g = make_graph(chain_preds(CHAIN_N), mask)
    return WideCase("long-chain", g, [mask[CHAIN_END - 11:CHAIN_END + 1]], limit="nodes", plane_check=False)


FAR_N, FAR_STEP, FAR_AT = 33300, 200, 20000


@functools.lru_cache(maxsize=None)
def far_edges():
    """A chain of 33 300 nodes with an extra edge m-200 -> m for every m: every row with such a successor is further
    than kFarLds = 192 rows from it and takes a spill row, 33 100 of them.  The query is six nodes before and six
    nodes behind one far edge."""
    rng = np.random.default_rng(903)
    mask = rng.choice(BASES, size=FAR_N)
    preds = [[]] + [([m - FAR_STEP] if m >= FAR_STEP else []) + [m - 1] for m in range(1, FAR_N)]
    g = make_graph(preds, mask)
    q = np.concatenate([mask[FAR_AT - 5:FAR_AT + 1], mask[FAR_AT + FAR_STEP:FAR_AT + FAR_STEP + 6]])
    return WideCase("far-edges", g, [q], limit="spill rows", plane_check=False)


@functools.lru_cache(maxsize=None)
def long_query():
    """10 241 bases against a chain of 40 nodes (the chain's bases sit in the middle of the query)."""
    rng = np.random.default_rng(904)
    mask = rng.choice(BASES, size=40)
    g = make_graph(chain_preds(40), mask)
    q = rng.choice(BASES, size=10241)
    q[5000:5040] = mask
    return WideCase("long-query", g, [q], limit="query length")


@functools.lru_cache(maxsize=None)
def long_diagonal():
    """L > N with diagonals of 1100 cells, more than the 1024 threads of a workgroup: a mutated copy of a chain of 1100
    nodes with 200 bases spliced in."""
    rng = np.random.default_rng(905)
    mask = rng.choice(BASES, size=1100)
    g = make_graph(chain_preds(1100), mask)
    q = mask.copy()
    mut = rng.random(len(q)) < 0.05
    q[mut] = rng.choice(BASES, size=int(mut.sum()))
    q = np.concatenate([q[:400], rng.choice(BASES, size=200), q[400:]])
    return WideCase("long-diagonal", g, [q])


@functools.lru_cache(maxsize=None)
def tiny():
    rng = np.random.default_rng(906)
    one = make_graph([[]], [1], width=4)
    five = make_graph(chain_preds(5), [1, 1, 1, 1, 1], width=8)
    # sources that are not the first rows: 0 -> 1 -> 2, source 3, 4 <- {2, 3}, source 5, 6 <- {4, 5}
    late = make_graph([[], [0], [1], [], [2, 3], [], [4, 5]], [1, 2, 4, 8, 1, 2, 4], pos=[0, 1, 2, 2, 3, 3, 4], width=9)
    # three equal nodes in a chain, two equal bases: rows 1 (not a sink) and 2 (the sink) tie in the last column
    tie = make_graph(chain_preds(3), [1, 1, 1], width=5)
    return [WideCase("tiny-1x1", one, [[1]]), WideCase("tiny-1x5", one, [[1, 2, 1, 8, 1]]),
            WideCase("tiny-5x1", five, [[1]]),
            WideCase("tiny-late-sources", late, [[8, 1, 2, 4], [2, 4], rng.choice(BASES, size=9)]),
            WideCase("tiny-end-tie", tie, [[1, 1]])]


def over_limit():
    return [fan_in(), long_chain(), far_edges(), long_query()]


def plane_cases():
    return [c for c in tiny() + [fan_in(), long_query(), long_diagonal()] if c.plane_check]


@functools.lru_cache(maxsize=None)
def reference(name, qi, variant="simple"):
    """(planes, plain walk) of query qi of the named case under a scoring variant, computed once per process."""
    case = by_name(name)
    kw = dict(variants(case.width, max(len(m) for m in case.qmasks)))[variant]
    planes = oracle_planes(case.graph, case.qmasks[qi], po.align_opts(**kw))
    wk = walk_ref.walk(case.graph, planes, case.qmasks[qi], case.width, walk_ref.opts_dict(weights=kw.get("weights")))
    return planes, wk


def by_name(name):
    for c in tiny() + [fan_in(), long_chain(), far_edges(), long_query(), long_diagonal()]:
        if c.name == name:
            return c
    raise KeyError(name)
