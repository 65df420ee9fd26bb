"""Named families for the device DAG build's tests (family_graph_kernel, sina_amd/csrc/graph_build.hip), shared by
tests/test_graph_cpu.py (which asserts that every case sits on the edge it names) and tests/test_gpu_graph.py (which
runs them).  Everything here is CPU work on hand-built packed arrays (alignment column | iupac mask << 24 per base).

A case is a small store of its own (its members), the family as ids into it, the alignment width, and a predicate over
the plain build (tests/graph_ref.py) that says what the case is there for.  The kernel's numbers are restated here
from its source: kTC = 128 occupied columns per tile, kTNW = 512 nodes per LDS window, 64 near predecessors in one
word, kFarLds = 192, 12 288 nodes of first capacity, the LDS / global switch of steps 6-9 at graph_bitmap_off(F) bytes
of row codes, allocation segments of max(256, ceil(N / 16)) rows."""
import functools

import numpy as np

from sina_amd import synth
from tests import graph_ref as gr

A, G, C, U = 1, 2, 4, 8
TILE_COLS = 128        # kTC
WINDOW_NODES = 512     # kTNW
NEAR_BITS = 64         # predecessors at distance 1..64 are a bit each
FIRST_NCAP = 12288     # build_family_graphs' first node capacity
WIDTH = 6400
RINGS = (1, 3, 4, 5, 8)        # (the slot search is compiled for 4 and for 8 slots)
FS_WEIGHTS = (1.0, 0.0, 2.5)


def graph_bitmap_off(max_family):
    """graph_build.hip, graph_bitmap_off: the LDS bytes in front of the occupied-column bitmap = what steps 6-9 have
    for the rows' codes (4 bytes a row); the constants are the kernel's LDS carve (kOCpos .. kOE)."""
    o = 4 * TILE_COLS                                   # kONbase
    o += 4 * (TILE_COLS + 2)                            # kOPres
    o += 4 * TILE_COLS                                  # kOWA
    o += 3 * 4 * WINDOW_NODES                           # kOWC, kOWD, then kOWB on 8 bytes
    o = (o + 7) & ~7
    o += 8 * WINDOW_NODES                               # kOLi
    o += 32 * TILE_COLS                                 # kONn
    o += TILE_COLS                                      # kONfar
    o += 3 * WINDOW_NODES                               # kOMask, kONcol, then kOE on 16 bytes
    o = (o + 15) & ~15
    return (o + 2 * max_family * TILE_COLS + 15) & ~15


def slot_segment(n_rows):
    """common.h, dp_slot_segment"""
    return max(256, (n_rows + 15) // 16)


def mem(cols, masks=A):
    """A packed member: the columns (ascending) with one mask for all, or one each."""
    cols = np.asarray(list(cols), np.uint32)
    masks = np.full(len(cols), masks, np.uint32) if np.isscalar(masks) else np.asarray(list(masks), np.uint32)
    assert len(cols) == len(masks) and (masks < 32).all()
    return cols | (masks << np.uint32(24))


class Case:
    def __init__(self, name, members, edge, fam=None, width=WIDTH, profile=False, big=False):
        self.name, self.members, self.edge, self.width = name, [np.asarray(m, np.uint32) for m in members], edge, width
        self.fam = list(range(len(members))) if fam is None else list(fam)
        self.profile = profile   # cheap enough for the profile kernel's comparison as well
        self.big = big
        assert all(len(m) == 0 or int((m & 0xFFFFFF).max()) < width for m in self.members)

    def family(self):
        return [self.members[i] for i in self.fam]

    @functools.lru_cache(maxsize=None)
    def graph(self, fs_weight=1.0):
        return gr.build(self.family(), fs_weight)

    @functools.lru_cache(maxsize=None)
    def words(self, ring):
        return gr.dp_words(self.graph(), ring)

    def on_edge(self):
        return bool(self.edge(self.graph(), self))

    def __repr__(self):
        return self.name


def refset(cases):
    """One store for cases of one width, and every case's family as ids into it."""
    width = cases[0].width
    assert all(c.width == width for c in cases)
    seqs, fams = [], []
    for c in cases:
        fams.append(np.asarray([len(seqs) + i for i in c.fam], np.uint32))
        seqs += c.members
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    ab = np.concatenate(seqs).astype(np.uint32) if off[-1] else np.zeros(0, np.uint32)
    return synth.RefSet(ab=ab, off=off, width=int(width)), fams


def query_of(case):
    """Member 0 -- the first member that has a base -- with a few substitutions, as upper-case iupac masks with a base
    bit (what the aligner hands the device)."""
    m = next(m for m in case.family() if len(m))
    q = ((m >> 24) & 0x0F).astype(np.uint8)
    q[q == 0] = A
    q = q[:600]
    for i in range(2, len(q), 7):
        q[i] = {A: G, G: C, C: U}.get(int(q[i]), A)
    return q


# ---------------------------------------------------------------- what the predicates read off a plain build
def distances(g):
    node = np.repeat(np.arange(g["n"]), np.diff(g["pred_off"].astype(np.int64)))
    return node - g["pred"].astype(np.int64)


def n_columns(g):
    return len(np.unique(g["pos"]))


def tile_nodes(g, tile=0):
    """Nodes of the tile-th stretch of kTC occupied columns."""
    cols = np.unique(g["pos"])[tile * TILE_COLS:(tile + 1) * TILE_COLS]
    return int(np.isin(g["pos"], cols).sum())


def tile_of(g, node):
    return int(np.searchsorted(np.unique(g["pos"]), g["pos"][node])) // TILE_COLS


def spilled(case, ring, row):
    w = int(case.words(ring)["store"][row])
    return w != gr.ROW_NONE and (w & gr.ROW_SPILLED) != 0


def _fan_in(g, node):
    return distances(g)[int(g["pred_off"][node]):int(g["pred_off"][node + 1])]


def _cross_tile_far(g, d):
    dist = distances(g)
    node = np.repeat(np.arange(g["n"]), np.diff(g["pred_off"].astype(np.int64)))
    hit = np.flatnonzero(dist == d)
    return len(hit) == 1 and tile_of(g, node[hit[0]]) == tile_of(g, g["pred"][hit[0]]) + 1


def _cases():
    cs = []

    def add(*a, **kw):
        cs.append(Case(*a, **kw))

    # ---- the 64-bit "near predecessor" word: distance 64 is its last bit, 65 the first far predecessor
    add("pred-dist-64-65", [mem(range(80)), mem([0, 64]), mem([0, 65])],
        lambda g, c: {64, 65} <= set(distances(g)) and distances(g).max() == 65, profile=True)
    # ---- kFarLds: an edge of 192 rows may take a slot, one of 193 raises the fence flag and is always a spill row
    add("edge-192-193", [mem(range(400)), mem([0, 192]), mem([1, 194])],
        lambda g, c: sorted(set(distances(g)))[-2:] == [192, 193] and not c.words(8)["z"][0] & gr.REC_FENCE and
        c.words(8)["z"][1] & gr.REC_FENCE and not spilled(c, 8, 0) and spilled(c, 8, 1), profile=True)
    # ---- occupied columns around the tile's 128 (and its waves' 64)
    for k in (1, 63, 64, 65, 127, 128, 129, 256, 257):
        add("columns-%d" % k, [mem(range(0, 3 * k, 3), [(A, G, C, U)[i % 4] for i in range(k)]), mem(range(0, 3 * k, 9), U)],
            lambda g, c, k=k: n_columns(g) == k, profile=True)
    # ---- nodes per tile around the window's 512
    four = [mem(range(256), m) for m in (A, G, C, U)]
    add("tile-512-nodes", four, lambda g, c: tile_nodes(g, 0) == WINDOW_NODES and tile_nodes(g, 1) == WINDOW_NODES)
    add("tile-513-nodes", four + [mem([127], 16 | A)], lambda g, c: tile_nodes(g, 0) == WINDOW_NODES + 1)
    add("tile-31x128-nodes", [mem(range(128), m) for m in range(1, 32)],
        lambda g, c: g["n"] == 31 * TILE_COLS and tile_nodes(g, 0) == 31 * TILE_COLS and (distances(g) == 31).all())
    # ---- one node with 128 predecessors, 64 of them further back than the near word: dozens of far rounds
    add("fan-in-128", [mem([j, 300, 301]) for j in range(128)],
        lambda g, c: len(_fan_in(g, 128)) == 128 and int((_fan_in(g, 128) > NEAR_BITS).sum()) > 60, profile=True)
    add("fan-in-straddles-64", [mem([j, 300, 301]) for j in range(70)],
        lambda g, c: sorted(_fan_in(g, 70)) == list(range(1, 71)), profile=True)
    # ---- a far predecessor carried from the tile before
    add("carry-far-across-tiles", [mem(range(300), m) for m in (A, G, C)] + [mem([3, 200, 201], A)],
        lambda g, c: distances(g).max() == 591 and _cross_tile_far(g, 591))
    # ---- members of length 0 and 1
    add("empty-member-first", [mem([]), mem(range(5, 60)), mem(range(0, 50), G)],
        lambda g, c: len(g["chain"]) == 0 and g["n"] > 0, profile=True)
    add("empty-member-middle", [mem(range(5, 60)), mem([]), mem(range(0, 50), G)],
        lambda g, c: len(c.family()[1]) == 0 and len(g["chain"]) == 55, profile=True)
    add("single-base-member", [mem(range(50)), mem([25], G)], lambda g, c: len(c.family()[1]) == 1 and g["n"] == 51, profile=True)
    add("one-node", [mem([17], C)], lambda g, c: g["n"] == 1 and g["sink"][0] == 1 and len(g["pred"]) == 0, profile=True)
    add("same-reference-twice", [mem(range(3, 90, 2), [(A, C)[i % 2] for i in range(44)])], lambda g, c: c.fam == [0, 0] and
        g["n"] == 44 and (g["weight"] == gr.node_weight(2, 2, 1.0)).all(), fam=[0, 0], profile=True)
    add("128-identical-members", [mem(range(60), U) for _ in range(128)],
        lambda g, c: g["n"] == 60 and (g["weight"] == np.float32(1.5)).all(), profile=True)
    # ---- characters, not masks: 0 and 16 are both '.'
    body = [A] * 10
    m0, m16 = mem(range(10), body[:5] + [0] + body[6:]), mem(range(10), body[:5] + [16] + body[6:])
    add("masks-0-then-16", [m0, m16, mem(range(10), G)],
        lambda g, c: g["n"] == 20 and list(g["mask"][g["pos"] == 5]) == [0, G], profile=True)
    add("masks-16-then-0", [m16, m0, mem(range(10), G)],
        lambda g, c: g["n"] == 20 and list(g["mask"][g["pos"] == 5]) == [16, G], profile=True)
    add("all-32-masks", [mem([0, 1, 2], [A, m, A]) for m in range(32)],
        lambda g, c: int((g["pos"] == 1).sum()) == 31 and g["weight"][1] == np.float32(0.5625) and g["mask"][1] == 0,
        profile=True)
    # ---- capacity and where steps 6-9 keep the rows' codes
    add("nodes-15000", [mem(range(5000), m) for m in (A, G, C)], lambda g, c: g["n"] == 15000 and g["n"] > FIRST_NCAP, big=True)
    add("one-member-4000-lds", [mem(range(4000), [(A, G)[i % 2] for i in range(4000)])],
        lambda g, c: 4 * g["n"] <= graph_bitmap_off(1) and 4 * (g["n"] + 500) > graph_bitmap_off(1), big=True)
    add("one-member-6000-global", [mem(range(6000), [(A, G)[i % 2] for i in range(6000)])],
        lambda g, c: 4 * g["n"] > graph_bitmap_off(1), big=True)
    # ---- allocation segments
    add("rows-256-one-segment", [mem(range(256)), mem([253, 255])],
        lambda g, c: g["n"] == 256 and g["n"] <= slot_segment(g["n"]) and not spilled(c, 1, 253) and c.words(1)["store"][253] == 0,
        profile=True)
    add("rows-257-two-segments", [mem(range(257)), mem([254, 256])],
        lambda g, c: g["n"] == 257 and slot_segment(g["n"]) == 256 and spilled(c, 8, 254), profile=True)
    # ---- a width that is no multiple of the bitmap's 32-bit words, its first and last column occupied
    add("width-4001", [mem([0, 31, 32, 4000]), mem([31, 4000], G)],
        lambda g, c: c.width % 32 == 1 and list(np.unique(g["pos"])) == [0, 31, 32, 4000], width=4001, profile=True)
    return cs


CASES = _cases()
# A family without a single base: no DAG to align against.  The entries refuse it before anything is launched.
NO_BASE_FAMILIES = [[mem([])], [mem([]), mem([]), mem([])]]


def by_width():
    """The cases grouped by store: [(width, [cases])]."""
    out = {}
    for c in CASES:
        out.setdefault(c.width, []).append(c)
    return sorted(out.items())
