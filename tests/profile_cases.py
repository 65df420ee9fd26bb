"""Named families for the device profile build's tests (family_profile_kernel, sina_amd/csrc/profile_build.hip), shared
by tests/test_profile_cpu.py (which asserts that every case sits on the edge it names) and
tests/test_gpu_profile_edges.py (which runs them).  Everything here is CPU work on hand-built packed arrays (alignment
column | iupac mask << 24 per base).

A case is a small store of its own (its members), the alignment width, the SINA_HIP_TEST=profile_tile values to run it
under (None: the tile the host chooses) and a predicate over the plain build (tests/profile_ref.py) that says what the
case is there for; where an edge depends on the tile, the predicate is about the case's FIRST tile value.  The kernel's
numbers are restated here from its source: kPT = 512 threads, kTileMax = 6144 nodes per LDS tile, 4096 nodes of first
capacity, 256 bases per wave chunk (64 lanes, four loads each), 16-bit counters of 12 points per member.

In most cases member 0 is a "spine" with a real base in every column 0 .. n - 1, so that node == column and no column
is left to bases without a base bit; the other members carry the edge."""
import functools

import numpy as np

from sina_amd import synth
from tests import profile_ref as pr
from tests.graph_cases import A, C, G, U, mem

THREADS = 512          # kPT
TILE_MAX = 6144        # kTileMax
FIRST_NCAP = 4096      # build_family_profiles' first node capacity
CHUNK = 256            # bases of a member a wave takes at a time
LANES = 64
FAMILY_MAX = 128
LDS_BYTES, LDS_SLACK, MEMBER_BYTES = 160 * 1024, 256, 24
SMALL_TILES = (1, 2, 64, 511, 512, 513)
SCORES = (-1.7, 0.9, 3.3, 0.7)   # a scheme whose terms are not representable (test_gpu_profile_device.py)
LOWER = 16                        # the case bit: not a base bit


def host_tile(width, max_family, ncap, forced=None):
    """profile_build.hip, profile_lds: the nodes per LDS tile the host chooses."""
    nwords = (width + 31) // 32
    bm = (6 * nwords + 15) & ~15
    room = (LDS_BYTES - LDS_SLACK - bm - MEMBER_BYTES * max_family - 16) // 12
    tile = min(ncap, TILE_MAX, room)
    if forced:
        tile = min(tile, forced)
    return max(1, tile)


def grown_ncap(n):
    """build_family_profiles: the capacity the launch is repeated with for a family of n nodes that did not fit, and
    what a context keeps for its next call."""
    return min(65535, n + n // 8 + 16)


class Case:
    def __init__(self, name, members, edge, width=800, tiles=(64,), fam=None, fresh=False):
        self.name, self.members, self.edge, self.width = name, [np.asarray(m, np.uint32) for m in members], edge, int(width)
        self.fam = list(range(len(members))) if fam is None else list(fam)
        self.fresh = fresh       # on the real numbers: a context of its own, so that the first capacity is 4096
        self.tiles = tuple(tiles) if fresh else tuple(tiles) + tuple(t for t in SMALL_TILES + (None,) if t not in tiles)
        assert 1 <= len(self.fam) <= FAMILY_MAX
        assert all(len(m) == 0 or int((m & 0xFFFFFF).max()) < width for m in self.members)

    @property
    def tile(self):
        """The tile the edge is built for: the forced one, or the host's own after its capacity has grown."""
        n = self.build()["n"]
        ncap = FIRST_NCAP if n <= FIRST_NCAP else grown_ncap(n)
        return host_tile(self.width, len(self.fam), ncap, self.tiles[0])

    def family(self):
        return [self.members[i] for i in self.fam]

    @functools.lru_cache(maxsize=None)
    def build(self):
        return pr.build(self.family(), self.width)

    @functools.lru_cache(maxsize=None)
    def tables(self, scores=SCORES):
        return pr.table(self.build()["points"], *scores)

    @functools.lru_cache(maxsize=None)
    def words(self):
        return pr.chain_words(self.build()["pos"])

    def on_edge(self):
        return bool(self.edge(self.build(), self))

    def __repr__(self):
        return self.name


def widened(case, width):
    """The case in a wider store (the several-families launch puts cases of different widths into one)."""
    return Case(case.name, case.members, case.edge, width=width, tiles=case.tiles[:1], fam=case.fam, fresh=True)


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


def query_of(case, salt=0):
    """The first member that has a base -- its first 300 bases -- with a few substitutions, as upper-case iupac masks with a
    base bit (graph_cases.query_of); a family without a base gets a query of one base."""
    m = next((m for m in case.family() if len(m)), mem([0]))
    q = ((m >> 24) & 0x0F).astype(np.uint8)[:300]
    q[q == 0] = A
    for i in range(2 + salt, len(q), 7):
        q[i] = {A: G, G: C, C: U}.get(int(q[i]), A)
    return q


def finite(case):
    """No column whose only bases have no base bit (its shares would be 0 / 0) -- column 0 without any base is a column of
    gaps, and fine."""
    real, bitless = set(), set()
    for m in case.family():
        cols, bit = (m & 0xFFFFFF), ((m >> 24) & 0x0F) != 0
        real.update(cols[bit].tolist())
        bitless.update(cols[~bit].tolist())
    return bitless <= real


# ---------------------------------------------------------------- what the predicates read off a case
def nodes(b, member):
    """The node of every base of a member."""
    return np.searchsorted(b["pos"], member & 0xFFFFFF).astype(np.int64)


def real(member):
    return ((member >> 24) & 0x0F) != 0


def stretches(b, member):
    """(r, r1, i) for every base i of the member: its node and the node of its next base (n behind the last)."""
    r = nodes(b, member)
    return [(int(r[i]), int(r[i + 1]) if i + 1 < len(r) else b["n"], i) for i in range(len(r))]


def handovers(b, member, T):
    """Per tile boundary k * T the index of the member's last base in front of it (the kernel's cursor), -1: none yet."""
    r = nodes(b, member)
    return [int(np.searchsorted(r, n0)) - 1 for n0 in range(T, b["n"], T)]


def opened(b, node):
    return int(b["points"][node, 4]) // 12


def extended(b, node):
    return int(b["points"][node, 5]) // 12


def spine(n, lo=0):
    return mem(range(lo, n), [(A, G, C, U)[i % 4] for i in range(lo, n)])


def _cases():
    cs = []

    def add(*a, **kw):
        cs.append(Case(*a, **kw))

    T = 64
    # ---------------------------------------------------------------- the tile sweep
    # a last base on the tile's last node, its gap opening on the next tile's first node
    add("tile-open-on-next-tiles-first-node", [spine(200), mem([60, 61, 62, 63, 70, 71])],
        lambda b, c: (63, 70, 3) in stretches(b, c.members[1]) and 64 % c.tile == 0 and opened(b, 64) == 1 and extended(b, 65) == 1)
    # a stretch that opened in an earlier tile, clamped to the tile's first node
    add("tile-stretch-clamped-to-n0", [spine(200), mem([40, 41, 90, 91])],
        lambda b, c: (41, 90, 1) in stretches(b, c.members[1]) and 42 < c.tile < 89 and extended(b, c.tile) == 1 and opened(b, c.tile) == 0)
    add("tile-member-absent-from-a-whole-tile", [spine(260), mem([10, 11, 200, 201])],
        lambda b, c: any(r // c.tile + 2 <= r1 // c.tile for r, r1, _ in stretches(b, c.members[1])[:-1]))
    add("tile-member-ended-tiles-ago", [spine(300), mem(range(5, 30), G)],
        lambda b, c: nodes(b, c.members[1])[-1] // c.tile + 3 <= (b["n"] - 1) // c.tile)
    # cur stays 0 and the leading gap comes again through i == 0, clamped, in every tile
    add("tile-first-base-in-the-third-tile", [spine(260), mem(range(150, 170), C)],
        lambda b, c: nodes(b, c.members[1])[0] // c.tile == 2 and handovers(b, c.members[1], c.tile)[:2] == [-1, -1])
    add("tile-cursor-hand-over", [spine(330), mem(range(2, 330, 5), U), mem([3, 4, 5, 300])],
        lambda b, c: len(handovers(b, c.members[1], c.tile)) >= 4 and (np.diff(handovers(b, c.members[1], c.tile)) > 0).all() and
        handovers(b, c.members[2], c.tile) == [2] * 4 + [3])
    # the whole wave past the tile with two or more chunks still to go
    add("tile-beyond-exit-two-chunks-left", [spine(900), mem(range(0, 900, 1), G)],
        lambda b, c: c.tile <= 64 and len(c.members[1]) >= 3 * CHUNK + c.tile and nodes(b, c.members[1])[CHUNK] >= c.tile, width=1100)
    for name, n in (("tile-n-equals-t", T), ("tile-n-equals-t-plus-1", T + 1), ("tile-n-equals-2t", 2 * T)):
        add(name, [spine(n), mem(range(1, n, 3), C), mem([0, n - 1])],
            lambda b, c, k={T: (1, 0), T + 1: (1, 1), 2 * T: (2, 0)}[n]: divmod(b["n"], c.tile) == k)
    for name, n in (("tile-n-equals-512", 512), ("tile-n-equals-513", 513), ("tile-n-equals-1024", 1024)):
        add(name, [spine(n), mem(range(1, n, 3), C), mem([0, n - 1])],
            lambda b, c, k={512: (1, 0), 513: (1, 1), 1024: (2, 0)}[n]: divmod(b["n"], c.tile) == k, width=1100, tiles=(512,))
    # the tile's prefix sum: fewer nodes than threads (chunk 1, idle threads), 512 and 513 nodes (chunk 1 -> 2)
    add("tile-fewer-nodes-than-threads", [spine(100), mem(range(0, 100, 9), G), mem([50])],
        lambda b, c: b["n"] < THREADS and c.tile == 64 and extended(b, 99) == 1, tiles=(64, 100, 300))
    gappy = [mem([c for c in range(600) if c % 11 < 4], G), mem([c for c in range(600) if c % 13 > 9], U), mem([7, 511, 512, 590])]
    add("tile-of-512-nodes", [spine(600)] + gappy, lambda b, c: c.tile == THREADS and b["n"] > THREADS, tiles=(512,))
    add("tile-of-513-nodes", [spine(600)] + gappy, lambda b, c: c.tile == THREADS + 1 and b["n"] > c.tile, tiles=(513,))

    # as many members as the workgroup has waves: a member each, all at once
    # (dense, the spine's bases with short gaps: a query of the spine's aligns along the whole profile)
    add("members-8-one-per-wave", [spine(150)] + [spine(150)[[(c + 3 * j) % (11 + j) >= 2 for c in range(150)]] for j in range(7)],
        lambda b, c: len(c.fam) == THREADS // LANES and all(100 < len(m) <= 150 for m in c.members) and
        sum(opened(b, n) for n in range(b["n"])) > 50)

    # ---------------------------------------------------------------- bases without a base bit (0 and the lower-case 16)
    def bitless_at(b, c, base, **want):
        m = c.members[1]
        return not real(m)[base] and all({"opened": opened, "extended": extended}[k](b, node) == v
                                         for k, (node, v) in want.items())

    # the member's first base: nothing to walk back through, the leading gap goes on
    add("bitless-first-base", [spine(100), mem([20, 30, 31], [0, G, G])],
        lambda b, c: bitless_at(b, c, 0, extended=(21, 1), opened=(21, 0)))
    # a run of them behind a real base: the gap behind the run opens
    add("bitless-run-behind-a-base", [spine(100), mem([10, 11, 12, 13, 30], [G, 0, LOWER, 0, G])],
        lambda b, c: bitless_at(b, c, 3, opened=(14, 1), extended=(15, 1)))
    # ... behind a gap: it extends (a single one, and a run whose first is the one that sees the gap)
    add("bitless-behind-a-gap", [spine(100), mem([10, 20, 40], [G, 0, G])],
        lambda b, c: bitless_at(b, c, 1, opened=(11, 1), extended=(21, 1)) and opened(b, 21) == 0)
    add("bitless-run-behind-a-gap", [spine(100), mem([10, 20, 21, 22, 40], [G, 0, 0, LOWER, G])],
        lambda b, c: bitless_at(b, c, 3, opened=(11, 1), extended=(23, 1)) and opened(b, 23) == 0)
    add("bitless-leading-run", [spine(100), mem([5, 6, 40], [LOWER, 0, G])],
        lambda b, c: bitless_at(b, c, 1, extended=(7, 1)) and opened(b, 7) == 0 and extended(b, 4) == 1)
    add("bitless-behind-a-base", [spine(100), mem([10, 11, 40], [G, 0, G])],
        lambda b, c: bitless_at(b, c, 1, opened=(12, 1), extended=(13, 1)))
    # the walk back reads bases in front of the tile's cursor: the run straddles the boundary, the real base is two back
    add("bitless-walk-back-across-a-tile", [spine(200), mem([61, 62, 63, 64, 80], [U, G, 0, 0, G])],
        lambda b, c: bitless_at(b, c, 3, opened=(65, 1)) and c.tile == 64 and handovers(b, c.members[1], 64)[0] == 2)
    add("bitless-walk-back-across-a-tile-in-a-gap", [spine(200), mem([30, 62, 63, 64, 80], [U, 0, 0, 0, G])],
        lambda b, c: bitless_at(b, c, 3, extended=(65, 1)) and opened(b, 65) == 0 and c.tile == 64)
    add("bitless-last-base", [spine(100), mem([10, 11, 50], [G, G, 0]), mem([10, 40, 50], [C, 0, LOWER]), mem([49, 50], [G, 0])],
        lambda b, c: bitless_at(b, c, 2, opened=(12, 1)) and extended(b, 51) == 2 and opened(b, 51) == 1 and extended(b, 99) == 3)
    add("bitless-column-0", [spine(100), mem([0, 1, 9], [0, 0, G]), mem([0, 9], [LOWER, C])],
        lambda b, c: bitless_at(b, c, 0) and extended(b, 1) == 1 and extended(b, 2) == 2 and opened(b, 1) == 0 and opened(b, 2) == 0)

    # ---------------------------------------------------------------- column ranks
    nw = lambda c: (c.width + 31) // 32  # noqa: E731
    add("rank-one-word", [mem([0, 3, 19], [A, G, C]), mem([3, 7], U)], lambda b, c: nw(c) == 1 and c.width % 32 and b["n"] == 4,
        width=20, tiles=(2,))
    add("rank-width-4001", [mem([0, 31, 32, 4000]), mem([31, 4000], G)],
        lambda b, c: c.width % 32 == 1 and list(b["pos"]) == [0, 31, 32, 4000], width=4001, tiles=(2,))
    for words in (512, 513):   # (the rank pass's chunk 1 -> 2)
        w = 32 * words
        cols = list(range(0, w, 97)) + [w - 1]
        add("rank-%d-words" % words, [mem(cols, [(A, G, C, U)[i % 4] for i in range(len(cols))]), mem(cols[3::5], U)],
            lambda b, c, words=words: nw(c) == words and b["pos"][-1] // 32 == words - 1 and b["n"] > 100, width=w)
    add("rank-bit-0-and-bit-31", [mem([0, 31, 32, 63, 64, 95, 100], G), mem([32, 63, 100], C)],
        lambda b, c: {32, 63, 64, 95} <= set(b["pos"].tolist()), tiles=(2,))
    add("rank-last-column-occupied", [mem([5, 700, 799], C), mem([799], C)], lambda b, c: b["pos"][-1] == c.width - 1, tiles=(2,))
    add("rank-column-0-occupied", [mem([0, 4, 5], U), mem([4, 9], C)], lambda b, c: b["pos"][0] == 0 and extended(b, 0) == 1, tiles=(2,))
    add("rank-column-0-empty", [mem([3, 4, 5], U), mem([4, 9], C)],
        lambda b, c: b["pos"][0] == 0 and extended(b, 0) == 2 and b["points"][0].sum() == 24, tiles=(2,))

    # ---------------------------------------------------------------- the packed 16-bit counters
    add("count-128-same-base", [mem([3, 4, 5], [A, G, U]) for _ in range(128)],
        lambda b, c: b["points"][1, 0] == 1536 and b["points"][2, 1] == 1536 and b["points"][3, 3] == 1536, tiles=(2,))
    add("count-orders-2-3-4", [mem([0, 1, 2, 3, 4], [A, A | G, A | G | C, 15, C | U]), mem([5, 6], [G | C | U, A | U])],
        lambda b, c: [list(b["points"][k, :4]) for k in (1, 2, 3)] == [[6, 6, 0, 0], [4, 4, 4, 0], [3, 3, 3, 3]], tiles=(2,))
    # (a node needs a base: of 128 members one holds the column, so 127 gaps open there at the most)
    add("count-127-gaps-open", [mem([0, 1, 2, 3, 4])] + [mem([0, 1, 4], G) for _ in range(127)],
        lambda b, c: opened(b, 2) == 127 and extended(b, 3) == 127, tiles=(2,))
    add("count-128-gaps-extend", [mem([1 + j % 4, 6], C) for j in range(128)],
        lambda b, c: extended(b, 0) == 128 and extended(b, 1) == 96 and extended(b, 4) == 64 and opened(b, 4) == 32, tiles=(2,))
    # (the leading gaps of all 128 end on node 1: the -1 of the difference array 128 times)
    add("count-128-stretches-end-on-one-node", [mem([5, 6, 9], U) for _ in range(128)],
        lambda b, c: extended(b, 0) == 128 and extended(b, 1) == 0 and b["points"][1, 3] == 1536, tiles=(2,))

    # ---------------------------------------------------------------- member lengths against the 64 lanes and the 256-base chunk
    for k in (0, 1, 63, 64, 65, 255, 256, 257, 513):   # (every base with a gap behind it: the look-ahead bases[i + 1] matters)
        add("length-%d" % k, [spine(2 * k + 3), mem(range(1, 2 * k + 1, 2), U)],
            lambda b, c, k=k: len(c.members[1]) == k and all(opened(b, n) == 1 for n in range(2, 2 * k + 2, 2)), width=1100)

    # ---------------------------------------------------------------- the chain the DP kernel is handed
    add("chain-one-node", [mem([]), mem([])], lambda b, c: b["n"] == 1 and extended(b, 0) == 2 and c.words()["rec"][0, 2] ==
        pr.gr.REC_SINK | pr.gr.REC_DIST_FAR << pr.gr.REC_DIST_SHIFT, tiles=(1,))
    add("chain-one-node-a-base", [mem([0], C)], lambda b, c: b["n"] == 1 and b["points"][0, 2] == 12, tiles=(1,))
    add("chain-two-nodes", [mem([17], C)], lambda b, c: b["n"] == 2 and len(c.words()["pred"]) == 1 and
        list(c.words()["succ_min"]) == [17, pr.NO_SUCCESSOR], tiles=(1,))
    add("same-reference-twice", [mem(range(3, 90, 2), [(A, C)[i % 2] for i in range(44)])],
        lambda b, c: c.fam == [0, 0] and b["points"][1, 0] == 24 and extended(b, 0) == 2, fam=[0, 0])

    # ---------------------------------------------------------------- the host loop, on the real numbers (a fresh context each)
    def real_family(n):
        marks = sorted(c for c in {9, TILE_MAX - 1, TILE_MAX + 4, n - 1} if c < n)   # (a base on the full tile's last node)
        return [spine(n), mem([c for c in range(n) if c % 7 < 3], G), mem(marks, C)]

    for n, launches, tile, tiles in ((4096, 1, 4096, (1, 0)), (4097, 2, 4625, (0, 4097)), (6144, 2, TILE_MAX, (1, 0)),
                                     (6145, 2, TILE_MAX, (1, 1)), (12288, 2, TILE_MAX, (2, 0)), (12289, 2, TILE_MAX, (2, 1))):
        add("host-%d-nodes" % n, real_family(n), lambda b, c, n=n, launches=launches, tile=tile, tiles=tiles: b["n"] == n and
            (n > FIRST_NCAP) == (launches == 2) and c.tile == tile and divmod(n, c.tile) == tiles, width=12800, tiles=(None,),
            fresh=True)
    return cs


CASES = _cases()
EDGES = [c.name for c in CASES]


def by_width(fresh=False):
    """The cases that share a context, grouped by store: [(width, [cases])]."""
    out = {}
    for c in CASES:
        if c.fresh == fresh:
            out.setdefault(c.width, []).append(c)
    return sorted(out.items())


# ---------------------------------------------------------------- the seeded fuzz generator
def fuzz_case(seed):
    """1 to 128 members over a random set of columns, every member present in runs with long absences between them, codes
    of every order including none; a random tile of 1 to 700 nodes.  Finite by construction: after the draw, every column
    whose bases are all without a base bit has its first base given one -- one pass, nothing is drawn again."""
    rng = np.random.default_rng(77000 + seed)
    F = int(rng.choice([1, 2, 3, 8, 40, 128, int(rng.integers(1, 129))]))
    width = int(rng.choice([700, 3000, 20000]))
    ncols = int(rng.integers(1, min(width, 1500) + 1))
    universe = np.sort(rng.choice(width, size=ncols, replace=False))
    codes = np.array(list(range(16)) + [0, 0, LOWER, LOWER | A, A, G, C, U], np.uint32)
    members = []
    for _ in range(F):
        keep = np.zeros(ncols, bool)
        at, here = 0, bool(rng.integers(0, 2))
        while at < ncols:   # runs of presence and of absence; one run in six is long
            run = int(rng.integers(1, 400)) if rng.integers(0, 6) == 0 else int(rng.integers(1, 12))
            keep[at:at + run] = here
            at, here = at + run, not here
        if rng.integers(0, 12) == 0:
            keep[:] = False
        cols = universe[keep]
        members.append(cols.astype(np.uint32) | (rng.choice(codes, size=len(cols)) << np.uint32(24)))
    has_bit = set()
    for m in members:
        has_bit.update((m & 0xFFFFFF)[real(m)].tolist())
    for m in members:   # (in family order: the first base of a column without a base bit gets one)
        for i in np.flatnonzero(~real(m)):
            if int(m[i] & 0xFFFFFF) not in has_bit:
                has_bit.add(int(m[i] & 0xFFFFFF))
                m[i] |= np.uint32((A, G, C, U, A | G, 15)[i % 6] << 24)
    tile = int(rng.integers(1, 701))
    return Case("fuzz-%d" % seed, members, lambda b, c: True, width=width, tiles=(tile, None), fresh=True)
