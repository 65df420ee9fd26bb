"""Named inputs of the --show-dist tests, shared by tests/test_showdist_cpu.py (which asserts every case's predicate and
pins tests/showdist_ref.py and the host's show_dist_report on them) and tests/test_gpu_showdist.py (which runs them
through sina_hip_show_dist).

A case is a dict: width, refs (packed base lists, column | mask << 24), names (the store's: ref0, ref1, ...), and per
query orig (the input alignment), aligned (the finished one) and lists (the ids of its relatives); `why` is the predicate
that says what the case exists for, in plain numpy on the case and its expected rows.  Everything here is CPU work."""
import functools

import numpy as np

from tests import compare_cases as cc
from tests import compare_ref
from tests import showdist_ref as sr

WAVES = 4          # of a workgroup of show_dist_kernel: list position x goes to wave x % 4


def _world(width, n_refs, length, seed):
    """References around a common ancestor: shared columns, a tenth of the bases substituted, some dropped."""
    rng = np.random.default_rng(9100 + seed)
    length = min(length, width)
    base_cols = np.sort(rng.choice(width, size=length, replace=False))
    anc = rng.choice([1, 2, 4, 8], size=length)
    refs = []
    for _ in range(n_refs):
        keep = rng.random(length) > 0.08
        m = anc.copy()
        sub = rng.random(length) < 0.1
        m[sub] = rng.choice([1, 2, 4, 8], size=int(sub.sum()))
        refs.append(cc.seq(base_cols[keep], m[keep]))
    return refs, rng


def _variant(ab, width, rng, move=0.08, drop=0.0):
    """A finished alignment of the same sequence: some bases one column to the right where that column is free, some
    dropped."""
    pos, m = cc.cols(ab).copy(), cc.masks(ab).astype(np.uint32)
    for x in np.flatnonzero(rng.random(len(pos)) < move):
        nxt = pos[x + 1] if x + 1 < len(pos) else width
        if pos[x] + 1 < nxt:
            pos[x] += 1
    keep = rng.random(len(pos)) >= drop
    return (pos[keep].astype(np.uint32) | (m[keep] << 24)).astype(np.uint32)


def _case(width, refs, orig, aligned, lists, why):
    lists = [np.asarray(x, np.uint32) for x in lists]
    cc.check_wellformed(width, list(refs) + list(orig), aligned, lists)      # (every sequence: uint32, columns ascending, below the width)
    assert len(orig) == len(aligned) == len(lists) and all(len(x) == 0 or int(x.max()) < len(refs) for x in lists)
    return dict(width=width, refs=refs, names=sr.names_of(len(refs)), orig=orig, aligned=aligned, lists=lists, why=why)


def _queries(refs, picks, width, rng, **kw):
    orig = [_variant(refs[p], width, rng, move=0.05) for p in picks]
    return orig, [_variant(o, width, rng, **kw) for o in orig]


def _closest(rows):
    return [int(r[sr.CLOSEST]) for r in rows]


def _scores(case, q):
    return [float(sr.score(compare_ref.compare_ref(case["orig"][q], case["refs"][int(i)], 0, False))) for i in case["lists"][q]]


# ---------------------------------------------------------------- list lengths: one member per wave, then a wave's second

def list_sizes():
    refs, rng = _world(300, 48, 60, 1)
    sizes = [0, 1, 4, 5, 41]
    orig, aligned = _queries(refs, [3, 9, 17, 25, 40], 300, rng)
    lists = [np.arange(n) + 2 for n in sizes]

    def why(case, rows):
        assert [len(x) for x in case["lists"]] == [0, 1, WAVES, WAVES + 1, 41]
        assert rows[0][sr.CLOSEST] == sr.NONE and not rows[0][sr.BEFORE:sr.CLOSEST].any() and all(c != sr.NONE for c in _closest(rows)[1:])
    return _case(300, refs, orig, aligned, lists, why)


def winner_places():
    """The closest relative first and last in its list (and its wave's only member / its last)."""
    refs, rng = _world(300, 30, 60, 2)
    orig, aligned = _queries(refs, [5, 5, 12, 12], 300, rng)
    others5 = [i for i in range(20, 29)]
    others12 = [i for i in range(14, 24)]
    lists = [[5] + others5, others5 + [5], [12] + others12, others12 + [12]]

    def why(case, rows):
        for q, (ids, c) in enumerate(zip(case["lists"], _closest(rows))):
            s = _scores(case, q)
            assert sorted(s)[-1] > sorted(s)[-2]                     # no tie: the place alone must not matter
            assert c == (ids[0] if q % 2 == 0 else ids[-1]) and len(ids) > 2 * WAVES
    return _case(300, refs, orig, aligned, lists, why)


def ties():
    """Two members with the same best score whose name order is the reverse of their id order (ref10 < ref2 byte-wise):
    in one wave (list positions i and i + 4, both orders) and in different waves."""
    refs, rng = _world(300, 24, 60, 3)
    refs[10] = refs[2].copy()
    orig, aligned = _queries(refs, [2, 2, 2, 2], 300, rng)
    far = [15, 16, 17, 18, 19, 20]
    lists = [[far[0], 2, far[1], far[2], far[3], 10, far[4]],        # positions 1 and 5: wave 1 sees id 2 first
             [far[0], 10, far[1], far[2], far[3], 2, far[4]],        # ... id 10 first
             [far[0], 2, 10, far[1]],                                # waves 1 and 2
             [10, far[1], far[2], 2, far[3]]]                        # waves 0 and 3

    def why(case, rows):
        assert case["names"][10] < case["names"][2]                  # byte-wise: the greater id has the lesser name
        for q, ids in enumerate(case["lists"]):
            ids = [int(i) for i in ids]
            s = _scores(case, q)
            assert s[ids.index(2)] == s[ids.index(10)] == max(s) and sorted(s)[-3] < max(s)
            assert rows[q][sr.CLOSEST] == 2                          # the name decides, not the id and not the place
        pos = [[int(x) for x in np.flatnonzero((ids == 2) | (ids == 10))] for ids in case["lists"]]
        assert pos[0][1] - pos[0][0] == WAVES and pos[1][1] - pos[1][0] == WAVES
        assert all(a % WAVES != b % WAVES for a, b in pos[2:])
    return _case(300, refs, orig, aligned, lists, why)


def search_result():
    """A list that is a search result, not a family: ids in no order."""
    refs, rng = _world(300, 40, 60, 4)
    orig, aligned = _queries(refs, [7, 21], 300, rng)
    lists = [[31, 4, 22, 7, 39, 0, 18, 12, 35, 9], [3, 38, 21, 1, 30, 16]]

    def why(case, rows):
        for ids in case["lists"]:
            d = np.diff(ids.astype(np.int64))
            assert (d > 0).any() and (d < 0).any()
    return _case(300, refs, orig, aligned, lists, why)


def fewer_bases():
    """aligned has fewer bases than orig (the aligner dropped some)."""
    refs, rng = _world(300, 20, 60, 5)
    orig, aligned = _queries(refs, [4, 11, 15], 300, rng, drop=0.2)
    lists = [np.arange(12), np.arange(6, 20), np.arange(3, 8)]

    def why(case, rows):
        for o, a, r in zip(case["orig"], case["aligned"], rows):
            assert 0 < len(a) < len(o) and r[sr.SELF + 2] + r[sr.SELF + 0] > 0      # bases of orig that aligned lacks
    return _case(300, refs, orig, aligned, lists, why)


def rebuild():
    """The closest relative has bases in columns that orig occupies and aligned does not: after.only_b counts them only
    if the tables were rebuilt for aligned -- a bitmap that still held orig's bits would call them matches or
    mismatches."""
    width = 200
    cols = list(range(10, 170, 2))
    masks = [1, 2, 4, 8] * (len(cols) // 4)
    rel = cc.seq(cols, masks)
    orig = cc.seq(cols, masks)
    moved = list(range(30, 60, 2))                                   # aligned has these bases one column to the right
    aligned = cc.seq([c + 1 if c in moved else c for c in cols], masks)
    other = cc.seq(range(11, 171, 2), [8, 4, 2, 1] * 20)
    refs = [other, rel, other.copy()]

    def why(case, rows):
        o, a, w = (set(cc.cols(x).tolist()) for x in (case["orig"][0], case["aligned"][0], case["refs"][1]))
        gone = w & (o - a)
        assert len(gone) == 15 and rows[0][sr.CLOSEST] == 1
        assert rows[0][sr.AFTER + 3] == len(gone) and rows[0][sr.AFTER + 2] == len(gone)   # only_b, and only_a beside them
        assert rows[0][sr.BEFORE + 4] == len(o) and rows[0][sr.BEFORE + 3] == 0
    return _case(width, refs, [orig], [aligned], [[0, 1, 2]], why)


def _width_case(width):
    def build():
        refs, rng = _world(width, 12, 48, 100 + width)
        # the first and the last column occupied on both sides of some pair
        edge = cc.seq([0, width // 2, width - 1], [1, 2, 4])
        refs[0] = edge
        orig, aligned = _queries(refs, [0, 3, 8], width, rng, drop=0.05)
        orig[0], aligned[0] = edge.copy(), cc.seq([0, width - 1], [1, 4])
        lists = [[0, 1, 2], np.arange(12), [8, 3, 5, 0, 11]]

        def why(case, rows):
            assert case["width"] == width and (width + 31) // 32 == {33: 2, 64: 2, 8224: 257, 50000: 1563}[width]
            assert max(int(cc.cols(r)[-1]) for r in case["refs"] if len(r)) == width - 1
            assert rows[0][sr.CLOSEST] == 0 and rows[0][sr.BEFORE + 4] == 3 and rows[0][sr.AFTER + 4] == 2
        return _case(width, refs, orig, aligned, lists, why)
    return build


def iupac_lower():
    """An orig with lower-case and ambiguous bases: EXACT (self) and OPTIMISTIC (the relatives) disagree on them, and
    neither filters lower case."""
    refs, rng = _world(300, 16, 60, 6)
    o = refs[5].copy()
    m = cc.masks(o).astype(np.uint32)
    m[::5] = 15                                                     # N
    m[1::7] |= 4 | 1                                                # two-base codes
    m[2::3] |= cc.LC                                                # lower case, kept
    o = (cc.cols(o).astype(np.uint32) | (m << 24)).astype(np.uint32)
    a = _variant(refs[5], 300, rng)                                 # the unambiguous bases, moved a little
    lists = [np.arange(16)]

    def why(case, rows):
        o, a = case["orig"][0], case["aligned"][0]
        exact, opt = compare_ref.compare_ref(o, a, 2, False), compare_ref.compare_ref(o, a, 0, False)
        assert exact[4] < opt[4] and tuple(rows[0][sr.SELF:sr.SELF + 6]) == exact
        assert (cc.masks(o) & cc.LC).any() and compare_ref.compare_ref(o, a, 2, True) != exact     # the filter would differ
        w = case["refs"][int(rows[0][sr.CLOSEST])]
        assert tuple(rows[0][sr.BEFORE:sr.BEFORE + 6]) != compare_ref.compare_ref(o, w, 2, False)
    return _case(300, refs, [o], [a], lists, why)


def nq_1():
    refs, rng = _world(120, 9, 40, 7)
    orig, aligned = _queries(refs, [4], 120, rng)

    def why(case, rows):
        assert len(case["orig"]) == 1 and len(rows) == 1
    return _case(120, refs, orig, aligned, [np.arange(9)], why)


def nq_600():
    """600 one-member queries: more workgroups than the device has compute units."""
    refs, rng = _world(64, 8, 24, 8)
    picks = [q % 8 for q in range(600)]
    orig, aligned = _queries(refs, picks, 64, rng)
    lists = [[(q * 3) % 8] for q in range(600)]

    def why(case, rows):
        assert len(case["orig"]) == 600 > 256 and all(len(x) == 1 for x in case["lists"])
        assert len({tuple(r) for r in rows}) > 50
    return _case(64, refs, orig, aligned, lists, why)


def no_score():
    """Rows whose floats are NaN and rows that come back flagged: an aligned without a base (self and after all zero,
    the host's floats from them NaN, the row not flagged: every member has a score); a member without a base (flagged,
    the others still compete); an orig without a base (every member left out: flagged, no closest)."""
    refs, rng = _world(300, 10, 60, 9)
    refs[6] = np.zeros(0, np.uint32)
    orig, aligned = _queries(refs, [2, 3, 4], 300, rng)
    aligned[0] = np.zeros(0, np.uint32)
    orig[2] = np.zeros(0, np.uint32)
    lists = [[0, 1, 2, 3], [5, 6, 7, 3], [1, 2]]

    def why(case, rows):
        assert not rows[0][sr.SELF:sr.SELF + 6].any() and not rows[0][sr.AFTER:sr.AFTER + 6].any()
        assert rows[0][sr.FLAGS] == sr.FLAG_COMPUTED and rows[0][sr.CLOSEST] != sr.NONE and rows[0][sr.BEFORE + 4] > 0
        rep = sr.report(rows[0], 4)
        assert np.isnan(rep["sps"]) and np.isnan(rep["cpm"]) and not np.isnan(rep["idty"])
        assert rows[1][sr.FLAGS] == sr.FLAG_COMPUTED | sr.FLAG_NAN and rows[1][sr.CLOSEST] == 3
        assert rows[2][sr.FLAGS] == sr.FLAG_COMPUTED | sr.FLAG_NAN and rows[2][sr.CLOSEST] == sr.NONE
    return _case(300, refs, orig, aligned, lists, why)


CASES = dict(list_sizes=list_sizes, winner_places=winner_places, ties=ties, search_result=search_result, fewer_bases=fewer_bases,
             rebuild=rebuild, iupac_lower=iupac_lower, nq_1=nq_1, nq_600=nq_600, no_score=no_score)
for _w in (33, 64, 8224, 50000):
    CASES["width_%d" % _w] = _width_case(_w)
NAMES = sorted(CASES)
FUZZ_SEEDS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """uint32 [nq, 20] by tests/showdist_ref.py, computed once per process and shared (read only)."""
    out = sr.rows(case(name))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fuzz(seed):
    """A world of compare_cases.fuzz_case as a show-dist case: its queries are the input alignments, the finished ones
    are made from them, its candidate lists (0 to 40 ids, an id may repeat, an empty and an all-lower-case reference
    among them) are the relatives."""
    width, refs, qs, cand = cc.fuzz_case(seed)
    rng = np.random.default_rng(9900 + seed)
    aligned = [_variant(q, width, rng, move=0.1, drop=0.05) for q in qs]
    c = _case(width, refs, list(qs), aligned, cand, None)
    out = sr.rows(c)
    out.setflags(write=False)
    return c, out


def flat_call(c):
    """The arrays sina_hip_show_dist takes: orig_ab, orig_off, al_ab, al_off, ref_ids, ref_off."""
    return (cc.flat(c["orig"]), cc.offsets(c["orig"]), cc.flat(c["aligned"]), cc.offsets(c["aligned"]), cc.flat(c["lists"]),
            cc.offsets(c["lists"]))
