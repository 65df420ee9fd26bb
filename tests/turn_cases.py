"""The inputs of the orientation tests, shared by tests/test_turn_cpu.py (which pins tests/turn_ref.py to the oracle and
asserts every case's predicate) and tests/test_gpu_turn.py (which runs them through sina_hip_kmer_topk_turn).  Hand-built
posting lists in the way of tests/kmer_cases.py (its helpers, unchanged), so scores are designed and not hoped for.

The worlds.  k = 6; the index holds lists for the k-mers of a PALETTE only, chosen so that the reverse, the complement
and the reverse complement of a palette k-mer are never palette k-mers: a k-mer scores in the one orientation it was
written for.  A SEGMENT seg(kmers, o) is "N, then each k-mer followed by an N", turned by o: a query made of segments
shows, read in orientation o, exactly the k-mers of its segments written for o, whatever stands around them.  Families
F_0 .. F_11 of eight k-mers each have score rows over sixty references of their own (index_for_scores: reference r is in
the family's first row[r] lists, one reference in all eight), and four background k-mers BG_0 .. BG_3, one per
orientation, are each in 200 references that lie with 200 different threads of tile 0 of the count kernel: a query that
carries all four background segments has, in every orientation, a candidate-list threshold of 1 and at most a few
hundred candidates, so on the candidate path nothing overflows unless the case means it to.

A case: a world, the queries of one call, and its runs -- all four orientations or two, `max`, SINA_HIP_TEST knobs --
with a predicate `why(case)` that asserts the edge it exists for from turn_ref's results.  Everything here is CPU work."""
import functools

import numpy as np

from tests import kmer_cases as kc
from tests import kmer_ref
from tests import turn_ref as tr

K = 6
N = kc.N_MASK
SMALL, BIG = 5000, 70000                          # score rows / candidate lists (65 536 references and more)
LENGTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)
MAXES = (1, 41, 128, 129)
ALL30 = tuple(range(1, 16)) + tuple(range(17, 32))
# IUPAC codes by mask: bits A = 1, G = 2, C = 4, T = 8
IUPAC = {"A": 1, "G": 2, "C": 4, "T": 8, "R": 3, "Y": 12, "K": 10, "M": 5, "S": 6, "W": 9, "B": 14, "V": 7, "D": 11, "H": 13, "N": 15}
COMPLEMENT = {"A": "T", "G": "C", "R": "Y", "K": "M", "B": "V", "D": "H", "S": "S", "W": "W", "N": "N"}


# ---------------------------------------------------------------- k-mers and segments

def kmer_image(v, o, k=K):
    """The value of k-mer v read in orientation o (base codes A G C T = 0 1 2 3: the complement of code c is 3 - c)."""
    d = [(v >> (2 * (k - 1 - i))) & 3 for i in range(k)]
    if o & 1:
        d = d[::-1]
    if o & 2:
        d = [3 - c for c in d]
    out = 0
    for c in d:
        out = (out << 2) | c
    return out


def seg(kmers, o=0):
    return tr.variant(np.concatenate([[N], kc.query_of([int(v) for v in kmers], K)]).astype(np.uint8), o)


def cat(*parts):
    return np.concatenate([np.asarray(p, np.uint8) for p in parts]) if parts else np.zeros(0, np.uint8)


@functools.lru_cache(maxsize=None)
def palette(a_only):
    """108 k-mers none of whose images under o = 1, 2, 3 is one of them (a_only: all of them start with A)."""
    rng = np.random.default_rng(9100 + int(a_only))
    taken, images, out = set(), set(), []
    for v in rng.permutation(1 << (2 * (K - 1)) if a_only else 1 << (2 * K)).tolist():
        im = {kmer_image(v, o) for o in (1, 2, 3)}
        if v in im or v in images or im & taken:
            continue
        taken.add(v)
        images |= im
        out.append(v)
        if len(out) == 108:
            break
    assert len(out) == 108 and not (taken & images)
    return tuple(out)


class World:
    def __init__(self, n_refs, nofast=True):
        self.n_refs, self.k, self.nofast = n_refs, K, nofast
        rng = np.random.default_rng(9200 + n_refs // 1000 + int(nofast))
        pal = palette(not nofast)
        self.bg = pal[:4]
        self.fam = [pal[4 + 8 * j:12 + 8 * j] for j in range(12)]
        self.spare = pal[100:]
        lists = {}
        bg_ids = np.arange(5, min(n_refs, kc.TILE), kc.THREAD_REFS)[:200]
        assert len(bg_ids) >= 150
        for v in self.bg:
            lists[v] = bg_ids.astype(np.uint32)
        free = rng.permutation(np.flatnonzero(np.arange(n_refs) % kc.THREAD_REFS != 5))
        self.rows = []
        for j, fam in enumerate(self.fam):                   # (sixty references of its own: no reference is in two families)
            row = np.zeros(n_refs, np.int64)
            at = free[60 * j:60 * j + 60]
            row[at] = rng.integers(1, 8, size=60)
            row[at[0]] = 8                                   # one reference holds the whole family
            lists.update(kc.index_for_scores(row, list(fam)))
            self.rows.append(row)
        self.off, self.ids = kc.build_csr(lists, K)

    def ref_store(self):
        return np.full(self.n_refs, 1 << 24, np.uint32), np.arange(self.n_refs + 1, dtype=np.uint64), 8

    def background(self):
        """The four background segments: every orientation of a query that carries them scores 1 on 200 references."""
        return cat(*[seg([self.bg[o]], o) for o in range(4)])

    def scores(self, qmask):
        return kmer_ref.scores(self.off, self.ids, self.n_refs, qmask, K, not self.nofast)


@functools.lru_cache(maxsize=None)
def world(n_refs, nofast=True):
    return World(n_refs, nofast)


class Case:
    def __init__(self, name, w, qmasks, runs, why, labels=None):
        self.name, self.world, self.why = name, w, why
        self.qmasks = [np.ascontiguousarray(m, np.uint8) for m in qmasks]
        self.runs = runs                                     # dicts: all (bool), mx, knobs ({} or SINA_HIP_TEST keys)
        self.labels = list(labels) if labels else ["q%d" % i for i in range(len(self.qmasks))]
        assert all(len(m) <= kc.LONG_MAX for m in self.qmasks)

    @property
    def qmask(self):
        return cat(*self.qmasks)

    @property
    def qoff(self):
        off = np.zeros(len(self.qmasks) + 1, np.uint64)
        off[1:] = np.cumsum([len(m) for m in self.qmasks])
        return off

    @functools.cached_property
    def rows(self):
        """Per query the score row of each of its four orientations: kmer_ref's, computed once."""
        w = self.world
        return [tr.rows_of(w.off, w.ids, w.n_refs, m, K, not w.nofast) for m in self.qmasks]

    @functools.lru_cache(maxsize=None)
    def expected(self, all_four, mx):
        """Per query turn_ref's dict(turn, top1, ids, scores), over the shared rows."""
        return [tr.orient(rows, all_four, mx) for rows in self.rows]

    def n_long(self):
        return sum(len(m) > kc.FAST_MAX for m in self.qmasks)

    def pick_launches(self, knobs):
        """Launch ranges of one call, none of which is cut further: whole queries, the long ones in ranges of their own."""
        per = int(knobs.get("turn_range", 0)) or len(self.qmasks)
        n_long = self.n_long()
        return -(-(len(self.qmasks) - n_long) // per) + -(-n_long // per)

    def cand_overflows(self, all_four, mx, knobs):
        """Does any orientation tried overflow its candidate list (and where: (query, variant) pairs)?"""
        if not (mx <= kc.CAND_MAX_M and self.world.n_refs >= 2 * kc.TILE and not knobs.get("kmer_rows")):
            return None
        return [(qi, x) for qi, rows in enumerate(self.rows) for x, o in enumerate(tr.ORDER[bool(all_four)])
                if len(self.qmasks[qi]) <= kc.FAST_MAX and kc.cand_model(rows[o], mx)["overflow"]]


def _runs(maxes=MAXES, alls=(True, False), knobs=({},)):
    return [dict(all=a, mx=m, knobs=dict(kn)) for kn in knobs for a in alls for m in maxes]


def _truth(w, fam, n_kmers, t, extra=()):
    """A query whose orientation t shows the first n_kmers k-mers of family fam, with the background in every orientation."""
    return cat(seg(w.fam[fam][:n_kmers], t), w.background(), *extra)


# ---------------------------------------------------------------- lengths and alignment

@functools.lru_cache(maxsize=None)
def lengths():
    """Every length of LENGTHS starting at every byte offset mod 4 of the concatenation (fillers of 0 to 3 bases between
    them; a filler of no bases is a query too).  Lengths below k: all four scores 0, the pick 0."""
    w = world(SMALL)
    rng = np.random.default_rng(9301)
    qs, labels, at, x = [], [], 0, 0
    for L in LENGTHS:
        for r in range(4):
            fill = (r - at) % 4
            qs.append(rng.choice([1, 2, 4, 8], size=fill).astype(np.uint8))
            labels.append("fill_%d" % fill)
            at += fill
            if L < K + 1:
                q = rng.choice([1, 2, 4, 8], size=L).astype(np.uint8)
            else:
                t, fam = x % 4, x % 12
                x += 1
                q = tr.variant(kc.pad_n(seg(w.fam[fam][:(L - 1) // (K + 1)]), L), t)
            assert at % 4 == r and len(q) == L
            qs.append(q)
            labels.append("len_%d_at_%d" % (L, r))
            at += L

    def why(c):
        off = c.qoff.astype(np.int64)
        seen = {(len(m), int(off[i]) % 4) for i, m in enumerate(c.qmasks)}
        assert {(L, r) for L in LENGTHS for r in range(4)} <= seen
        e = c.expected(True, 1)
        assert {x["turn"] for x in e} == {0, 1, 2, 3}
        for m, x in zip(c.qmasks, e):
            if len(m) < K + 1:
                assert (x["top1"] == 0).all() and x["turn"] == 0
            else:
                assert x["top1"].max() >= 8 and (np.sort(x["top1"])[:3] == 0).all()
    return Case("lengths", w, qs, _runs((1, 41)), why, labels)


# ---------------------------------------------------------------- alphabet

@functools.lru_cache(maxsize=None)
def alphabet():
    """One query holding all 30 non-gap mask values between two runs of k-mers, handed in complemented."""
    w = world(SMALL)
    truth = cat(seg(w.fam[0]), ALL30, seg(w.fam[1][:3]))
    q = tr.variant(truth, 2)

    def why(c):
        m = c.qmasks[0]
        assert set(ALL30) <= set(m.tolist()) and len(set(ALL30)) == 30
        for a, b in COMPLEMENT.items():
            for case_bit in (0, 16):
                assert tr.complement([IUPAC[a] | case_bit])[0] == IUPAC[b] | case_bit
                assert tr.complement([IUPAC[b] | case_bit])[0] == IUPAC[a] | case_bit
        amb = lambda v: np.flatnonzero(np.isin(np.asarray(v) & 15, [1, 2, 4, 8], invert=True))   # noqa: E731
        assert (amb(tr.variant(m, 1)) == (len(m) - 1 - amb(m))[::-1]).all()         # windows break at the mirrored place
        assert (amb(tr.variant(m, 2)) == amb(m)).all()
        fwd = kmer_ref.window_values(truth, K, False).tolist()
        rev = kmer_ref.window_values(tr.variant(truth, 1), K, False).tolist()
        assert fwd == list(w.fam[0]) + list(w.fam[1][:3]) and rev == [kmer_image(v, 1) for v in fwd[::-1]]
        e = c.expected(True, 41)[0]
        assert e["turn"] == 2 and e["top1"][2] == 8 and (e["top1"][[0, 1, 3]] == 0).all()
        assert c.expected(False, 41)[0]["turn"] == 0
    return Case("alphabet", w, [q], _runs((1, 41)), why)


# ---------------------------------------------------------------- winners and ties

def _winner_queries(w):
    qs = [_truth(w, t, 8, t) for t in range(4)]
    labels = ["truth_%d" % t for t in range(4)]
    # truth "reversed", and two k-mers of another family for "reversed and complemented": with two orientations tried the
    # scores of 1 and 2 are 0 and the pick is from {0, 3}
    qs.append(_truth(w, 4, 8, 1, [seg(w.fam[5][:2], 3)]))
    labels.append("rev_only")
    a = _truth(w, 6, 8, 0)
    qs.append(cat(a, tr.variant(a, 3)))
    labels.append("palindrome")
    qs.append(cat(seg(w.fam[7][:4], 1), seg(w.fam[8][:4], 2), w.background()))
    labels.append("tie_1_2")
    qs.append(cat(*[seg(w.fam[8 + o][:3], o) for o in range(4)], w.background()))
    labels.append("tie_all")
    return qs, labels


def _why_winners(c):
    e = {lb: x for lb, x in zip(c.labels, c.expected(True, 41))}
    e2 = {lb: x for lb, x in zip(c.labels, c.expected(False, 41))}
    for t in range(4):
        x = e["truth_%d" % t]
        assert x["turn"] == t and x["top1"][t] == 8 and (np.delete(x["top1"], t) == 1).all()
    x, y = e["rev_only"], e2["rev_only"]
    assert x["turn"] == 1 and x["top1"].tolist() == [1, 8, 1, 2]
    assert y["turn"] == 3 and y["top1"].tolist() == [1, 0, 0, 2]
    assert e2["truth_1"]["turn"] == 0 and e2["truth_2"]["turn"] == 0 and e2["truth_3"]["turn"] == 3
    m = c.qmasks[c.labels.index("palindrome")]
    x = e["palindrome"]
    assert (tr.variant(m, 3) == m).all() and x["top1"][0] == x["top1"][3] == 8 and x["turn"] == 0 and x["top1"][1] < 8
    x = e["tie_1_2"]
    assert x["top1"].tolist() == [1, 4, 4, 1] and x["turn"] == 1
    x = e["tie_all"]
    assert x["top1"].tolist() == [3, 3, 3, 3] and x["turn"] == 0


@functools.lru_cache(maxsize=None)
def winners(n_refs):
    """A winner at each of 0, 1, 2, 3; "reversed" under two orientations tried; a reverse palindrome; ties.  Below 65 536
    references on score rows; at 70 000 on candidate lists (no list overflows: every query carries the background), with
    the score rows forced, and cut into ranges of two queries."""
    w = world(n_refs)
    qs, labels = _winner_queries(w)
    knobs = ({},) if n_refs < 2 * kc.TILE else ({}, {"kmer_rows": 1}, {"turn_range": 2})

    def why(c):
        _why_winners(c)
        for r in c.runs:
            over = c.cand_overflows(r["all"], r["mx"], r["knobs"])
            assert over is None or over == []
            assert (over is not None) == (n_refs == BIG and r["mx"] <= 128 and not r["knobs"].get("kmer_rows"))
    return Case("winners_%d" % n_refs, w, qs, _runs(knobs=knobs), why, labels)


@functools.lru_cache(maxsize=None)
def nothing():
    """A store that holds none of the query's k-mers in any orientation; and a query shorter than k."""
    w = world(SMALL)
    qs = [seg(w.spare[:5]), kc.kmer_mask(w.fam[0][0], K)[:4], _truth(w, 2, 8, 3)]

    def why(c):
        e = c.expected(True, 41)
        assert all(c.world.off[v + 1] == c.world.off[v] for v in w.spare)
        for x in e[:2]:
            assert (x["top1"] == 0).all() and x["turn"] == 0 and len(x["ids"]) == 41 and x["ids"][0] == SMALL - 1
        assert e[2]["turn"] == 3
    return Case("nothing", w, qs, _runs((1, 41)), why)


@functools.lru_cache(maxsize=None)
def overflow_late():
    """70 000 references, the candidate path.  Query 1 carries the background for orientation 0 only: its first variant's
    list holds, the others' score rows are all zero -- a giant group of equal scores -- and their lists overflow.  The
    range is repeated on score rows, in sub-ranges that keep a query's variants together."""
    w = world(BIG)
    qs = [_truth(w, 0, 8, 3), cat(seg(w.fam[1], 0), seg([w.bg[0]], 0)), _truth(w, 2, 8, 1), _truth(w, 3, 8, 2)]

    def why(c):
        for r in c.runs:
            over = c.cand_overflows(r["all"], r["mx"], r["knobs"])
            assert over and all(qi == 1 and x >= 1 for qi, x in over), over
        e = c.expected(True, 41)
        assert [x["turn"] for x in e] == [3, 0, 1, 2] and e[1]["top1"].tolist() == [8, 0, 0, 0]
    return Case("overflow_late", w, qs, _runs((1, 41, 128), knobs=({}, {"turn_range": 3})), why)


# ---------------------------------------------------------------- fast index

@functools.lru_cache(maxsize=None)
def fast_index():
    """A fast index (only k-mers that start with A count): the query's own k-mer count differs by orientation."""
    w = world(SMALL, nofast=False)
    qs = [_truth(w, t, 8, t) for t in range(4)]

    def why(c):
        for t, (m, x) in enumerate(zip(c.qmasks, c.expected(True, 41))):
            counts = [len(kmer_ref.window_values(tr.variant(m, o), K, True)) for o in range(4)]
            assert len(set(counts)) > 1 and counts[t] >= 9 and x["turn"] == t and x["top1"][t] == 8
        assert all(v < 1 << (2 * (K - 1)) for v in palette(True))
    return Case("fast_index", w, qs, _runs((1, 41)), why)


# ---------------------------------------------------------------- the big select, a long query, ranges

@functools.lru_cache(maxsize=None)
def big_select():
    """max = 4097 on 5000 references: the big select ranks every variant's row."""
    w = world(SMALL)
    qs = [_truth(w, 0, 8, 2), _truth(w, 1, 8, 3)]

    def why(c):
        assert 4097 > kc.SEL_MAX and [x["turn"] for x in c.expected(True, 4097)] == [2, 3]
        assert all(len(x["ids"]) == 4097 for x in c.expected(True, 4097))
    return Case("big_select", w, qs, _runs((4097,), alls=(True,)), why)


@functools.lru_cache(maxsize=None)
def long_query():
    """One query of 10 241 bases among short ones: the long count kernel, put last, rows back in the caller's order."""
    w = world(SMALL)
    long_q = tr.variant(kc.pad_n(cat(np.tile(seg(w.fam[5]), 20), seg(w.fam[6][:4])), kc.FAST_MAX + 1), 3)
    qs = [_truth(w, 0, 8, 1), long_q, _truth(w, 1, 8, 2)]

    def why(c):
        assert [len(m) > kc.FAST_MAX for m in c.qmasks] == [False, True, False] and len(long_q) == 10241 and c.n_long() == 1
        e = c.expected(True, 41)
        assert [x["turn"] for x in e] == [1, 3, 2] and e[1]["top1"][3] == 160
        assert c.pick_launches({}) == 2
    return Case("long_query", w, qs, _runs((1, 41)), why)


@functools.lru_cache(maxsize=None)
def ranges():
    """Seven queries in launch ranges of 1, 2 and 3 whole queries; queries 2 and 5 are byte-identical."""
    w = world(SMALL)
    qs = [_truth(w, j, 8, (3 * j + 1) % 4) for j in range(7)]
    qs[5] = qs[2].copy()

    def why(c):
        assert len(c.qmasks) == 7 and (c.qmasks[2] == c.qmasks[5]).all()
        assert [c.pick_launches(r["knobs"]) for r in c.runs[::2]] == [7, 4, 3, 1]
        e = c.expected(True, 41)
        assert [x["turn"] for x in e] == [1, 0, 3, 2, 1, 3, 3]
        assert (e[2]["ids"] == e[5]["ids"]).all()
    return Case("ranges", w, qs, _runs((41,), knobs=({"turn_range": 1}, {"turn_range": 2}, {"turn_range": 3}, {})), why)


@functools.lru_cache(maxsize=None)
def one_query():
    w = world(SMALL)

    def why(c):
        assert len(c.qmasks) == 1 and c.expected(True, 41)[0]["turn"] == 3 and c.expected(False, 1)[0]["turn"] == 3
    return Case("one_query", w, [_truth(w, 9, 8, 3)], _runs((1, 41)), why)


CASES = {"lengths": lengths, "alphabet": alphabet, "winners_small": functools.partial(winners, SMALL),
         "winners_big": functools.partial(winners, BIG), "nothing": nothing, "overflow_late": overflow_late,
         "fast_index": fast_index, "big_select": big_select, "long_query": long_query, "ranges": ranges,
         "one_query": one_query}
NAMES = tuple(CASES)


def case(name):
    return CASES[name]()


# ---------------------------------------------------------------- fuzz

FUZZ_SEEDS = 6


@functools.lru_cache(maxsize=None)
def fuzz(seed):
    """A seeded call on one of the worlds (the ORDER of the draws is part of it): 3 to 9 queries, each a shuffle of
    segments in random orientations, sometimes cut at a random place or byte-reversed whole; random `max`, two or four
    orientations, sometimes ranges of one or two queries."""
    rng = np.random.default_rng(9500 + seed)
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]  # noqa: E731
    w = world(*pick([(SMALL, True), (SMALL, False), (BIG, True)]))
    qs = []
    for _ in range(int(rng.integers(3, 10))):
        parts = [seg(w.fam[int(rng.integers(0, 12))][:int(rng.integers(1, 9))], int(rng.integers(0, 4))) for _ in range(int(rng.integers(1, 6)))]
        if rng.random() < 0.8:
            parts.append(w.background())
        q = cat(*[parts[i] for i in rng.permutation(len(parts))])
        if rng.random() < 0.3:
            q = q[int(rng.integers(0, 4)):len(q) - int(rng.integers(0, 9))]
        qs.append(q)
    runs = [dict(all=bool(rng.integers(0, 2)), mx=int(pick([1, 2, 41, 128, 129, 400])), knobs=pick([{}, {}, {"turn_range": 1}, {"turn_range": 2}]))
            for _ in range(2)]
    return Case("fuzz_%d" % seed, w, qs, runs, lambda c: None)
