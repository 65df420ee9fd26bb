"""Hand-built (query, reference) pairs for the containment kernel (sina_hip_find_bases), each with a predicate that says
which edge it sits on: tests/test_contain_cpu.py runs the predicates over tests/contain_ref.py's answers, the GPU tests
compare the kernel's words with the same answers.

A case: dict(refs=[mask bytes], queries=[mask bytes], lists=[reference ids per query], why=predicate(case, want)) --
`want` the flat answers (contain_ref.expected).  Needles are written over the letters A and C, the text around a planted
needle over G and U, so that the planted places are the only hits and the filter's key still meets its first letters
often in the near misses."""
import functools

import numpy as np

from tests import contain_ref as cr

A, G, C, U, N, R_ = 1, 2, 4, 8, 15, 3  # (R_: the ambiguity code A|G)
LOWER = 0x10
NEEDLE_LENGTHS = (1, 7, 8, 9, 63, 64, 65, 128, 129)


def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (1 << 32))


def needle(rng, n):
    return rng.choice(np.array([A, C], np.uint8), size=n)


def text(rng, n):
    return rng.choice(np.array([G, U], np.uint8), size=n)


def plant(ref, nd, *starts):
    ref = ref.copy()
    for s in starts:
        assert 0 <= s and s + len(nd) <= len(ref)
        ref[s:s + len(nd)] = nd
    return ref


def changed(nd, at):
    """The needle with the base at index `at` swapped for the needle alphabet's other letter."""
    out = nd.copy()
    out[at] = A if out[at] == C else C
    return out


def _answers(case, want):
    """want, cut per query."""
    out, at = [], 0
    for ids in case["lists"]:
        out.append(want[at:at + len(ids)])
        at += len(ids)
    return out


# ---------------------------------------------------------------- the cases

def _needle_lengths(n):
    """A needle of n bases against references of n, n + 1, 63, 64, 65, 127, 128, 129 and 1500 bases: the hit at R - n
    where the needle fits (alone: at 0), no hit where it does not (n > R)."""
    rng = _rng("needle_lengths_%d" % n)
    nd = needle(rng, n)
    lens = [n, n + 1, 63, 64, 65, 127, 128, 129, 1500 + n % 7]
    refs = [plant(text(rng, R), nd, R - n) if R >= n else text(rng, R) for R in lens]

    def why(case, want):
        got = _answers(case, want)[0]
        assert [int(x) for x in got] == [R - n if R >= n else cr.NONE for R in lens]
        assert got[0] == 0 and got[1] == 1                          # R == n, R == n + 1
        assert (cr.NONE in got) == (n > 63)
    return dict(refs=refs, queries=[nd], lists=[np.arange(len(refs))], why=why)


def _placement():
    """Hits at 0, at R - n, starting at 63 and at 64 (the edge of the first chunk of 64 starts), one that straddles the
    edge; two hits in one chunk and two in different chunks: the lower wins."""
    rng = _rng("placement")
    nd = needle(rng, 20)
    R = 200
    starts = [(0,), (R - 20,), (63,), (64,), (50,), (60,), (10, 40), (40, 10), (30, 100), (130, 70), (63, 64 + 20), (0, R - 20)]
    refs = [plant(text(rng, R), nd, *s) for s in starts]

    def why(case, want):
        assert [int(x) for x in want] == [min(s) for s in starts]
        assert 50 < 64 < 50 + 20 and 60 < 64 < 60 + 20              # the straddling ones
        assert 10 // 64 == 40 // 64 and 30 // 64 != 100 // 64 and 130 // 64 != 70 // 64
    return dict(refs=refs, queries=[nd], lists=[np.arange(len(refs))], why=why)


def _near_misses():
    """References that hold the needle but for one base -- its last, the one at index 8 (just behind the key), at index 63
    and at index 64 (the verify's lane wrap) --, alone (no hit) and in front of a real hit (the real hit's start)."""
    rng = _rng("near_misses")
    nd = needle(rng, 100)
    refs, want_at, diff_at = [], [], (99, 8, 63, 64, 0, 7)
    for d in diff_at:
        miss = changed(nd, d)
        refs.append(plant(text(rng, 400), miss, 20))
        want_at.append(cr.NONE)
        refs.append(plant(plant(text(rng, 400), miss, 20), nd, 170))
        want_at.append(170)
        refs.append(plant(plant(text(rng, 400), nd, 250), miss, 101))     # (in another chunk than the hit)
        want_at.append(250)
    short = needle(rng, 9)                                                 # index 8 is the last base: one verify step
    refs.append(plant(plant(text(rng, 130), changed(short, 8), 3), short, 70))

    def why(case, want):
        per = _answers(case, want)
        assert [int(x) for x in per[0]] == want_at
        assert [int(x) for x in per[1]] == [70]
        for d in diff_at:
            assert (changed(nd, d) != nd).sum() == 1 and changed(nd, d)[d] != nd[d]
    return dict(refs=refs, queries=[nd, short], lists=[np.arange(len(refs) - 1), np.array([len(refs) - 1])], why=why)


def _periodic():
    """A homopolymer reference: a homopolymer needle hits at 0; the same needle but for its last base has no hit and
    every start is a candidate that fails in its last verify step -- the kernel's worst case."""
    ref = np.full(1500, A, np.uint8)
    two = np.tile(np.array([A, C], np.uint8), 750)
    queries = []
    for n in (7, 8, 9, 64, 65, 100, 129, 750, 1499, 1500):
        queries.append(np.full(n, A, np.uint8))
        last = np.full(n, A, np.uint8)
        last[-1] = C
        queries.append(last)

    def why(case, want):
        per = _answers(case, want)
        for x, q in enumerate(case["queries"]):
            if (q == A).all():
                assert per[x][0] == 0
            else:
                assert per[x][0] == cr.NONE and (q[:-1] == A).all() and q[-1] == C    # every start a candidate
            assert per[x][1] == cr.NONE     # (the period-two text ACAC...: neither two As in a row nor A...AC of 7 and more)
    return dict(refs=[ref, two], queries=queries, lists=[np.array([0, 1])] * len(queries), why=why)


def _lengths_and_masks():
    """n > R; n == R equal and differing; lower-case bits on either side still match; T and U are one code; N does not
    match A; equal ambiguity codes match, different ones do not."""
    rng = _rng("lengths_and_masks")
    nd = needle(rng, 40)
    amb = nd.copy()
    amb[[5, 20]] = [N, R_]
    refs = [
        nd[:39].copy(),                                   # 0: n > R
        nd.copy(),                                        # 1: n == R, equal
        changed(nd, 17),                                  # 2: n == R, differing
        plant(text(rng, 90), nd, 30) | LOWER,             # 3: the reference in lower case
        plant(text(rng, 90), nd, 30),                     # 4
        plant(text(rng, 90), amb, 11),                    # 5: holds the needle with N and R in it
        np.array([U, U, A, N, U], np.uint8),              # 6
    ]
    lower_q = nd | LOWER
    mixed_q = nd.copy()
    mixed_q[::3] |= LOWER
    queries = [nd, lower_q, mixed_q, amb, np.array([A], np.uint8), np.array([N], np.uint8), np.array([U | LOWER], np.uint8),
               np.array([R_], np.uint8)]
    lists = [np.array([0, 1, 2, 3, 4, 5]), np.array([1, 3, 4]), np.array([1, 3, 4]), np.array([5, 4, 1]), np.array([6]),
             np.array([6, 1]), np.array([6]), np.array([6, 5])]

    def why(case, want):
        per = [[int(x) for x in p] for p in _answers(case, want)]
        assert per[0] == [cr.NONE, 0, cr.NONE, 30, 30, cr.NONE]    # (5: A or C where the reference has N or R: not equal)
        assert per[1] == [0, 30, 30] and per[2] == [0, 30, 30]
        assert per[3] == [11, cr.NONE, cr.NONE]                     # N and R match themselves only
        assert per[4] == [2]                                        # A is the A at 2, not the N behind it
        assert per[5] == [3, cr.NONE]                               # N matches the N, not an A
        assert per[6] == [0]                                        # u is U (and T: the same code)
        assert per[7] == [cr.NONE, 11 + 20]
        assert cr.is_query_itself(per[0][1], 40, 40) and not cr.is_query_itself(per[0][3], 40, 90)
    return dict(refs=refs, queries=queries, lists=lists, why=why)


def _pair_layout():
    """One query against many references; many queries against one reference; an empty candidate list between two full
    ones; (the GPU test also addresses queries 1 .. of these arrays as a sub-range)."""
    rng = _rng("pair_layout")
    nd = needle(rng, 30)
    refs = [plant(text(rng, 100 + 3 * i), nd, 2 * i) if i % 3 else text(rng, 100 + 3 * i) for i in range(41)]
    host = text(rng, 1000)
    many = [needle(rng, 10 + i) for i in range(25)]
    for i, q in enumerate(many):
        if i % 4:
            host = plant(host, q, 40 * i)
    refs.append(host)
    queries = [nd] + many[:12] + [needle(rng, 5)] + many[12:]
    lists = [np.arange(41)] + [np.array([41])] * 12 + [np.array([], np.int64)] + [np.array([41, 0])] * 13

    def why(case, want):
        per = [[int(x) for x in p] for p in _answers(case, want)]
        assert per[0] == [2 * i if i % 3 else cr.NONE for i in range(41)]
        assert per[13] == [] and len(per[12]) == 1 and len(per[14]) == 2
        got = [p[0] for p in per[1:13]] + [p[0] for p in per[14:]]
        assert got == [40 * i if i % 4 else cr.NONE for i in range(25)]
        assert len(want) == 41 + 12 + 26
    return dict(refs=refs, queries=queries, lists=lists, why=why)


_BUILDERS = {"needle_%d" % n: functools.partial(_needle_lengths, n) for n in NEEDLE_LENGTHS}
_BUILDERS.update(placement=_placement, near_misses=_near_misses, periodic=_periodic, lengths_and_masks=_lengths_and_masks,
                 pair_layout=_pair_layout)
NAMES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILDERS[name]()
    c["refs"] = [np.asarray(r, np.uint8) for r in c["refs"]]
    c["queries"] = [np.asarray(q, np.uint8) for q in c["queries"]]
    c["lists"] = [np.asarray(x, np.uint32) for x in c["lists"]]
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    want = cr.expected(c["queries"], c["refs"], c["lists"])
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def merged(names=None):
    """Every named case in ONE world: the references one after the other, the lists' ids moved accordingly.  Gives the
    case and, per name, the slice of the flat answers that is its own."""
    refs, queries, lists, own, at = [], [], [], {}, 0
    for name in (names or tuple(NAMES)):
        c = case(name)
        lists += [x + np.uint32(len(refs)) for x in c["lists"]]
        queries += c["queries"]
        refs += c["refs"]
        n = sum(len(x) for x in c["lists"])
        own[name] = slice(at, at + n)
        at += n
    return dict(refs=refs, queries=queries, lists=lists), own


FUZZ_SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def fuzz(seed):
    """A few hundred pairs of 1 .. 300 bases over a two-letter alphabet -- hits and near misses are frequent --, a share
    of the needles cut from their reference, some of those with one base changed."""
    rng = np.random.default_rng(7000 + seed)
    refs = [rng.choice(np.array([A, C], np.uint8), size=int(rng.integers(1, 301))) for _ in range(60)]
    queries, lists = [], []
    for _ in range(90):
        ids = rng.integers(0, len(refs), size=int(rng.integers(0, 7)))
        kind = int(rng.integers(0, 4))
        if kind == 0 or len(ids) == 0:
            q = rng.choice(np.array([A, C], np.uint8), size=int(rng.integers(1, 301 if kind == 0 else 12)))
        else:
            src = refs[int(ids[0])]
            n = int(rng.integers(1, len(src) + 1))
            s = int(rng.integers(0, len(src) - n + 1))
            q = src[s:s + n].copy()
            if kind == 2:
                q = changed(q, int(rng.integers(0, n)))
            if kind == 3:
                q |= rng.choice(np.array([0, LOWER], np.uint8), size=n)
        queries.append(q)
        lists.append(ids.astype(np.uint32))
    c = dict(refs=refs, queries=queries, lists=lists)
    return c, cr.expected(queries, refs, lists)


# ---------------------------------------------------------------- a case as the calls take it

def packed(mask):
    """A reference's packed words: base i in column i."""
    m = np.asarray(mask, np.uint8)
    return np.arange(len(m), dtype=np.uint32) | (m.astype(np.uint32) << 24)


def width_of(c):
    return max(max(len(r) for r in c["refs"]), 8)


def flat_refs(c):
    off = np.zeros(len(c["refs"]) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in c["refs"]])
    return np.concatenate([packed(r) for r in c["refs"]]), off


def flat_call(c):
    """qmask, q_off, cand_ids, cand_off of sina_hip_find_bases."""
    q_off = np.zeros(len(c["queries"]) + 1, np.uint64)
    q_off[1:] = np.cumsum([len(q) for q in c["queries"]])
    c_off = np.zeros(len(c["lists"]) + 1, np.uint64)
    c_off[1:] = np.cumsum([len(x) for x in c["lists"]])
    ids = np.concatenate([np.asarray(x, np.uint32) for x in c["lists"]] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return np.concatenate(c["queries"]).astype(np.uint8), q_off, ids, c_off
