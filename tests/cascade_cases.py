"""Named hand-built candidate lists for the family cascade (sina_amd/csrc/family.hip): the smallest shapes on which a
wave that takes 64 candidates per step, keeps its counters in scalar registers and leaves early can go wrong.  Shared
by tests/test_cascade_cpu.py (every predicate, and the plain loop against the oracle) and tests/test_gpu_cascade.py
(every case through sina_hip_family_cascade).

All cases are lists over ONE small store (store()): references of a few bases whose size, first and last column are
what the cascade reads.  A case is Case(rule, ids, scores, match or None, query_bases, selfs or None); every builder
asserts its edge before anything is compared.  CPU work only."""
import collections
import functools

import numpy as np

from tests import cascade_ref as cr

Case = collections.namedtuple("Case", "rule ids scores match query_bases selfs")
WIDTH = 64
FULL_LEN, MIN_LEN = 16, 4
# kinds of reference: (how many, bases, first column)
KINDS = collections.OrderedDict(N=(300, 8, 5), F=(20, 16, 3), L=(20, 8, 0), FL=(10, 16, 0), S=(10, 2, 7), E=(5, 0, 0))


@functools.lru_cache(maxsize=None)
def store():
    """(width, packed base lists, {kind: ids}): N normal, F full length, L left end (first column 0), FL both, S shorter
    than fs_min_len, E without bases."""
    refs, ids = [], {}
    for kind, (count, size, first) in KINDS.items():
        ids[kind] = np.arange(len(refs), len(refs) + count, dtype=np.uint32)
        for i in range(count):
            cols = first + np.arange(size, dtype=np.uint32) * (2 if i % 2 else 1)      # (two last columns per kind)
            refs.append((cols | (np.uint32(1 << (i % 4)) << np.uint32(24))).astype(np.uint32))
    meta = cr.meta_of(refs)
    assert (meta[ids["N"], 1] > 0).all() and (meta[ids["L"], 1] == 0).all() and (meta[ids["FL"], 1] == 0).all()
    assert (meta[ids["F"], 0] >= FULL_LEN).all() and (meta[ids["N"], 0] < FULL_LEN).all() and (meta[ids["S"], 0] < MIN_LEN).all()
    assert (meta[ids["E"]] == 0).all() and meta[:, 2].max() < WIDTH
    return WIDTH, refs, ids


def meta():
    return cr.meta_of(store()[1])


def rule(**kw):
    base = dict(fs_min=5, fs_max=5, fs_req_full=0, fs_full_len=FULL_LEN, fs_min_len=MIN_LEN, fs_cover_gene=0, fs_msc=0.7, fs_msc_max=2.0)
    base.update(kw)
    return cr.Rule(**base)


def mk(r, ids, scores=None, match=None, query_bases=10, selfs=None):
    ids = np.asarray(ids, np.uint32)
    if scores is None:
        scores = 500 - np.arange(len(ids))                                              # descending, none below any fs_msc used
    scores = np.asarray(scores, np.float32)
    assert len(scores) == len(ids) and (np.diff(scores) <= 0).all()
    if match is not None:
        match = np.asarray(match, np.uint16)
        assert len(match) == len(ids)
    if selfs is not None:
        selfs = np.asarray(selfs, np.uint32)
    return Case(r, ids, scores, match, query_bases, selfs)


def run(c, early_exit=False):
    """The plain pass over a case."""
    return cr.cascade(cr.candidates(meta(), c.ids, c.scores, c.match, c.query_bases, c.selfs), c.rule, early_exit)


def scanned(c, step=64):
    """Candidates a kernel that checks `saturated` before every step of 64 covers."""
    cands = cr.candidates(meta(), c.ids, c.scores, c.match, c.query_bases, c.selfs)
    total = 0
    for base in range(0, len(cands), step):
        p = cr.cascade(cands[:base], c.rule)
        if cr.saturated(c.rule, p.have, p.have_full, p.have_left, p.have_right):
            break
        total += min(step, len(cands) - base)
    return total


def _N(n, start=0):
    return store()[2]["N"][start:start + n]


# ---------------------------------------------------------------- list lengths and steps

def _length(n):
    def build():
        c = mk(rule(fs_min=130, fs_max=130), _N(n))
        p = run(c)
        assert p.kept == list(range(n)) and not p.enough and cr.bound(c.rule) == 130
        return c
    return build


# ---------------------------------------------------------------- quotas across the 64-lane step

def _min_at(m):
    """fs_min reached by candidate m - 1; then the middle phase: scores below fs_msc from rank 70 on, until fs_max."""
    def build():
        c = mk(rule(fs_min=m, fs_max=m + 3, fs_msc=50.5), _N(100), scores=120 - np.arange(100))
        p = run(c)
        assert (c.scores[:70] > 50.5).all() and (c.scores[70:] < 50.5).all()
        assert p.kept == list(range(m)) + [70, 71, 72] and p.enough
        return c
    return build


def _max_at(m):
    def build():
        c = mk(rule(fs_min=m, fs_max=m), _N(100))
        p = run(c)
        assert p.kept == list(range(m)) and p.enough
        return c
    return build


def _bulk(fs_min):
    """Every other candidate of the first step is too short: 32 eligible lanes, the last of them lane 63.  The bulk
    step ends in the middle of the step (20) or with its last eligible lane (32); two more are kept behind it."""
    def build():
        s = store()[2]
        ids = np.empty(80, np.uint32)
        ids[0::2] = s["S"][np.arange(40) % len(s["S"])]
        ids[1::2] = _N(40)
        c = mk(rule(fs_min=fs_min, fs_max=fs_min + 2, fs_msc=1000.0), ids)
        p = run(c)
        assert p.kept == [2 * i + 1 for i in range(fs_min + 2)] and (p.kept[fs_min - 1] == 63) == (fs_min == 32)
        return c
    return build


# ---------------------------------------------------------------- option extremes

def min_above_max():
    c = mk(rule(fs_min=10, fs_max=4), _N(30))
    p = run(c)
    assert p.kept == list(range(10)) and p.enough and cr.bound(c.rule) == 10
    return c


def min_zero_good():
    c = mk(rule(fs_min=0, fs_max=5, fs_msc=1000.0), _N(30))
    assert run(c).kept == list(range(5))
    return c


def min_zero_bad():
    c = mk(rule(fs_min=0, fs_max=5), _N(30))
    p = run(c)
    assert p.kept == [] and not p.enough
    return c


def max_zero():
    c = mk(rule(fs_min=3, fs_max=0), _N(30))
    p = run(c)
    assert p.kept == [0, 1, 2] and p.enough
    return c


def all_zero():
    c = mk(rule(fs_min=0, fs_max=0), _N(3))
    p = run(c)
    assert p.kept == [] and p.enough and cr.bound(c.rule) == 0
    return c


# ---------------------------------------------------------------- full-length quota

def full_behind_max():
    """fs_req_full = 2, the only full-length candidates behind the point where fs_max is reached: the family exceeds
    fs_max -- and has exactly K entries."""
    s = store()[2]
    c = mk(rule(fs_req_full=2), np.concatenate([_N(10), s["F"][:3], _N(5, 10)]))
    p = run(c)
    assert p.kept == [0, 1, 2, 3, 4, 10, 11] and p.enough and p.have == cr.bound(c.rule) == 7 > c.rule.fs_max
    return c


def no_full():
    c = mk(rule(fs_req_full=1), _N(20))
    p = run(c)
    assert p.kept == list(range(5)) and not p.enough
    return c


# ---------------------------------------------------------------- range cover and size 0

def _cover(cover):
    def build():
        s = store()[2]
        ids = np.concatenate([_N(6), s["L"][:1], _N(1, 6), s["L"][1:3], _N(1, 7)])
        c = mk(rule(fs_min=3, fs_max=3, fs_cover_gene=cover), ids)
        p = run(c)
        assert p.kept == [0, 1, 2] + [6, 8][:cover] and p.enough and p.have_left == cover
        assert p.have_right == (len(p.kept) if cover else 0)
        return c
    return build


def size_zero():
    """A reference without bases under fs_min_len = 0: counted in have, neither left nor right."""
    s = store()[2]
    ids = np.concatenate([s["E"][:2], _N(3), s["L"][:1]])
    c = mk(rule(fs_min=3, fs_max=3, fs_min_len=0, fs_cover_gene=1), ids)
    p = run(c)
    assert p.kept == [0, 1, 2, 5] and p.have_right == 2 and p.have_left == 1 and p.enough
    return c


# ---------------------------------------------------------------- score threshold

def msc_5_6():
    c = mk(rule(fs_min=2, fs_max=6, fs_msc=5.5), _N(10), scores=[9, 8, 6, 6, 5, 5, 5, 5, 5, 5])
    p = run(c)
    assert p.kept == [0, 1, 4, 5, 6, 7] and p.enough
    return c


def msc_zero():
    c = mk(rule(fs_min=1, fs_max=4), _N(8), scores=[3, 2, 1, 0, 0, 0, 0, 0])
    p = run(c)
    assert p.kept == [0, 3, 4, 5] and p.enough
    return c


# ---------------------------------------------------------------- identity

def identity_limit():
    """|query| = 10, match = 9, fs_msc_max = 0.9f: kept (`>` is strict); one match more: removed."""
    c = mk(rule(fs_min=3, fs_max=3, fs_msc_max=0.9), _N(6), match=[10, 9, 10, 9, 10, 0], query_bases=10)
    assert cr.identity(9, 10) == np.float32(0.9) and cr.identity(10, 10) > np.float32(0.9)
    p = run(c)
    assert p.kept == [1, 3, 5] and p.enough
    return c


def _no_limit(msc_max):
    def build():
        c = mk(rule(fs_msc_max=msc_max), _N(8))
        assert c.match is None and run(c).kept == list(range(5))
        return c
    return build


def no_bases():
    c = mk(rule(fs_min=3, fs_max=3, fs_msc_max=0.5), _N(5), match=[0] * 5, query_bases=0)
    assert run(c).kept == [0, 1, 2]
    return c


# ---------------------------------------------------------------- self list

def _self(selfs, gone):
    def build():
        ids = _N(70)
        c = mk(rule(fs_min=70, fs_max=70), ids, selfs=[int(ids[x]) if x >= 0 else 299 for x in selfs])
        p = run(c)
        assert p.kept == [x for x in range(70) if x not in gone] and len(c.selfs) == len(selfs)
        return c
    return build


# ---------------------------------------------------------------- early exit

def early_exit():
    """Behind the saturation point: candidates that pass every stateless test and have a good score.  Leaving early
    does not change the row, and the steps cover fewer candidates than the list holds."""
    s = store()[2]
    ids = np.concatenate([s["F"][:1], _N(4), _N(150, 4), s["F"][1:20], _N(26, 154)])
    c = mk(rule(fs_req_full=1, fs_msc=1000.0), ids)
    p, e = run(c), run(c, early_exit=True)
    assert len(ids) == 200 and p.kept == e.kept == [0, 1, 2, 3, 4] and e.stop == 5 and p.stop == 200
    assert (c.scores < 1000).all() and scanned(c) == 64 < len(ids)
    return c


CASES = collections.OrderedDict()
for _n in (0, 1, 63, 64, 65, 128, 129):
    CASES["len_%d" % _n] = _length(_n)
for _m in (63, 64, 65):
    CASES["min_at_%d" % _m] = _min_at(_m)
    CASES["max_at_%d" % _m] = _max_at(_m)
CASES.update(bulk_mid=_bulk(20), bulk_end=_bulk(32), min_above_max=min_above_max, min_zero_good=min_zero_good,
             min_zero_bad=min_zero_bad, max_zero=max_zero, all_zero=all_zero, full_behind_max=full_behind_max, no_full=no_full,
             cover_0=_cover(0), cover_1=_cover(1), cover_2=_cover(2), size_zero=size_zero, msc_5_6=msc_5_6, msc_zero=msc_zero,
             identity_limit=identity_limit, msc_max_1=_no_limit(1.0), msc_max_2=_no_limit(2.0), no_bases=no_bases,
             self_empty=_self([], []), self_rank0=_self([0], [0]), self_lanes_63_64=_self([63, 64], [63, 64]),
             self_absent=_self([-1], []), early_exit=early_exit)
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    n_refs = len(store()[1])
    assert len(c.ids) == 0 or int(c.ids.max()) < n_refs
    assert cr.bound(c.rule) <= cr.MAX_K
    return c


def expected(name):
    c = case(name)
    return cr.row(meta(), c.ids, c.scores, c.match, c.query_bases, c.selfs, c.rule)


def groups():
    """The cases by rule: those of one rule can share a call.  {rule: [names]}"""
    g = collections.OrderedDict()
    for name in NAMES:
        g.setdefault(case(name).rule, []).append(name)
    return g
