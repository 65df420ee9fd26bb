"""The inputs of the big-select tests: score rows built to order, as in tests/kmer_cases.py (whose helpers these cases
are made of), for searches that want more than 4096 candidates per query -- kmer_select_big_kernel, the segmented sort
behind it and the launch ranges of csrc/kmer_plan.h.  tests/test_kmer_big_cpu.py builds every case (which runs the
builders' own assertions on the edge a case exists for) and tests/test_gpu_kmer_big.py runs them on the device.  The
restatements here (big_queries, ranges_model, launches_model and kmer_cases.shortcut_model) decide reachability and
counter values only: every expected result comes from tests/kmer_ref.py.

Also here: the world of the stage-level escalation test (tests/test_gpu_escalation.py) and the plain statement of which
of its queries famfinder cannot satisfy from their first 410 or 4100 candidates.  Everything in this file is CPU work."""
import copy
import functools

import numpy as np

from sina_amd import synth
from tests import kmer_cases as kc
from tests import kmer_ref

SEL_MAX = kc.SEL_MAX
BIG_BUDGET = 1 << 30              # kBigSelBudget (csrc/kmer_plan.h)
BIG_BYTES_PER_CAND = 24           # kBigSelBytesPerCand
SCORE_MATRIX_BYTES = 2 << 30      # the older bound on a launch range: its int16 score matrix


# ---------------------------------------------------------------- restatements (reachability, counters)

def is_big(n_refs, mx):
    """The big select runs iff M = min(max, n_refs) is above 4096."""
    return min(mx, n_refs) > SEL_MAX


def ranges_model(nq, M, budget=BIG_BUDGET):
    """big_select_range / big_select_ranges of csrc/kmer_plan.h: (queries per range, number of ranges)."""
    per = max(1, min(nq, budget // (BIG_BYTES_PER_CAND * max(M, 1))))
    return per, (nq + per - 1) // per if nq else 0


def launches_model(c, mx, budget=BIG_BUDGET):
    """By how much kmer_launches advances for one kmer_topk of the case's batch with score rows (max > 128): the fast
    queries and the long ones in ranges of their own, each cut by the score-matrix bound and, for a big select, by the
    byte budget."""
    M = min(mx, c.n_refs)
    n_long = sum(len(m) > kc.FAST_MAX for m in c.qmasks)
    n_fast = len(c.qmasks) - n_long
    per = max(1, SCORE_MATRIX_BYTES // (2 * max(c.n_refs, 1)))
    if is_big(c.n_refs, mx):
        per = min(per, ranges_model(len(c.qmasks), M, budget)[0])
    return sum((n + per - 1) // per for n in (n_fast, n_long) if n)


def big_queries(c, mx):
    """By how much sina_hip_big_select_queries advances for that call."""
    return len(c.qmasks) if is_big(c.n_refs, mx) else 0


def first_tie_taken(case, qi, mx):
    """(cut score, smallest id among the taken references that score the cut, how many references score the cut)."""
    ids, sc = case.expected[qi]["find"][mx]
    cut = sc[-1]
    return int(cut), int(ids[sc == cut].min()), int((case.expected[qi]["scores"] == int(cut)).sum())


# ---------------------------------------------------------------- the cases

@functools.lru_cache(maxsize=None)
def seam():
    """5000 references; max = 4096 is the last the LDS kernel sorts, 4097 the first of the big select; 4999, 5000 take
    all but one and all; 5001 and 100 000 are clipped to 5000.  Row 0 spreads, row 1 has a giant tie group (3000
    references of score 2) that every one of the max values cuts through or takes whole."""
    rng = np.random.default_rng(9100)
    n = 5000
    rows = [kc._spread_row(rng, n), kc._row(rng, n, {5: 40, 3: 900, 2: 3000, 1: 500})]
    c = kc._score_case("big_seam", n, rows, (4096, 4097, 4999, 5000, 5001, 100000))
    assert [is_big(n, mx) for mx in c.maxes] == [False, True, True, True, True, True]
    assert all(len(c.expected[0]["find"][mx][0]) == min(mx, n) for mx in c.maxes)
    assert first_tie_taken(c, 1, 4097)[0] == 1 and first_tie_taken(c, 1, 4999)[0] == 0
    return c


@functools.lru_cache(maxsize=None)
def fewer_refs():
    """3000 references, max = 5000: clipped to 3000, the LDS kernel's."""
    rng = np.random.default_rng(9110)
    c = kc._score_case("big_fewer_refs", 3000, [kc._spread_row(rng, 3000)], (5000,))
    assert not is_big(3000, 5000) and big_queries(c, 5000) == 0 and len(c.expected[0]["find"][5000][0]) == 3000
    return c


@functools.lru_cache(maxsize=None)
def zeros_fill():
    """17 positive scores in 20 000 references, max = 4500: the zeros with the largest ids fill the list (and the short
    cut's sample finds too few positives to place a threshold)."""
    rng = np.random.default_rng(9120)
    n = 20000
    c = kc._score_case("big_zeros_fill", n, [kc._row(rng, n, {5: 3, 2: 6, 1: 8})], (4500,))
    ids, sc = c.expected[0]["find"][4500]
    assert len(ids) == 4500 and (sc > 0).sum() == 17
    rest = np.setdiff1d(np.arange(n), ids[:17])
    assert (ids[17:] == rest[::-1][:4500 - 17]).all()
    m = kc._models(c, 0, 4500)
    assert m["T0"] == -1 and m["exit"] == "unusable"
    return c


@functools.lru_cache(maxsize=None)
def tie_split():
    """The row layout of kmer_cases.tie_split -- ties at the cut (score 2) dense below id 5120 and on every eighth id
    from there on, 20 000 references, four waves with ranges of 640 vectors read 64 at a time -- with 4200 more
    references above the cut, so that every M is above 4096: the first tie taken is the first id of wave range 1
    (5120), the last id of a 64-vector iteration, an id in mid-vector, and the last reference alone."""
    rng = np.random.default_rng(9130)
    n = 20000
    ids = np.arange(n)
    tie = (ids < 5120) | (ids % 8 == 0) | np.isin(ids, list(kc.TIE_FIRST.values()))
    tie[[7, 100, 5000]] = False
    free = np.flatnonzero(~tie & (ids >= 5120))
    above = rng.choice(free, 4210, replace=False)
    row = np.where(tie, 2, rng.integers(0, 2, size=n)).astype(np.int64)
    row[above] = 3
    maxes = {name: len(above) + int((tie & (ids >= x)).sum()) for name, x in kc.TIE_FIRST.items()}
    c = kc._score_case("big_tie_split", n, [row], sorted(set(maxes.values())))
    c.tie_maxes = maxes
    assert (2500 + 3) // 4 <= 640 and 640 * 8 == kc.TIE_FIRST["wave_range"]
    assert tie.sum() > SEL_MAX and min(maxes.values()) == len(above) + 1 > SEL_MAX
    for name, mx in maxes.items():
        cut, first, n_at = first_tie_taken(c, 0, mx)
        assert cut == 2 and first == kc.TIE_FIRST[name] and n_at == tie.sum() > SEL_MAX, name
    return c


SHORTCUT_M = 4500


@functools.lru_cache(maxsize=None)
def shortcut_exits():
    """20 000 references, M = 4500; the sample's target is 2 * 4500 / 16 + 8 = 570 scores.  Query 0, "found": 4700
    references of score 8 and 9, the threshold lands below them and at least M scores reach it.  Query 1, "fewer": 600
    references with the top score, all in sampled vectors -- T0 = 9, and only 600 < M reach it.  Query 2, "unusable":
    6000 positive scores, every one in a vector the sample does not read, so it places no threshold (a group of equal
    scores too large for the sample -- the other way to this exit -- needs 73 000 references at this M)."""
    rng = np.random.default_rng(9140)
    n = 20000
    found = kc._row(rng, n, {9: 500, 8: 4200, 7: 3000, 6: 3000})
    tops = kc._vector_ids(rng, n, True, 600)
    rest = np.setdiff1d(np.arange(n), tops)
    fewer = np.zeros(n, np.int64)
    fewer[rest] = kc._row(rng, len(rest), {8: 2000, 7: 3000, 5: 4000, 2: 3000})
    fewer[tops] = 9
    blind = np.zeros(n, np.int64)
    hi = kc._vector_ids(rng, n, False, 6000)
    blind[hi] = rng.integers(2, 10, size=len(hi))
    c = kc._score_case("big_shortcut_exits", n, [found, fewer, blind], (SHORTCUT_M,))
    m = [kc._models(c, qi, SHORTCUT_M) for qi in range(3)]
    assert m[0]["exit"] == "found" and m[0]["cut"] == 8 and m[0]["n_ge_cut"] == 4700 > SEL_MAX
    assert m[1]["exit"] == "fewer" and m[1]["T0"] == 9 and m[1]["n_ge_t0"] == 600 < SHORTCUT_M
    assert m[2]["exit"] == "unusable" and m[2]["T0"] == -1 and c.expected[2]["find"][SHORTCUT_M][1][-1] >= 2
    return c


@functools.lru_cache(maxsize=None)
def shortcut_not_tried_rows():
    """16 376 references are 2047 vectors: one too few for the short cut."""
    rng = np.random.default_rng(9150)
    n = 16376
    c = kc._score_case("big_shortcut_2047_vectors", n, [kc._spread_row(rng, n), kc._row(rng, n, {3: 5, 2: 5000, 1: 3000})],
                       (SHORTCUT_M,))
    assert all(kc._models(c, qi, SHORTCUT_M) is None for qi in range(2))
    assert kc.shortcut_model(np.zeros(16377, np.int64), SHORTCUT_M, len(c.qmasks[0]), c.k) is not None
    return c


@functools.lru_cache(maxsize=None)
def shortcut_not_tried_windows():
    """The rows of shortcut_exits behind queries padded with N to 10 240 bases: 10 234 windows are more bins than the
    histogram has, the 8-way search does it all."""
    rows = [e["scores"] for e in shortcut_exits().expected]
    c = kc._score_case("big_shortcut_8192_windows", 20000, rows, (SHORTCUT_M,), pad=kc.FAST_MAX)
    assert all(len(m) - c.k >= 8192 for m in c.qmasks) and all(kc._models(c, qi, SHORTCUT_M) is None for qi in range(3))
    assert all(kc._models(shortcut_exits(), qi, SHORTCUT_M) is not None for qi in range(3))
    return c


@functools.lru_cache(maxsize=None)
def everything(n_refs):
    """M == n_refs: the cut is 0 and nothing is skipped.  32 769: one score in the last vector, one reference in the
    second tile; 65 537: three tiles."""
    rng = np.random.default_rng(9160 + n_refs % 100)
    c = kc._score_case("big_everything_%d" % n_refs, n_refs, [kc._spread_row(rng, n_refs)], (n_refs,))
    ids, sc = c.expected[0]["find"][n_refs]
    assert len(ids) == n_refs and sc[-1] == 0 and ids[0] == n_refs - 1 and n_refs % 8 == 1 and n_refs > kc.TILE
    assert len(np.unique(ids)) == n_refs
    return c


@functools.lru_cache(maxsize=None)
def long_query():
    """Through kmer_topk_any: AAAA...A of 32 767 bases (half of the references score 32 761), a two-block query of
    more than 10 240 bases whose scores are {0, a, c, a + c} in giant groups, and a short query in front that stays on
    the fast kernel -- a launch range of its own."""
    rng = np.random.default_rng(9170)
    n, k = 20000, 6
    la, lc = 6000, 6500
    in_a, in_c = rng.random(n) < 0.5, rng.random(n) < 0.4
    lists = {kc.poly_kmer("A", k): np.flatnonzero(in_a).astype(np.uint32), kc.poly_kmer("C", k): np.flatnonzero(in_c).astype(np.uint32)}
    qs = [kc.poly("A", 40), kc.poly("A", kc.LONG_MAX), np.concatenate([kc.poly("A", la), [kc.N_MASK], kc.poly("C", lc)])]
    c = kc.Case("big_long_query", n, k, True, lists, qs, (5000,), dense_divs=(None,), long_api=True)
    c.n_long = 2
    assert [len(m) > kc.FAST_MAX for m in qs] == [False, True, True]
    assert c.expected[1]["scores"].max() == kc.LONG_MAX - k > 10240 and (c.expected[1]["scores"] > 10240).sum() > 5000
    assert set(np.unique(c.expected[2]["scores"])) == {0, la - k + 1, lc - k, la - k + 1 + lc - k} and la - k + 1 + lc - k > 10240
    assert launches_model(c, 5000) == 2
    return c


MIXED_M = 4500


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """One call, four queries over 20 000 references: a spread row, a two-valued row, a query with no windows (all
    zeros, nkq = 0: the top M are the M largest ids) and a row whose only positive score sits on the last reference."""
    rng = np.random.default_rng(9180)
    n = 20000
    two = np.where(rng.random(n) < 0.3, 7, 2).astype(np.int64)
    last = np.zeros(n, np.int64)
    last[n - 1] = 4
    rows = [kc._spread_row(rng, n), two, np.zeros(n, np.int64), last]
    c = kc._score_case("big_mixed_batch", n, rows, (MIXED_M,))
    assert len(kmer_ref.window_values(c.qmasks[2], c.k, False)) == 0
    assert (c.expected[2]["find"][MIXED_M][0] == np.arange(n - 1, n - 1 - MIXED_M, -1)).all()
    assert c.expected[3]["find"][MIXED_M][0][0] == n - 1 and c.expected[3]["find"][MIXED_M][1][1] == 0
    assert set(np.unique(two)) == {2, 7} and launches_model(c, MIXED_M) == 1
    return c


def seam_budgets():
    """big_sel_bytes settings for mixed_batch and the ranges they cut its four queries into.  Ranges are uniform (a
    budget holds so many queries of M candidates), so a seam "after the first query" is one query per range -- four
    launches -- and a seam "after the third" is three per range, two launches; two per range for completeness."""
    q = BIG_BYTES_PER_CAND * MIXED_M
    return {"after_first": (q, [1, 1, 1, 1]), "after_second": (2 * q + 5, [2, 2]), "after_third": (4 * q - 1, [3, 1]),
            "below_one_query": (1000, [1, 1, 1, 1])}


# ---------------------------------------------------------------- fuzz

def fuzz_seeds(n):
    """The seeds below n whose kmer_cases.fuzz_world has more than 4097 references (its first draw)."""
    out = []
    for seed in range(n):
        n_refs = kc.FUZZ_N_REFS[int(np.random.default_rng(8500 + seed).integers(0, len(kc.FUZZ_N_REFS)))]
        if n_refs > 4097:
            out.append(seed)
    return out


@functools.lru_cache(maxsize=None)
def fuzz_big(seed):
    """kmer_cases.fuzz_world(seed) with three random max values in 4097 .. n_refs + 10."""
    w = kc.fuzz_world(seed)
    assert w.n_refs > 4097
    rng = np.random.default_rng(9500 + seed)
    c = copy.copy(w)
    c.name = "big_fuzz_%d" % seed
    c.maxes = tuple(sorted(int(x) for x in rng.integers(4097, w.n_refs + 11, size=3)))
    c.__dict__["expected"] = [dict(scores=e["scores"], find={mx: kmer_ref.topk(e["scores"], mx) for mx in c.maxes})
                              for e in w.expected]
    return c


BIG_CASES = {"seam": seam, "fewer_refs": fewer_refs, "zeros_fill": zeros_fill, "tie_split": tie_split,
             "shortcut_exits": shortcut_exits, "shortcut_not_tried_rows": shortcut_not_tried_rows,
             "shortcut_not_tried_windows": shortcut_not_tried_windows,
             "everything_32769": functools.partial(everything, 32769), "everything_65537": functools.partial(everything, 65537),
             "long_query": long_query, "mixed_batch": mixed_batch}


def case(name):
    return BIG_CASES[name]()


# ---------------------------------------------------------------- the stage-level escalation world

ESC_FF = dict(fs_min_len=100, fs_req_full=1, fs_full_len=240)                  # the oracle's names
ESC_FF_OPTS = {"fs-min-len": 100, "fs-req-full": 1, "fs-full-len": 240}        # the stages'
ESC_N_MAIN, ESC_N_FOREIGN = 6000, 10


@functools.lru_cache(maxsize=None)
def escalation_world():
    """6000 references of about 200 bases in one dense clade, and behind them ten of about 260 bases from an ancestor of
    their own: with fs-full-len = 240 only those ten are full length.  A query out of the 6000 shares k-mers with most
    of them and none with the ten, so famfinder -- which wants one full-length relative -- widens its list 41, 410,
    4100, 6010 until the zero scores, largest ids first, bring the ten in."""
    main = synth.make_refs(ESC_N_MAIN, length=200, width=2000, seed=9601, n_clades=1, long_del_prob=0.0)
    foreign = synth.make_refs(ESC_N_FOREIGN, length=260, width=2000, seed=9602, n_clades=1, long_del_prob=0.0)
    off = np.concatenate([main.off, main.off[-1] + foreign.off[1:]])
    refs = synth.RefSet(ab=np.concatenate([main.ab, foreign.ab]), off=off, width=2000)
    sizes = np.diff(refs.off)
    assert (sizes[:ESC_N_MAIN] < 240).all() and (sizes[ESC_N_MAIN:] >= 240).all() and (sizes >= 100).all()
    return refs, main, foreign


@functools.lru_cache(maxsize=None)
def escalation_queries():
    """Sixteen queries: ten out of the 6000 (they escalate), six out of the ten full-length references (they do not)."""
    refs, main, foreign = escalation_world()
    a = synth.make_queries(main, 10, seed=9603)
    b = synth.make_queries(foreign, 6, seed=9604)
    off = np.concatenate([a.off, a.off[-1] + b.off[1:]])
    return synth.QuerySet(mask=np.concatenate([a.mask, b.mask]), off=off, src=np.concatenate([a.src, ESC_N_MAIN + b.src]))


def satisfied_by_top(scores, sizes, n_top, fs_full_len=240, fs_req_full=1):
    """Does famfinder's cascade end on the first n_top candidates by k-mer score?  With these options (fs-req-full = 1
    and every reference above fs-min-len) it does iff a full-length reference is among them."""
    ids, _ = kmer_ref.topk(scores, n_top)
    return int((sizes[ids] >= fs_full_len).sum()) >= fs_req_full
