"""Directed inputs of the ranking tests, shared by tests/test_rank_cpu.py (which checks every case's declared number of
flagged queries against tests/rank_ref.py and the oracle) and tests/test_gpu_rank.py (which runs them through
sina_hip_compare_rank).

A case is a function returning a dict: width, refs, qs (packed base lists as in tests/compare_cases.py), cand (an id
list per query, or None: every reference in id order), names (one per reference; their byte-wise order breaks ties),
n_best, cover, rule, flc, chunk (None, or the SINA_HIP_TEST=rank_chunk value the launch is cut with) and flagged (how
many queries must come back flagged).  Every builder asserts, in plain numpy, the property it exists for.  CPU work."""
import functools

import numpy as np

from tests import compare_cases as cc
from tests import rank_ref

WAVES = 4            # waves of a workgroup: each keeps a list of its own, merged at the end
MAX_BEST = 64


def _names(n):
    """ref0 .. ref<n-1>: byte-wise, ref10 < ref2 -- the name order is not the id order."""
    return ["ref%d" % i for i in range(n)]


def _case(width, refs, qs, cand, n_best, cover="query", rule=0, flc=False, chunk=None, flagged=0, names=None):
    names = _names(len(refs)) if names is None else names
    assert len(names) == len(refs) and 1 <= n_best <= MAX_BEST
    return dict(width=width, refs=refs, qs=qs, cand=cand, names=names, n_best=n_best, cover=cover, rule=rule, flc=flc,
                chunk=chunk, flagged=flagged)


def lists_of(case):
    """The id list of every query (all references where the case says None)."""
    if case["cand"] is None:
        return [np.arange(len(case["refs"]), dtype=np.uint32) for _ in case["qs"]]
    return case["cand"]


def expected_of(case):
    """(ids [nq, n_best], score bits, n, flag) by the plain walk and tests/rank_ref.py."""
    cand = lists_of(case)
    rows = cc.walk_all(case["refs"], case["qs"], cand, case["rule"], case["flc"])
    return rank_ref.rank_call(rows, cand, rank_ref.name_order(case["names"]), case["cover"], case["n_best"])


# ---------------------------------------------------------------- list lengths

def _lengths_case(n_best):
    def build():
        refs = cc._small_world(6101, 300)
        lens = sorted({0, 1, n_best - 1, n_best, n_best + 1, WAVES - 1, WAVES, WAVES + 1, 257})
        qs = cc._small_world(6102, len(lens))
        rng = np.random.default_rng(6103 + n_best)
        cand = [rng.permutation(300)[:n].astype(np.uint32) for n in lens]
        assert {0, 1, n_best, n_best + 1, 3, 4, 5, 257} <= set(len(c) for c in cand) and 257 > 4 * MAX_BEST
        return _case(90, refs, qs, cand, n_best)
    return build


# ---------------------------------------------------------------- ties

def _ties(chunk):
    def build():
        base_cols = list(range(10, 70, 2))
        q = cc.seq(base_cols)
        m = cc.masks(q).copy()

        def variant(n_wrong):
            mm = m.copy()
            mm[:n_wrong] = np.where(mm[:n_wrong] == 1, 2, 1)
            return cc.seq(base_cols, mm)
        tied = variant(6)
        refs = [variant(1), tied, tied, variant(2), tied, tied, tied, variant(9), tied, tied, tied, variant(3), tied, tied,
                tied, variant(10), tied, tied, tied, variant(11)]
        refs = [r.copy() for r in refs]
        case = _case(90, refs, [q], [np.arange(20, dtype=np.uint32)], 10, chunk=chunk)
        ids, sb, n, flag = expected_of(case)
        tied_ids = [i for i in range(20) if (refs[i] == tied).all()]
        assert len(tied_ids) == 14 and n[0] == 10 and list(ids[0, :3]) == [0, 3, 11]
        got_tied = list(ids[0, 3:])
        # the tie straddles place 10: seven of the fourteen get in, the seven LAST names -- not the seven largest ids
        assert len(set(sb[0, 3:])) == 1 and set(got_tied) < set(tied_ids)
        by_name = sorted(tied_ids, key=lambda i: case["names"][i].encode(), reverse=True)
        assert got_tied == by_name[:7] and got_tied != sorted(tied_ids, reverse=True)[:7]
        assert case["names"][10].encode() < case["names"][2].encode() and 2 in got_tied and 10 not in got_tied
        if chunk:                        # the tied candidates lie in more than one chunk, winners and losers in each
            assert len({i // chunk for i in got_tied}) > 1 and len({i // chunk for i in tied_ids if i not in got_tied}) > 1
        return case
    return build


# ---------------------------------------------------------------- zero scores

def _zeros(n_best):
    def build():
        q = cc.seq(range(20, 40))
        other = np.where(cc.masks(q) == 1, 2, 1)
        zero_a = cc.seq(range(20, 40), other)            # every column shared, every base another: match 0
        zero_b = cc.seq(range(41, 61))                   # right of the query: match 0, the denominator is the query
        refs = [zero_a, cc.seq(range(20, 40)), zero_b, zero_a.copy(), zero_b.copy(), cc.seq(range(20, 30)), zero_a.copy(),
                zero_b.copy()]
        names = ["m", "k", "a", "z", "c", "b", "y", "d"]   # id 2 has the first name of all: its key is all zero bits
        case = _case(90, refs, [q], [np.arange(8, dtype=np.uint32)], n_best, names=names)
        ids, sb, n, flag = expected_of(case)
        rank = rank_ref.name_order(names)
        assert rank[2] == 0 and list(ids[0, :2]) == [1, 5] and (sb[0, 2:n[0]] == 0).all() and flag[0] == 0
        assert n[0] == min(n_best, 8)
        if n_best >= 8:
            assert ids[0, 7] == 2 and sb[0, 7] == 0        # the all-zero key holds the last place
        else:
            assert 2 not in ids[0, :n[0]] and list(ids[0, 2:5]) == [3, 6, 0]
        return case
    return build


# ---------------------------------------------------------------- scores above one

def cover_abs():
    refs = cc._small_world(6101, 300)
    qs = cc._small_world(6102, 4)
    cand = [np.arange(300, dtype=np.uint32)[::3], np.arange(5, dtype=np.uint32), np.arange(100, 300, dtype=np.uint32),
            np.arange(300, dtype=np.uint32)]
    case = _case(90, refs, qs, cand, 10, cover="abs")
    ids, sb, n, flag = expected_of(case)
    assert (sb[:, 0].view(np.float32) > 1).all() and (flag == 0).all()
    return case


# ---------------------------------------------------------------- no score at all

def _nan(kind):
    def build():
        q0 = cc.seq(range(10, 31))
        far = cc.seq(range(50, 71))                                        # no column range in common
        gaps = cc.seq(range(11, 30, 2))                                    # inside the range, on other columns
        lower = cc.seq(range(10, 31), lower=range(21))                     # lower case throughout
        refs = [cc.seq(range(10, 31, 2)), far, cc.seq(range(12, 40)), cc.seq(range(5, 25)), lower, gaps]
        q_even = cc.seq(range(10, 31, 2))
        assert not set(cc.cols(gaps)) & set(cc.cols(q_even))
        if kind == "overlap":
            qs, cand, kw = [q0, cc.seq(range(12, 28)), cc.seq(range(14, 26))], [[0, 1, 2, 3], [0, 2, 3], [3, 2, 0]], dict(cover="overlap")
        elif kind == "nogap":
            qs, cand, kw = [cc.seq(range(12, 28)), q_even, cc.seq(range(14, 26))], [[0, 2, 3, 5], [0, 5, 2], [0, 2, 3, 5]], dict(cover="nogap")
        else:
            qs, cand, kw = [cc.seq(range(12, 28)), cc.seq(range(14, 26)), q0], [[0, 2, 3], [2, 3, 0], [0, 4, 2, 3]], dict(flc=True)
        cand = [np.array(c, np.uint32) for c in cand]
        case = _case(90, refs, qs, cand, 3, flagged=1, **kw)
        ids, sb, n, flag = expected_of(case)
        want = {"overlap": [1, 0, 0], "nogap": [0, 1, 0], "lower": [0, 0, 1]}[kind]
        assert list(flag) == want and (n[flag == 0] == 3).all()
        return case
    return build


# ---------------------------------------------------------------- an id twice in a list

def duplicates():
    width, refs, qs, cand = cc.case("cand_lists")
    case = _case(width, refs, qs, cand, 3, cover="all")
    ids, sb, n, flag = expected_of(case)
    assert list(cand[9]).count(7) == 2 and list(ids[9, :n[9]]).count(7) == 2       # both copies get a place
    return case


# ---------------------------------------------------------------- forced chunks

def chunks_of_ten():
    refs = cc._small_world(6201, 10)
    q = refs[9].copy()
    case = _case(90, refs + [], [q, cc._small_world(6202, 1)[0]], [np.arange(10, dtype=np.uint32)] * 2, 4, chunk=3)
    ids, sb, n, flag = expected_of(case)
    assert ids[0, 0] == 9 and 9 // 3 == 3 and 10 % 3 == 1          # the best candidate alone in the last, short chunk
    return case


def _all_refs(n_refs, chunk=4):
    def build():
        refs = cc._small_world(6211, n_refs)
        qs = [refs[n_refs - 1].copy(), refs[0].copy(), cc._small_world(6212, 1)[0]]
        case = _case(90, refs, qs, None, 5, chunk=chunk)
        ids, sb, n, flag = expected_of(case)
        assert n_refs in (3 * chunk - 1, 3 * chunk, 3 * chunk + 1) and ids[0, 0] == n_refs - 1 and ids[1, 0] == 0
        assert (n == 5).all()
        return case
    return build


def all_refs_one_chunk():
    """Every reference, no knob: one chunk per query and no merge launch at this size."""
    refs = cc._small_world(6221, 70)
    return _case(90, refs, cc._small_world(6222, 5), None, 64, cover="max")


# ---------------------------------------------------------------- few and many queries

def _cc_world(name, n_best, cover):
    def build():
        width, refs, qs, cand = cc.case(name)
        return _case(width, refs, qs, cand, n_best, cover=cover)
    return build


CASES = {}
for _n in (1, 10, 64):
    CASES["lengths_%d" % _n] = _lengths_case(_n)
CASES.update(ties=_ties(None), ties_chunks=_ties(3), zeros_5=_zeros(5), zeros_8=_zeros(8), cover_abs=cover_abs,
             nan_overlap=_nan("overlap"), nan_nogap=_nan("nogap"), nan_lower=_nan("lower"), duplicates=duplicates,
             chunks_of_ten=chunks_of_ten, all_refs_11=_all_refs(11), all_refs_12=_all_refs(12), all_refs_13=_all_refs(13),
             all_refs_one_chunk=all_refs_one_chunk, nq_1=_cc_world("nq_1", 2, "target"), nq_600=_cc_world("nq_600", 2, "target"))
NAMES = sorted(CASES)

# tests/compare_cases.py worlds of width 90 and up that the device's rows are also held against, under every setting
CC_WORLDS = ("ranges", "filter", "mask_table_lc", "lengths", "cand_lists", "nwords_257", "lds_wide")


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    cc.check_wellformed(c["width"], c["refs"], c["qs"], lists_of(c))
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    return expected_of(case(name))


@functools.lru_cache(maxsize=None)
def cc_expected(world, cover, rule, flc, n_best):
    """A compare_cases world under names ref0, ref1, ...: the expected rows from its cached counters."""
    width, refs, qs, cand = cc.case(world)
    rows = cc.expected(world)[rule, flc]
    return rank_ref.rank_call(rows, cand, rank_ref.name_order(_names(len(refs))), cover, n_best)


def plan(nq, M, n_cu, floor=128, forced=0, wg_per_cu=4, grid_max=0x7FFFFFFF):
    """Mirror of rank_plan() in sina_amd/csrc/rank_plan.h: (chunk, chunks)."""
    if nq == 0 or M == 0 or nq > grid_max:
        return 0, 0
    if forced:
        chunk = forced
    else:
        want = wg_per_cu * max(n_cu, 1)
        per_query = max(1, (want + nq - 1) // nq)
        chunk = max((M + per_query - 1) // per_query, floor)
    room = grid_max // nq
    if (M + chunk - 1) // chunk > room:
        chunk = (M + room - 1) // room
    chunk = min(chunk, M)
    return chunk, (M + chunk - 1) // chunk


# ---------------------------------------------------------------- the stage-level world (tests/test_gpu_rank_stage.py)
# A store of tests/test_gpu_search.py's kind.  name -> (search options of the stage, the oracle's, kind of queries,
# references).  "full": queries derived from whole references; "fragments": pieces of 100 to 160 bases, which share
# no column with some of the shorter references -- under cover nogap such a pair has no score.

STAGE_FF = {"fs-min-len": 100, "fs-full-len": 250}
STAGE = {
    "query": ({}, {}, "full", 300),
    "abs": ({"search-cover": "abs", "search-min-sim": 100}, dict(cover="abs", min_sim=100.0), "full", 300),
    "all": ({"search-cover": "all", "search-min-sim": 0.5, "search-max-result": 7}, dict(cover="all", min_sim=0.5, max_result=7), "full", 300),
    "average": ({"search-cover": "average", "search-iupac": "pessimistic"}, dict(cover="average", iupac="pessimistic"), "full", 300),
    "max": ({"search-cover": "max", "search-min-sim": -1, "search-max-result": 64}, dict(cover="max", min_sim=-1.0, max_result=64), "full", 300),
    "target": ({"search-cover": "target", "search-kmer-candidates": 40, "search-filter-lowercase": True},
               dict(cover="target", kmer_candidates=40, filter_lc=1), "full", 300),
    "min": ({"search-cover": "min", "search-iupac": "exact", "search-max-result": 1}, dict(cover="min", iupac="exact", max_result=1), "full", 300),
    "nogap_fragments": ({"search-cover": "nogap", "search-min-sim": 0.0}, dict(cover="nogap", min_sim=0.0), "fragments", 300),
    "overlap_fragments": ({"search-cover": "overlap", "search-min-sim": 0.0}, dict(cover="overlap", min_sim=0.0), "fragments", 300),
    "search_all": ({"search-all": True, "search-max-result": 12}, dict(search_all=1, max_result=12), "full", 150),
}
STAGE_NAMES = sorted(STAGE)
FRAGMENT_LENGTHS = (100, 120, 140, 160, 110, 130, 150, 105, 125, 145, 155, 160)


def stage_taxonomy(i):
    phyla = ["Proteobacteria", "Firmicutes", "Bacteroidota"]
    return "Bacteria;%s;class%d;order%d;" % (phyla[i % 3], i % 6, i % 12)


@functools.lru_cache(maxsize=None)
def stage_refs(n_refs):
    from sina_amd import synth
    return synth.make_refs(n_refs, length=300, width=3000, seed=651, amb_rate=0.01, lower_rate=0.03)


@functools.lru_cache(maxsize=None)
def stage_queries(kind, n_refs):
    """A QuerySet: 14 queries derived from whole references and two exact pieces, or twelve fragments."""
    from sina_amd import synth
    refs = stage_refs(n_refs)
    if kind == "full":
        qs = synth.make_queries(refs, 14, seed=652, amb_rate=0.01, lower_rate=0.05)
        masks = [qs.seq(i) for i in range(qs.n)]
        masks += [((refs.seq(i) >> 24) & 0xff).astype(np.uint8)[a:b] for i, a, b in ((5, 10, 250), (77, 0, 200))]
    else:
        rng = np.random.default_rng(653)
        full = np.flatnonzero(np.diff(refs.off) >= 280)
        masks = []
        for n in FRAGMENT_LENGTHS:
            m = ((refs.seq(int(full[int(rng.integers(len(full)))])) >> 24) & 0xff).astype(np.uint8)
            a = int(rng.integers(0, len(m) - n + 1))
            piece = m[a:a + n].copy()
            sub = rng.random(n) < 0.03
            piece[sub] = rng.choice([1, 2, 4, 8], size=int(sub.sum()))
            masks.append(piece)
    off = np.zeros(len(masks) + 1, np.int64)
    off[1:] = np.cumsum([len(m) for m in masks])
    return synth.QuerySet(mask=np.concatenate(masks), off=off, src=np.zeros(len(masks), np.int64))


@functools.lru_cache(maxsize=None)
def stage_reference_run(name):
    """The oracle, query by query, on a stage case: a list with, per query, None (not searched) or a dict(ids, scores,
    nan) -- the search results and whether any of the query's candidates has a NaN score, i.e. whether the device must
    flag the query.  Also pins the order: the oracle's rows are tests/rank_ref.py's from the oracle's counters."""
    from oracle import pyoracle as po
    from tests import util
    sopts, oopts, kind, n_refs = STAGE[name]
    refs = stage_refs(n_refs)
    qs = stage_queries(kind, n_refs)
    cs = util.cseqs_from_refs(refs)
    idx = po.Index(cs, k=10)
    so = po.search_opts(**oopts)
    iupac, cover, flc = oopts.get("iupac", "optimistic"), oopts.get("cover", "query"), bool(oopts.get("filter_lc", 0))
    name_rank = rank_ref.name_order(_names(refs.n))
    out = []
    for qi in range(qs.n):
        q = util.query_cseq(qs, qi, upper=False)
        ids, sc, _ = idx.famfinder(q, po.ff_opts(fs_min_len=100, fs_full_len=250))
        al = po.align([cs[i] for i in ids], q, po.align_opts(realign=1)) if len(ids) else None
        if al is None or al["status"] not in (0, 1):
            out.append(None)
            continue
        aligned = po.Cseq.from_packed("query%d" % qi, al["packed"], al["width"])
        want_ids, want_sc, _ = po.search(idx, aligned, so)
        if want_ids is None:
            out.append(None)
            continue
        if oopts.get("search_all"):
            cand = np.arange(refs.n, dtype=np.uint32)
        else:
            cand, _ = idx.find(aligned, min(int(oopts.get("kmer_candidates", 1000)), refs.n))
            cand = np.asarray(cand, np.uint32)
        rows = [po.compare_counts(aligned, cs[int(i)], iupac, flc) for i in cand]
        nan = any(np.isnan(po.compare(aligned, cs[int(i)], iupac, "none", cover, flc)) for i in cand)
        r_ids, r_bits, r_flag = rank_ref.rank_query(rows, cand, name_rank, cover, int(oopts.get("max_result", 10)))
        assert bool(r_flag) == nan, (name, qi)
        if not nan:       # (with a NaN among them the reference's own order is whatever partial_sort leaves)
            min_sim = np.float32(oopts.get("min_sim", 0.7))
            cut = next((k for k in range(len(r_ids)) if not np.uint32(r_bits[k]).view(np.float32) > min_sim), len(r_ids))
            assert list(want_ids) == r_ids[:cut], (name, qi, list(want_ids), r_ids[:cut])
            assert [rank_ref.bits(x) for x in want_sc] == r_bits[:cut], (name, qi)
        out.append(dict(ids=want_ids, scores=want_sc, nan=nan))
    return out


# ---------------------------------------------------------------- repeated queries (one batch, dedup is per batch)
# kind of queries -> the stage case it runs under.  30 trays of which 12 are distinct, all in one batch.
REPEAT_STAGE = {"full": "query", "fragments": "overlap_fragments"}
REPEAT_SEED = 660


def stage_repeat_pick(kind):
    """(distinct, pick): twelve of the kind's queries, ascending, and the 30 trays -- every one of the twelve at least
    once, eighteen more drawn among them, shuffled.  tests/test_rank_cpu.py asserts that the fragments' pick repeats a
    query the reference flags."""
    n = stage_queries(kind, 300).n
    rng = np.random.default_rng(REPEAT_SEED)
    distinct = np.sort(rng.choice(n, 12, replace=False))
    pick = np.concatenate([distinct, rng.choice(distinct, 18)])
    rng.shuffle(pick)
    return distinct, pick
