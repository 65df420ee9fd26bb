"""The inputs of the combined riders' tests: one align call with the in-place pair count, the family
identity (3.5c), the ranking (3.5d) and, under assemble = 2, the shift log all active, shared by tests/test_riders_cpu.py
(which asserts with the oracle alone that every launch reaches the edge it is there for) and tests/test_gpu_riders.py
(which runs them through the align entries).  Everything here is CPU work.

A launch is one of tests/search_inplace_cases.py (which extends identity_cases.Launch: one launch serves every rider)
with knobs of its own and a nested helix map of its width.  Its expected rows come from the oracle's finished sequence
alone, per query:
  ranking    sic.rows(reference)                                          [130]
  identity   identity_cases.row_of(packed, members), (0, 0) where the device must not assemble    [2]
  pairs      bps_ref.counts(packed, helix), six zeros where the device must not assemble         [6]
  shift log  (assemble = 2) the events of the oracle's log, zero-padded   [1 + 3 * 32]
A query of the wide path (sina_hip_align_graphs_any) has zero rows in all of them."""
import functools

import numpy as np

from tests import bps_ref as br, identity_cases as ic, search_inplace_cases as sic, shift_cases as sc, shift_ref as sr, util
from tests import walk_cases as wc, wide_cases as wd

PAIR_WORDS, IDTY_WORDS, SHIFT_WORDS = 6, 2, 1 + 3 * sr.SHIFT_LOG
RIDERS = ("pairs", "identity", "rank")


def helix_map(width, step=10):
    """Nested: column c with column width - c, every step-th column (tests/test_gpu_align_entries.py's map for step 10:
    where synth's worlds have their bases)."""
    helix = np.zeros(width, np.uint32)
    for c in range(step, width // 2, step):
        helix[c], helix[width - c] = width - c, c
    return helix


class Riders:
    """launch: a sic.Launch (knobs: this table's, not sic's); entry: "families" (which of _families, _families_wsets and
    _profiles follows from the launch, as in test_gpu_search_inplace.py), "graphs" or "any"; name_order: whether the
    store gets one; helix: the store's map; batch (entry "any"): [(graph, qmask, launch query or None for a wide-path
    query)] and the batch's width."""

    def __init__(self, name, launch, entry="families", name_order=True, helix_step=10, batch=None, batch_width=None):
        self.name, self.launch, self.entry, self.name_order = name, launch, entry, name_order
        self.helix = helix_map(launch.width, helix_step)
        self.batch, self.batch_width = batch, batch_width

    @property
    def knobs(self):
        return self.launch.knobs

    @property
    def nq(self):
        return len(self.batch) if self.batch is not None else len(self.launch.qmasks)

    def slots(self):
        """Per query of the call: its index among the launch's queries, None for a wide-path query."""
        return [b[2] for b in self.batch] if self.batch is not None else list(range(self.nq))


def _relaunch(name, base, knobs=None):
    """The sic launch under another name and other knobs; the alignments are shared (align_key)."""
    return sic.Launch(name, base, align_key=base.align_key, assemble=base.assemble, knobs=knobs, **base.search)


def cut(nq, chunk_q=0, range_q=0):
    """align_family_batches' cut of nq queries as (q0, r0, r1): build chunks of chunk_q queries (fam_chunk_q), launch
    ranges of range_q inside each (dp_range_q); 0: not cut.  (dp_cut_range itself does not cut worlds of this size.)
    align_graphs has no chunks: chunk_q = 0."""
    out = []
    for q0 in range(0, nq, chunk_q or nq):
        bq = min(chunk_q or nq, nq - q0)
        for r0 in range(0, bq, range_q or bq):
            out.append((q0, r0, min(bq, r0 + (range_q or bq))))
    return out


def ranges(rd):
    """[(q_base, queries)] of the fast path's launch ranges of the call."""
    if rd.entry == "any":       # maximal runs of fitting queries (a query that fails the spill-row limit splits its run)
        out, inside = [], False
        for q, s in enumerate(rd.slots()):
            if s is not None and inside:
                out[-1] = (out[-1][0], out[-1][1] + 1)
            elif s is not None:
                out.append((q, 1))
            inside = s is not None
        return out
    chunk = 0 if rd.entry == "graphs" else int(rd.knobs.get("fam_chunk_q", 0))
    return [(q0 + r0, r1 - r0) for q0, r0, r1 in cut(rd.nq, chunk, int(rd.knobs.get("dp_range_q", 0)))]


def range_of(rd, q):
    """The number of the launch range that holds query q, None for a wide-path query."""
    for i, (b, n) in enumerate(ranges(rd)):
        if b <= q < b + n:
            return i
    return None


def _shift_events(launch):
    """Per query the (N, B, E) events of the oracle's log (assemble = 2: shift_cases' world, its alignments there)."""
    w = sc.dp_world()
    assert launch.refs is w["refs"] and len(launch.qmasks) == len(w["want"])
    return [sc.log_events(r["log"]) for r in w["want"]]


def expected(rd):
    """dict(ref: sic.reference's list per LAUNCH query; rank [nq, 130], identity [nq, 2] or None where the entry brings
    no family to the device, pairs [nq, 6], shift [nq, 97] or None, events: per query the shift log as the getter
    gives it) -- rows laid out like the call's `out`."""
    l = rd.launch
    ref = sic.reference(l)
    rank = np.zeros((rd.nq, sic.ROW_WORDS), np.uint32)
    idty = np.zeros((rd.nq, IDTY_WORDS), np.uint32)
    pairs = np.zeros((rd.nq, PAIR_WORDS), np.uint32)
    events = _shift_events(l) if l.assemble == 2 else None
    shift = np.zeros((rd.nq, SHIFT_WORDS), np.uint32) if l.assemble == 2 else None
    for q, s in enumerate(rd.slots()):
        if s is None:
            continue
        r = ref[s]
        rank[q] = r["row"]
        if r["must"]:
            idty[q] = ic.row_of(r["packed"], [l.refs.seq(int(i)) for i in l.fam_ids[s]])[:2]
            pairs[q] = br.counts(r["packed"], rd.helix)
        if shift is not None:
            if l.assemble == 2:
                assert len(r["packed"]) == len(sc.dp_world()["want"][s]["packed"]) and (r["packed"] == sc.dp_world()["want"][s]["packed"]).all()
            ev = events[s]
            assert len(ev) <= sr.SHIFT_LOG
            shift[q, 0] = len(ev)
            shift[q, 1:1 + 3 * len(ev)] = np.asarray(ev, np.uint32).reshape(-1)
    return dict(ref=ref, rank=rank, identity=None if rd.entry in ("graphs", "any") else idty, pairs=pairs, shift=shift,
                events=[events[s] if s is not None else [] for s in rd.slots()] if events is not None else None)


def shift_rows(log):
    """staged_shift_log()'s per-query event lists as rows [nq, 97]."""
    rows = np.zeros((len(log), SHIFT_WORDS), np.uint32)
    for q, ev in enumerate(log):
        rows[q, 0] = len(ev)
        rows[q, 1:1 + 3 * len(ev)] = np.asarray(ev, np.uint32).reshape(-1)
    return rows


# ---------------------------------------------------------------- the launches

RANGES_KNOBS = dict(dp_range_q=3, fam_chunk_q=4, rank_chunk=16)
SHIFTED_KNOBS = dict(dp_range_q=5, fam_chunk_q=6)
RANGES_CUT = [(0, 0, 3), (0, 3, 4), (4, 0, 3), (4, 3, 4), (8, 0, 2)]          # q_base 0, 3, 4, 7, 8
SHIFTED_CUT = [(0, 0, 5), (0, 5, 6), (6, 0, 5), (6, 5, 6), (12, 0, 4)]         # q_base 0, 5, 6, 11, 12


def _one(group, name=None):
    ls = sic.GROUPS[group]()
    return ls[0] if name is None else [l for l in ls if l.name == name][0]


ANY_FIT = 4
ANY_WIDTHS = {"all-any-mixed": 40000, "all-any-mixed-ranked": 70000}


@functools.lru_cache(maxsize=None)
def _any_launch():
    """The four fitting queries of test_gpu_wide.py's mixed batch -- the first of walk_cases' matrix on `small` -- as a
    launch on `small`'s store, their families the oracle's famfinder's (what walk_cases._fam_of takes)."""
    refs, qs, cs, idx = wc.world_small()
    case = wc.cases_matrix()[0]
    fams = []
    for qi in range(ANY_FIT):
        ids, _, _ = idx.famfinder(util.query_cseq(qs, qi))
        fams.append([int(i) for i in ids])
    base = ic.Launch("any-fit", refs, fams, case.qmasks[:ANY_FIT], overhang=case.opts["overhang"], lowercase=case.opts["lowercase"],
                     insertion=0)
    return sic.Launch("any-fit", base, cands=40)


def _any(name, over):
    """test_mixed_batch_routes_per_query's order: fitting 0, two over-limit, fitting 1 and 2, far-edges (which passes the
    cheap limits and splits the fast run), fitting 3."""
    l = _any_launch()
    ref = wc.group("matrix")[0][1]
    fit = [(ref[q]["graph"], l.qmasks[q], q) for q in range(ANY_FIT)]
    ov = [(c.graph, c.qmasks[0], None) for c in over]
    return Riders(name, l, entry="any", batch=[fit[0], ov[0], ov[1], fit[1], fit[2], ov[2], fit[3]], batch_width=ANY_WIDTHS[name])


def _build():
    out = [
        Riders("all-ranges", _relaunch("all-ranges", sic.launches_ranges()[0], RANGES_KNOBS)),
        # the same with 40 of the store's 160 references as candidates: with all 160 every query has the same candidates,
        # and a ranking that read another query's candidate row would give the same rows
        Riders("all-ranges-40", sic.Launch("all-ranges-40", sic.launches_ranges()[0], align_key="ranges", knobs=RANGES_KNOBS, cands=40)),
        Riders("all-shifted", _relaunch("all-shifted", _one("shifted", "shifted-flc1"), SHIFTED_KNOBS), helix_step=SHIFT_HELIX_STEP),
        Riders("all-unassembled", _relaunch("all-unassembled", _one("unassembled"))),
        Riders("all-lost-bases", _relaunch("all-lost-bases", _one("overhang_remove"))),
        Riders("all-nan", _relaunch("all-nan", _one("nan"))),
        Riders("all-no-hit", _relaunch("all-no-hit", _one("no_hit"))),
        Riders("all-tie", _relaunch("all-tie", _one("tie"))),
        Riders("all-profiles", _relaunch("all-profiles", _one("profiles"))),
        Riders("all-wsets", _relaunch("all-wsets", _one("wsets"))),
        Riders("all-graphs", _relaunch("all-graphs", _one("graphs")), entry="graphs"),
        # the mix of test_gpu_wide.py as it is: its 10 241-base query is beyond the k-mer count kernel's length, and an
        # align call with such a query does not rank at all (align_call::begin_rank) -- pairs count, the ranking is off
        _any("all-any-mixed", [wd.fan_in(), wd.long_query(), wd.far_edges()]),
        # ... and with the 66 000-node chain (a 12-base query) in its place: the ranking rides, the wide-path queries keep
        # zero rows in every rider
        _any("all-any-mixed-ranked", [wd.fan_in(), wd.long_chain(), wd.far_edges()]),
        Riders("all-no-name-order", _relaunch("all-no-name-order", sic.launches_ranges()[0], dict(dp_range_q=3)), name_order=False),
    ]
    assert all(r.nq <= 16 for r in out)
    return out


# shift_cases' block layout (blocks of 20 columns, 6 free between): every second column, so that both partners of a pair
# often carry a base
SHIFT_HELIX_STEP = 2
NAMES = ("all-ranges", "all-ranges-40", "all-shifted", "all-unassembled", "all-lost-bases", "all-nan", "all-no-hit", "all-tie", "all-profiles",
         "all-wsets", "all-graphs", "all-any-mixed", "all-any-mixed-ranked", "all-no-name-order")
# the launches whose call does not rank, and why
RANK_OFF = {"all-any-mixed": "a query beyond SINA_HIP_MAX_QUERY_LEN", "all-no-name-order": "no name order"}


@functools.lru_cache(maxsize=None)
def launches():
    out = _build()
    assert tuple(r.name for r in out) == NAMES
    return {r.name: r for r in out}


@functools.lru_cache(maxsize=None)
def case(name):
    """(Riders, expected(...)) of a launch of the table, computed once per process and left unchanged."""
    rd = launches()[name]
    return rd, expected(rd)
