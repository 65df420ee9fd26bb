"""One align call with every rider on: the in-place pair count (sina_hip_align_count_pairs), the family
identity (sina_hip_align_count_identity, 3.5c), the ranking (sina_hip_align_rank, 3.5d) and, under assemble = 2, the
shift log -- launch_inplace_counts' three kernels back to back behind the assembly, fetch_results' four differently
sized rows at q_base offsets, align_call's per-entry and per-call decisions -- on the launches of tests/riders_cases.py
through sina_hip_align_families, _families_wsets, _profiles, _graphs and _graphs_any.

The yardstick is the oracle's finished sequence alone (riders_cases.expected); tests/test_riders_cpu.py checks on the
CPU that every launch reaches its edge.  Every comparison is bit for bit."""
import itertools
import threading

import numpy as np
import pytest

from sina_amd import capi
from tests import rank_cases as rc, rank_ref, riders_cases as rdc, util, walk_cases as wc
from tests.test_gpu_search_inplace import _align as _family_align, _switch as _rank_switch

pytestmark = pytest.mark.gpu

ALL = frozenset(rdc.RIDERS)
SUBSETS = [frozenset(s) for n in (1, 2) for s in itertools.combinations(rdc.RIDERS, n)]
NO_KNOBS = dict(dp_range_q=None, fam_chunk_q=None, rank_chunk=None)


def _load(ctx, rd):
    l = rd.launch
    ctx.upload_refs(l.refs.ab, l.refs.off.astype(np.uint64), l.refs.width)
    ctx.build_index(k=l.search["k"])
    if rd.name_order:
        ctx.upload_name_order(rank_ref.name_order(l.names))
    ctx.upload_pairs(rd.helix)


class _Ctx:
    """A context that remembers which store it holds: launches that share references, name order and map share it."""

    def __init__(self):
        self.c = capi.Context(0)
        self.key = None

    def hold(self, rd):
        key = (id(rd.launch.refs), rd.name_order, rd.helix.tobytes())
        if self.key != key:
            _load(self.c, rd)
            self.key = key
        return self.c


@pytest.fixture(scope="module")
def holder():
    h = _Ctx()
    yield h
    h.c.close()


def _align(ctx, rd, assemble):
    l = rd.launch
    if rd.entry == "any":
        opts = wc.Case("opts", l.width, [], [], **l.opts).opts
        gb = ctx.graph_batch([g for g, _, _ in rd.batch], rd.batch_width)
        qoff = np.zeros(rd.nq + 1, np.uint64)
        qoff[1:] = np.cumsum([len(m) for _, m, _ in rd.batch])
        p = ctx.params(overhang=opts["overhang"], lowercase=opts["lowercase"], insertion=opts["insertion"], assemble=assemble)
        return ctx.align_graphs_any(gb, np.concatenate([m for _, m, _ in rd.batch]), qoff, p)
    return _family_align(ctx, l, assemble=assemble, graphs=rd.entry == "graphs")


def _stats(ctx):
    return dict(pairs=ctx.pair_inplace_stats(), identity=ctx.identity_inplace_stats(), rank=ctx.rank_inplace_stats(),
                assemble=ctx.assemble_stats(), rank_trip=ctx.rank_stats(), pair_trip=ctx.pair_stats(),
                compare_trip=ctx.stats()["compare_launches"])


def _switches(ctx, l, on):
    ctx.count_pairs("pairs" in on)
    ctx.count_identity("identity" in on)
    _rank_switch(ctx, l, "rank" in on)


def _call(ctx, rd, on, monkeypatch, assemble=None, knobs=None):
    """One align call of the launch with the riders of `on` switched on, under the launch's knobs: dict(out, pos, pairs,
    identity, rank, shift -- the staged rows, None where the getter gives NULL --, before, after -- the counters)."""
    l = rd.launch
    _switches(ctx, l, on)
    util.set_knobs(monkeypatch, **NO_KNOBS)
    util.set_knobs(monkeypatch, **(rd.knobs if knobs is None else knobs))
    try:
        before = _stats(ctx)
        out, pos = _align(ctx, rd, l.assemble if assemble is None else assemble)
        log = ctx.staged_shift_log()
        got = dict(out=out, pos=pos, pairs=ctx.staged_pair_counts(), identity=ctx.staged_identity(), rank=ctx.staged_rank(),
                   shift=None if log is None else rdc.shift_rows(log), before=before, after=_stats(ctx))
    finally:
        _switches(ctx, l, frozenset())
        util.set_knobs(monkeypatch, **NO_KNOBS)
    return got


def _same_rows(rd, rider, got, want, what="the oracle's"):
    """got == want row for row; a mismatch names the launch, the rider, the first differing query and its launch range."""
    assert got is not None, (rd.name, rider, "the getter gave NULL")
    assert got.shape == want.shape, (rd.name, rider, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad):
        q = int(bad[0])
        r = rdc.range_of(rd, q)
        where = "the wide path" if r is None else "range %d (q_base %d, %d queries) of %s" % ((r,) + rdc.ranges(rd)[r] + (rdc.ranges(rd),))
        raise AssertionError("%s: rider %s differs from %s rows first at query %d, in %s: got %s, want %s"
                             % (rd.name, rider, what, q, where, got[q].tolist(), want[q].tolist()))


def _delta(got, key):
    return {k: got["after"][key][k] - got["before"][key][k] for k in got["after"][key] if k != "kernel_ms"}


def _active(rd, on):
    """The riders and the shift log a call of this launch with the switches `on` carries."""
    act = set(on)
    if rd.entry in ("graphs", "any"):
        act.discard("identity")                       # (no family comes to the device)
    if rd.name in rdc.RANK_OFF:
        act.discard("rank")
    return act


def _check_counters(rd, want, got, on):
    """Each rider's counters move by what that rider's own test expects of it alone."""
    l, ref, slots = rd.launch, want["ref"], rd.slots()
    act = _active(rd, on)
    n_ranges = len(rdc.ranges(rd))
    fast = [(q, s) for q, s in enumerate(slots) if s is not None]
    must = [(q, s) for q, s in fast if ref[s]["must"]]
    ranked = [(q, s) for q, s in fast if ref[s]["ranked"]]
    exp = dict(pairs=dict(sequences=len(must), launches=n_ranges),
               identity=dict(sequences=len(must), pairs=sum(len(l.fam_ids[s]) for _, s in must), launches=n_ranges),
               rank=dict(sequences=len(ranked), pairs=sum(len(ref[s]["cand"]) for _, s in ranked), launches=n_ranges))
    for rider in rdc.RIDERS:
        d = _delta(got, rider)
        zero = {k: 0 for k in d}
        assert d == (exp[rider] if rider in act else zero), (rd.name, rider, sorted(on), d, exp[rider], rdc.ranges(rd))
        assert got["after"][rider]["kernel_ms"] >= got["before"][rider]["kernel_ms"], (rd.name, rider)
    ev = want["events"] or [[] for _ in slots]
    assert _delta(got, "assemble") == dict(queries=len(fast), assembled=len(must), shifted_queries=sum(bool(ev[q]) for q, _ in must),
                                           shifted_runs=sum(len(ev[q]) for q, _ in must)), (rd.name, _delta(got, "assemble"))
    # no second trip: the re-upload routes' counters stand still
    for trip in ("rank_trip", "pair_trip", "compare_trip"):
        assert got["after"][trip] == got["before"][trip], (rd.name, trip)


def _check_rows(rd, want, got, on, base=None):
    """The active riders' rows against `base` (the all-on call's) or the oracle's; an inactive rider's getter gives NULL."""
    act = _active(rd, on)
    for rider in rdc.RIDERS:
        if rider not in act:
            assert got[rider] is None, (rd.name, rider, sorted(on), "rows staged by a rider that is not active")
            continue
        if base is None:
            _same_rows(rd, rider, got[rider], want[rider])
        else:
            _same_rows(rd, rider, got[rider], base[rider], what="the all-on call's")
    if rd.launch.assemble == 2:
        _same_rows(rd, "shift log", got["shift"], want["shift"])
    else:
        assert got["shift"] is None, rd.name


def _check(holder, rd, want, monkeypatch):
    ctx = holder.hold(rd)
    l, ref, slots = rd.launch, want["ref"], rd.slots()
    # 1. the reference call: every rider off, no knobs
    plain = _call(ctx, rd, frozenset(), monkeypatch, knobs={})
    out0, pos0 = plain["out"], plain["pos"]
    assert all(plain[r] is None for r in rdc.RIDERS), rd.name
    _check_counters(rd, want, plain, frozenset())
    assert (out0["status"] == 0).all(), rd.name
    assert [int(a) for a in out0["assembled"]] == [int(s is not None and ref[s]["must"]) for s in slots], rd.name
    # 2. everything on, under the launch's knobs
    full = _call(ctx, rd, ALL, monkeypatch)
    assert full["out"].tobytes() == out0.tobytes() and full["pos"].tobytes() == pos0.tobytes(), rd.name
    _check_rows(rd, want, full, ALL)
    _check_counters(rd, want, full, ALL)
    print(rd.name, "ranges", rdc.ranges(rd), "pairs num", full["pairs"][:, 0].tolist(),
          "ranked n", None if full["rank"] is None else full["rank"][:, 0].tolist(),
          "scored", None if full["identity"] is None else full["identity"][:, 1].tolist(),
          "events", None if full["shift"] is None else full["shift"][:, 0].tolist())
    # 3. the same call with each rider alone and with each pair of riders
    for on in SUBSETS:
        got = _call(ctx, rd, on, monkeypatch)
        assert got["out"].tobytes() == out0.tobytes() and got["pos"].tobytes() == pos0.tobytes(), (rd.name, sorted(on))
        _check_rows(rd, want, got, on, base=full)
        _check_counters(rd, want, got, on)
    return full


@pytest.mark.parametrize("name", rdc.NAMES)
def test_all_riders_in_one_call(oracle, holder, monkeypatch, name):
    """The table of tests/riders_cases.py: ranges under build chunks (a non-zero chunk base), shifted queries, host-
    finished ones, lost bases, the ranking's flag, zero k-mer scores and name tie behind the other riders, the other
    entries, the wide path's zero rows, a store without a name order."""
    rd, want = rdc.case(name)
    _check(holder, rd, want, monkeypatch)


def test_no_stale_rows_between_calls(oracle, holder, monkeypatch):
    """all-on all-ranges, all-unassembled with only the pairs on, all-on all-ranges again: the third call's rows are the
    first's, the second's identity and ranking getters give NULL.  Then a call with the shift log (assemble = 2) and a
    call the entry refuses before it begins: every getter gives NULL -- a refused call has counted nothing."""
    rd, want = rdc.case("all-ranges")
    ud, uwant = rdc.case("all-unassembled")
    assert ud.launch.refs is rd.launch.refs
    ctx = holder.hold(rd)
    first = _call(ctx, rd, ALL, monkeypatch)
    _check_rows(rd, want, first, ALL)
    second = _call(ctx, ud, frozenset(["pairs"]), monkeypatch)
    assert second["identity"] is None and second["rank"] is None and second["shift"] is None
    _same_rows(ud, "pairs", second["pairs"], uwant["pairs"])
    assert second["pairs"].shape[0] < first["pairs"].shape[0]
    third = _call(ctx, rd, ALL, monkeypatch)
    for rider in rdc.RIDERS:
        _same_rows(rd, rider, third[rider], first[rider], what="the first call's")
    assert third["out"].tobytes() == first["out"].tobytes() and third["pos"].tobytes() == first["pos"].tobytes()
    shifted = _call(ctx, rd, ALL, monkeypatch, assemble=2)
    assert shifted["shift"] is not None and shifted["shift"].shape == (rd.nq, rdc.SHIFT_WORDS)
    for rider in rdc.RIDERS:                    # (this world's insertions fit their gaps: assemble = 2 finishes what 1 does)
        _same_rows(rd, rider, shifted[rider], first[rider], what="the first call's")
    _switches(ctx, rd.launch, ALL)
    try:
        fam, foff = rd.launch.packed_families()
        qmask, qoff = rd.launch.packed_queries()
        foff = foff.copy()
        foff[1] = foff[0]                       # an empty family: refused by name, before anything is launched
        with pytest.raises(capi.SinaHipError, match="family size"):
            ctx.align_families(fam, foff, qmask, qoff, ctx.params(assemble=2))
        assert ctx.staged_pair_counts() is None and ctx.staged_identity() is None and ctx.staged_rank() is None
        assert ctx.staged_shift_log() is None
    finally:
        _switches(ctx, rd.launch, frozenset())
    again = _call(ctx, rd, ALL, monkeypatch)
    _check_rows(rd, want, again, ALL)


def test_forks_with_every_rider_run_concurrently(oracle, monkeypatch):
    """Three forks of one context, every rider on in each, each with a launch of its own -- all-ranges, all-unassembled,
    all-lost-bases -- on one store (identity_cases' world with the overhang launch's cut references behind it), twice
    each behind a barrier, all under all-ranges' knobs: every result and every staged row equals what the same fork gave
    alone."""
    rds = [rdc.case(n)[0] for n in ("all-ranges", "all-unassembled", "all-lost-bases")]
    big = rds[2].launch.refs
    assert (big.ab[:len(rds[0].launch.refs.ab)] == rds[0].launch.refs.ab).all() and rds[1].launch.refs is rds[0].launch.refs
    util.set_knobs(monkeypatch, **NO_KNOBS)
    util.set_knobs(monkeypatch, **rdc.RANGES_KNOBS)
    ctx = capi.Context(0)
    forks = []
    try:
        ctx.upload_refs(big.ab, big.off.astype(np.uint64), big.width)
        ctx.build_index(k=10)
        ctx.upload_name_order(rank_ref.name_order(rc._names(big.n)))
        ctx.upload_pairs(rds[0].helix)
        forks = [ctx.fork() for _ in rds]

        def run(i):
            f, rd = forks[i], rds[i]
            out, pos = _align(f, rd, rd.launch.assemble)
            return dict(out=out, pos=pos, pairs=f.staged_pair_counts(), identity=f.staged_identity(), rank=f.staged_rank())

        alone = []
        for i, rd in enumerate(rds):
            _switches(forks[i], rd.launch, ALL)
            alone.append(run(i))
            assert all(alone[i][r] is not None for r in rdc.RIDERS) and alone[i]["pairs"].any() and alone[i]["identity"].any(), rd.name
        barrier = threading.Barrier(len(rds))
        got, errors = [[] for _ in rds], []

        def work(i):
            try:
                barrier.wait(timeout=60)
                for _ in range(2):
                    got[i].append(run(i))
            except Exception as e:  # noqa: BLE001
                errors.append((i, repr(e)))

        ts = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(rds))]
        [t.start() for t in ts]
        [t.join(timeout=120) for t in ts]
        assert not any(t.is_alive() for t in ts), "a fork's thread did not come back"
        assert not errors, errors
        for i, rd in enumerate(rds):
            assert len(got[i]) == 2, rd.name
            for g in got[i]:
                assert g["out"].tobytes() == alone[i]["out"].tobytes() and g["pos"].tobytes() == alone[i]["pos"].tobytes(), rd.name
                for rider in rdc.RIDERS:
                    _same_rows(rd, rider, g[rider], alone[i][rider], what="the same fork's own, alone,")
    finally:
        for f in forks:
            f.close()
        ctx.close()
