"""The search stage's ranking where the device assembles the alignment (rank_assembled_kernel):
sina_hip_align_rank / sina_hip_staged_rank / sina_hip_rank_inplace_stats through sina_hip_align_families,
_families_wsets, _profiles and _graphs on the launches of tests/search_inplace_cases.py.

The yardstick is the oracle's k-mer search over the input bases, tests/compare_ref.py over the oracle's finished
sequences and tests/rank_ref.py; the re-upload route (sina_hip_kmer_topk_rank over the words the call returned) is asked
for the same rows.  tests/test_search_inplace_cpu.py checks on the CPU that these inputs are worth running."""
import numpy as np
import pytest

from sina_amd import capi
from tests import rank_ref, search_inplace_cases as sic, util, walk_cases as wc

pytestmark = pytest.mark.gpu

ZERO = dict(kernel_ms=0.0, sequences=0, pairs=0, launches=0)


class _Ctx:
    """A context that remembers which store it holds: the launches of a group mostly share one."""

    def __init__(self):
        self.c = capi.Context(0)
        self.refs = None

    def hold(self, launch):
        if self.refs is not launch.refs:
            _load(self.c, launch)
            self.refs = launch.refs
        return self.c


def _load(ctx, launch, k=None, order=True):
    ctx.upload_refs(launch.refs.ab, launch.refs.off.astype(np.uint64), launch.refs.width)
    ctx.build_index(k=launch.search["k"] if k is None else k)
    if order:
        ctx.upload_name_order(rank_ref.name_order(launch.names))


@pytest.fixture(scope="module")
def holder():
    h = _Ctx()
    yield h
    h.c.close()


def _switch(ctx, launch, on=True):
    s = launch.search
    ctx.rank_assembled(on, k=s["k"], kmer_candidates=s["cands"], iupac=s["rule"], filter_lc=s["flc"], cover=s["cover"],
                       max_result=s["n_best"])


def _align(ctx, launch, assemble=None, graphs=False):
    fam, foff = launch.packed_families()
    qmask, qoff = launch.packed_queries()
    assemble = launch.assemble if assemble is None else assemble
    opts = wc.Case("opts", launch.width, [], [], **launch.opts).opts
    popts = {k: v for k, v in opts.items() if k not in ("fs_no_graph", "weights")}
    if graphs:
        gb = ctx.graph_batch([util.graph_dict(util.cseqs_from_refs(launch.refs, f)) for f in launch.fam_ids], launch.width)
        return ctx.align_graphs(gb, qmask, qoff, ctx.params(assemble=assemble, **popts))
    if opts["fs_no_graph"]:
        return ctx.align_profiles(fam, foff, qmask, qoff, ctx.params(assemble=assemble, **popts))
    if launch.sets is not None:
        return ctx.align_families_wsets(fam, foff, qmask, qoff, ctx.params_wsets(launch.weight_vectors, assemble=assemble, **popts),
                                        launch.sets, len(launch.weight_vectors))
    return ctx.align_families(fam, foff, qmask, qoff, ctx.params(assemble=assemble, **popts))


def _reupload_rows(ctx, launch, out, pos, ranked):
    """The rows by the old route: sina_hip_kmer_topk_rank over the finished words of the ranked queries."""
    _, qoff = launch.packed_queries()
    rows = np.zeros((len(out), sic.ROW_WORDS), np.uint32)
    if not ranked:
        return rows
    parts = [pos[int(qoff[q]):int(qoff[q]) + int(out[q]["n_out"])] for q in ranked]
    q_off = np.zeros(len(ranked) + 1, np.uint64)
    q_off[1:] = np.cumsum([len(p) for p in parts])
    s = launch.search
    ids, sc, n, flag = ctx.kmer_topk_rank(np.concatenate(parts).astype(np.uint32), q_off, s["cands"], iupac=s["rule"], filter_lc=s["flc"],
                                          cover=s["cover"], max_result=s["n_best"])
    for x, q in enumerate(ranked):
        rows[q, 0], rows[q, 1] = n[x], sic.RANKED | int(flag[x])
        rows[q, 2:2 + s["n_best"]] = ids[x]
        rows[q, 2 + sic.MAX_BEST:2 + sic.MAX_BEST + s["n_best"]] = util.f32_bits(sc[x])
    return rows


def _ranges(launch):
    n, per = len(launch.qmasks), launch.knobs.get("dp_range_q")
    return (n + per - 1) // per if per else 1


def _check_launch(holder, launch, ref, monkeypatch, graphs=False):
    ctx = holder.hold(launch)
    want = sic.rows(ref)
    util.set_knobs(monkeypatch, dp_range_q=None, rank_chunk=None)
    _switch(ctx, launch, False)
    s_off = ctx.rank_inplace_stats()
    out0, pos0 = _align(ctx, launch, graphs=graphs)
    assert ctx.staged_rank() is None and ctx.rank_inplace_stats() == s_off, launch.name
    assert (out0["status"] == 0).all(), launch.name
    assert [int(a) for a in out0["assembled"]] == [int(r["must"]) for r in ref], launch.name
    util.set_knobs(monkeypatch, **launch.knobs)
    _switch(ctx, launch)
    s0, r0 = ctx.rank_inplace_stats(), ctx.rank_stats()
    out, pos = _align(ctx, launch, graphs=graphs)
    rows = ctx.staged_rank()
    s1, r1 = ctx.rank_inplace_stats(), ctx.rank_stats()
    _switch(ctx, launch, False)
    util.set_knobs(monkeypatch, dp_range_q=None, rank_chunk=None)
    assert r1 == r0, launch.name                                         # no second trip
    assert rows is not None and rows.shape == (len(ref), sic.ROW_WORDS), launch.name
    print(launch.name, "n", rows[:, 0].tolist(), "flags", rows[:, 1].tolist())
    bad = np.flatnonzero((rows != want).any(axis=1))
    assert len(bad) == 0, (launch.name, "query %d" % bad[0], rows[bad[0]].tolist(), want[bad[0]].tolist())
    assert out.tobytes() == out0.tobytes() and pos.tobytes() == pos0.tobytes(), launch.name
    ranked = [q for q in range(len(ref)) if ref[q]["ranked"]]
    assert s1["launches"] - s0["launches"] == _ranges(launch), (launch.name, s0, s1)
    assert s1["sequences"] - s0["sequences"] == len(ranked), (launch.name, s0, s1)
    assert s1["pairs"] - s0["pairs"] == sum(len(ref[q]["cand"]) for q in ranked), (launch.name, s0, s1)
    assert s1["kernel_ms"] >= s0["kernel_ms"], launch.name
    again = _reupload_rows(ctx, launch, out, pos, ranked)
    assert (again == rows).all(), (launch.name, "the re-upload route differs", again.tolist(), rows.tolist())
    return rows


@pytest.mark.parametrize("name", sic.NAMED)
def test_rows_of_the_named_cases(oracle, holder, monkeypatch, name):
    """Candidate counts around N and the four waves, max_result of 1, 10 and 64, every cover rule, a query without a
    k-mer hit, a tie across place N decided by name, a candidate without a score (bit 0), a query that lost bases and
    unassembled ones (zero rows), shifted ones (assemble = 2) without and with the lower-case filter, launch ranges and
    rank chunks."""
    for launch, ref in sic.group(name):
        _check_launch(holder, launch, ref, monkeypatch)


@pytest.mark.parametrize("name", sic.OTHER_ENTRIES)
def test_rows_through_the_other_entries(oracle, holder, monkeypatch, name):
    """sina_hip_align_profiles (--fs-no-graph), sina_hip_align_families_wsets (a weight vector per query) and
    sina_hip_align_graphs (the caller's DAGs)."""
    for launch, ref in sic.group(name):
        _check_launch(holder, launch, ref, monkeypatch, graphs=name == "graphs")


def test_ranges_give_the_rows_of_the_whole_call(oracle, holder, monkeypatch):
    launches = sic.group("ranges")
    whole = sic.rows(launches[0][1])
    assert len(whole) == 10 and [sorted(l.knobs) for l, _ in launches[1:]] == [["dp_range_q"], ["rank_chunk"], ["dp_range_q", "rank_chunk"]]
    for launch, ref in launches[1:]:
        assert (_check_launch(holder, launch, ref, monkeypatch) == whole).all(), launch.name


def test_nothing_ranked(oracle):
    """NULL and no launch with the switch off, with assemble = 0, without an index, without a name order, with an index
    of another k, on a fresh fork; an unranked call after a ranked one returns NULL, not the rows before.  The align
    results are the same in each."""
    (launch, ref), = sic.group("graphs")
    want = sic.rows(ref)
    ctx = capi.Context(0)
    try:
        ctx.upload_refs(launch.refs.ab, launch.refs.off.astype(np.uint64), launch.refs.width)
        assert ctx.rank_inplace_stats() == ZERO and ctx.staged_rank() is None    # no align call yet
        out0, pos0 = _align(ctx, launch)                                         # off

        def same(got):
            return got[0].tobytes() == out0.tobytes() and got[1].tobytes() == pos0.tobytes()
        assert ctx.staged_rank() is None and ctx.rank_inplace_stats() == ZERO
        _switch(ctx, launch)                                                     # on: no index
        assert same(_align(ctx, launch)) and ctx.staged_rank() is None and ctx.rank_inplace_stats() == ZERO
        ctx.build_index(k=launch.search["k"])                                    # an index, no name order
        assert same(_align(ctx, launch)) and ctx.staged_rank() is None and ctx.rank_inplace_stats() == ZERO
        ctx.upload_name_order(rank_ref.name_order(launch.names))
        a0 = _align(ctx, launch, assemble=0)                                     # everything there, assemble = 0
        assert ctx.staged_rank() is None and ctx.rank_inplace_stats() == ZERO and (a0[0]["assembled"] == 0).all()
        assert same(_align(ctx, launch)) and (ctx.staged_rank() == want).all()   # ranked ...
        one = ctx.rank_inplace_stats()
        assert one["launches"] == 1 and one["sequences"] == len(ref)
        _align(ctx, launch, assemble=0)                                          # ... then not: no stale rows
        assert ctx.staged_rank() is None and ctx.rank_inplace_stats() == one
        assert same(_align(ctx, launch, graphs=True)) and (ctx.staged_rank() == want).all()
        ctx.build_index(k=8)                                                     # an index of another k
        assert same(_align(ctx, launch)) and ctx.staged_rank() is None
        ctx.build_index(k=launch.search["k"])
        assert same(_align(ctx, launch)) and (ctx.staged_rank() == want).all()
        two = ctx.rank_inplace_stats()
        fork = ctx.fork()                                                        # the parent is on: the fork is not
        try:
            assert fork.staged_rank() is None
            assert same(_align(fork, launch)) and fork.staged_rank() is None and fork.rank_inplace_stats() == ZERO
            _switch(fork, launch)
            assert same(_align(fork, launch)) and (fork.staged_rank() == want).all()
        finally:
            fork.close()
        assert ctx.rank_inplace_stats() == two
    finally:
        ctx.close()


def test_switch_refuses_what_the_rank_entry_refuses(oracle):
    (launch, _), = sic.group("graphs")
    ctx = capi.Context(0)
    try:
        _load(ctx, launch)
        for bad in (dict(max_result=0), dict(max_result=65), dict(kmer_candidates=0), dict(iupac=3), dict(k=0)):
            with pytest.raises(capi.SinaHipError):
                ctx.rank_assembled(True, **bad)
        ctx.rank_assembled(True, kmer_candidates=5000)          # clamps to the store's 160 references
        ctx.rank_assembled(False, max_result=0)                 # off: the rest is not looked at
        _align(ctx, launch)
        assert ctx.staged_rank() is None
    finally:
        ctx.close()


# ---------------------------------------------------------------- through the stages (the worlds of tests/rank_cases.py)

from sina_amd import pipeline, synth  # noqa: E402
from tests import rank_cases as rc, test_gpu_rank_stage as rs  # noqa: E402

IN_PLACE = {"realign": True, "device-search": True, "device-shift": True}
PLAIN = {"realign": True}


def _stage_run(st, qs, sopts, aligner, device_rank=None, single=None, batch=10):
    search = dict({"lca-fields": "tax_slv"}, **sopts)
    if device_rank is not None:
        search["device-rank"] = device_rank
    before = (st.search_inplace_stats(), st.rank_stats(), st.assemble_stats())
    pl = pipeline.Pipeline(st, famfinder=rc.STAGE_FF, aligner=aligner, search=search)
    if single is None:
        pl.run(qs.mask, qs.off, batch=batch, inflight=2)
    else:
        failed, err = pl.run_single_trays(qs.mask, qs.off, threads=single, max_batch=single)
        assert not failed.any(), err
    out = []
    for q in range(qs.n):
        r = pl.result(q)
        out.append(dict(ids=r["search_ids"], scores=r["search_scores"], log=r["log"],
                        nearest=pl.attr(q, "nearest_slv") if r["search_ids"] is not None else None,
                        lca=pl.attr(q, "lca_tax_slv") if r["search_ids"] is not None else None))
    pl.close()
    after = (st.search_inplace_stats(), st.rank_stats(), st.assemble_stats())
    return out, [{k: a[k] - b[k] for k in a} for a, b in zip(after, before)]


@pytest.fixture(scope="module")
def stage_stores():
    stores = {}

    def get(n_refs):
        if n_refs not in stores:
            stores[n_refs] = pipeline.Store(":mem:search-inplace-%d" % n_refs, rc.stage_refs(n_refs))
            rs._annotate(stores[n_refs], n_refs)
        return stores[n_refs]
    yield get
    for st in stores.values():
        st.close()


@pytest.mark.parametrize("name", rc.STAGE_NAMES)
def test_stage_takes_its_rows_in_place(stage_stores, name):
    """device-search + device-shift against both off: ids, score bits, nearest_slv, lca_tax_slv and the whole log of
    every query are equal (and the oracle's, where tests/test_gpu_rank_stage.py says so); the trays the device
    assembled take their rows in place -- all but those a candidate without a score flags --, the stage's own path
    (host, or device-rank beside it) handles exactly the rest."""
    sopts, oopts, kind, n_refs = rc.STAGE[name]
    qs = rc.stage_queries(kind, n_refs)
    ref_run = rc.stage_reference_run(name)
    st = stage_stores(n_refs)
    off, (s_off, r_off, a_off) = _stage_run(st, qs, sopts, PLAIN)
    assert s_off["trays"] == 0 and s_off["launches"] == 0 and s_off["sequences"] == 0
    on, (s_on, r_on, a_on) = _stage_run(st, qs, sopts, IN_PLACE)
    rs._same(off, on)
    searched = sum(1 for r in on if r["ids"] is not None)
    flagged = sum(1 for r in ref_run if r is not None and r["nan"])
    assembled = a_on["trays_device"]
    print(name, "searched", searched, "device-assembled", assembled, "in place", s_on["trays"], "flagged", flagged, s_on)
    assert searched == sum(1 for r in ref_run if r is not None) and assembled >= 10
    if oopts.get("search_all"):
        assert s_on["trays"] == 0 and s_on["launches"] == 0                  # (sina_hip_compare_rank serves search-all)
        return
    # (a flagged tray -- the fragments' worlds have them: a candidate that shares no column with the query -- is the host's)
    assert assembled - flagged <= s_on["trays"] <= assembled and s_on["trays"] >= 1
    assert s_on["sequences"] >= s_on["trays"]                                  # ranked on the device, flagged ones included
    assert s_on["launches"] >= 1 and s_on["sequences"] >= 1 and s_on["pairs"] >= s_on["sequences"]
    assert r_on["ranked"] == 0 and r_on["launches"] == 0                       # the rest went the host's way
    if not name.endswith("_fragments"):
        assert flagged == 0 and s_on["trays"] == assembled
        for q, r in enumerate(ref_run):
            if r is not None:
                assert on[q]["ids"].tolist() == list(r["ids"]) and util.f32_bits(on[q]["scores"]).tolist() == util.f32_bits(r["scores"]).tolist()
    # device-rank beside it: the rest, and only the rest, goes through sina_hip_kmer_topk_rank
    both, (s_b, r_b, a_b) = _stage_run(st, qs, sopts, IN_PLACE, device_rank=True)
    rs._same(off, both)
    assert s_b["trays"] == s_on["trays"] and r_b["ranked"] + r_b["fallen_back"] == searched - s_b["trays"]


def test_stage_single_trays_and_run_fasta(stage_stores, tmp_path):
    sopts, oopts, kind, n_refs = rc.STAGE["query"]
    qs = rc.stage_queries(kind, n_refs)
    st = stage_stores(n_refs)
    off, _ = _stage_run(st, qs, sopts, PLAIN)
    for threads in (8, 1):
        got, (s, _, a) = _stage_run(st, qs, sopts, IN_PLACE, single=threads)
        rs._same(off, got)
        assert s["trays"] == a["trays_device"] >= 10, threads
    src = str(tmp_path / "in.fasta")
    with open(src, "w") as f:
        for q in range(qs.n):
            f.write(">q%d\n%s\n" % (q, synth.bases_string(qs.seq(q))))
    runs = {}
    for on in (0, 1):
        dst = str(tmp_path / ("out%d.fasta" % on))
        s0 = st.search_inplace_stats()
        got = pipeline.run_fasta(st, src, dst, famfinder=rc.STAGE_FF, aligner=dict(PLAIN, **{"device-search": on, "device-shift": on}),
                                 search={"lca-fields": "tax_slv"}, fasta={"meta-fmt": "comment"}, batch=8)
        recs = [l for l in open(dst).read().splitlines() if not l.startswith(";aligned_slv")]     # (the date)
        runs[on] = (got, recs, st.search_inplace_stats()["trays"] - s0["trays"])
    assert runs[0][:2] == runs[1][:2] and any("nearest_slv" in l for l in runs[1][1])
    assert runs[0][2] == 0 and runs[1][2] >= 10


@pytest.mark.parametrize("name,sopts", [
    ("jc", {"search-correction": "jc", "search-cover": "target", "search-min-sim": 0.0}),
    ("ignore_super", {"search-ignore-super": True, "search-min-sim": 0.0}),
    ("max_result_65", {"search-max-result": 65, "search-min-sim": 0.0}),
])
def test_stage_option_changes_nothing(stage_stores, name, sopts):
    """Where the stage's options are not the ones the device ranks under, the aligner ranks nothing and the results
    are those without the option.  (A search-kmer-len other than the store's index cannot be set up through the
    stages -- a store keeps one index, reference_store::ensure_index refuses a second --: test_nothing_ranked has it
    at the device, tests/search_plan_check.cpp in the plan.)"""
    kind = "fragments" if name == "jc" else "full"
    qs = rc.stage_queries(kind, 300)
    st = stage_stores(300)
    off, _ = _stage_run(st, qs, sopts, PLAIN)
    on, (s, _, a) = _stage_run(st, qs, sopts, IN_PLACE)
    rs._same(off, on)
    assert s["trays"] == 0 and s["launches"] == 0 and s["sequences"] == 0 and a["trays_device"] >= 10


def test_stage_other_search_db_changes_nothing(stage_stores):
    """search-db names another store than the aligner's: its candidates are not the aligner's references."""
    qs = rc.stage_queries("full", 300)
    st, other = stage_stores(300), stage_stores(150)
    out = {}
    for on in (False, True):
        s0 = (st.search_inplace_stats(), other.search_inplace_stats())
        pl = pipeline.Pipeline(st, famfinder=rc.STAGE_FF, aligner=dict(PLAIN, **{"device-search": on, "device-shift": on}),
                               search={"lca-fields": "tax_slv", "search-db": other.key, "search-min-sim": 0.0})
        pl.run(qs.mask, qs.off, batch=10, inflight=2)
        out[on] = [(pl.result(q)["search_ids"], pl.result(q)["log"]) for q in range(qs.n)]
        pl.close()
        assert (st.search_inplace_stats(), other.search_inplace_stats()) == s0
    for (a, la), (b, lb) in zip(out[False], out[True]):
        assert (a is None) == (b is None) and la == lb and (a is None or a.tolist() == b.tolist())
    assert sum(1 for a, _ in out[True] if a is not None) >= 10


def test_stage_repeated_name_changes_nothing(tmp_path):
    refs = rc.stage_refs(300)
    qs = rc.stage_queries("full", 300)
    db = str(tmp_path / "twice.fasta")
    with open(db, "w") as f:
        for i in range(refs.n):
            f.write(">%s\n%s\n" % ("ref%d" % (7 if i == 211 else i), synth.aligned_string(refs.seq(i), refs.width)))
    st = pipeline.Store.open(db)
    try:
        rs._annotate(st, refs.n)
        off, _ = _stage_run(st, qs, {"search-min-sim": 0.0}, PLAIN)
        on, (s, _, a) = _stage_run(st, qs, {"search-min-sim": 0.0}, IN_PLACE)
        rs._same(off, on)
        assert s["trays"] == 0 and s["launches"] == 0 and a["trays_device"] >= 10
    finally:
        st.close()
