"""--calc-idty where the device assembles the alignment (family_identity_kernel):
sina_hip_align_count_identity / sina_hip_staged_identity / sina_hip_identity_inplace_stats through
sina_hip_align_families, _families_wsets and _profiles on the launches of tests/identity_cases.py, and the aligner's
device-idty through the stages.

The yardstick is tests/compare_ref.py over the oracle's finished sequences, scored in numpy float32; the re-upload
route (sina_hip_compare over the words the call returned, the maximum taken here) is asked for the same rows.
tests/test_identity_cpu.py checks on the CPU that these inputs are worth running."""
import numpy as np
import pytest

from sina_amd import capi, pipeline, synth
from tests import identity_cases as ic, test_gpu_pipeline as gp, util, walk_cases as wc

pytestmark = pytest.mark.gpu


class _Ctx:
    """A context that remembers which store it holds: the launches of a group mostly share one."""

    def __init__(self):
        self.c = capi.Context(0)
        self.refs = None

    def hold(self, refs):
        if self.refs is not refs:
            self.c.upload_refs(refs.ab, refs.off.astype(np.uint64), refs.width)
            self.refs = refs
        return self.c


@pytest.fixture(scope="module")
def holder():
    h = _Ctx()
    yield h
    h.c.close()


def _align(ctx, launch, assemble=1):
    fam, foff = launch.packed_families()
    qmask, qoff = launch.packed_queries()
    opts = wc.Case("opts", launch.width, [], [], **launch.opts).opts
    popts = {k: v for k, v in opts.items() if k not in ("fs_no_graph", "weights")}
    if opts["fs_no_graph"]:
        return ctx.align_profiles(fam, foff, qmask, qoff, ctx.params(assemble=assemble, **popts))
    if launch.sets is not None:
        return ctx.align_families_wsets(fam, foff, qmask, qoff, ctx.params_wsets(launch.weight_vectors, assemble=assemble, **popts),
                                        launch.sets, len(launch.weight_vectors))
    return ctx.align_families(fam, foff, qmask, qoff, ctx.params(assemble=assemble, **popts))


def _reupload_rows(ctx, launch, out, pos):
    """The rows by the old route: sina_hip_compare over the finished words of the assembled queries and their
    families' members, the overlap score and the maximum taken here."""
    _, qoff = launch.packed_queries()
    rows = np.zeros((len(out), 2), np.uint32)
    idx = [q for q in range(len(out)) if out[q]["assembled"]]
    if not idx:
        return rows
    parts = [pos[int(qoff[q]):int(qoff[q]) + int(out[q]["n_out"])] for q in idx]
    q_off = np.zeros(len(idx) + 1, np.uint64)
    q_off[1:] = np.cumsum([len(p) for p in parts])
    c_off = np.zeros(len(idx) + 1, np.uint64)
    c_off[1:] = np.cumsum([len(launch.fam_ids[q]) for q in idx])
    cand = np.concatenate([np.asarray(launch.fam_ids[q], np.uint32) for q in idx])
    counts = ctx.compare(np.concatenate(parts).astype(np.uint32), q_off, cand, c_off, iupac=0, filter_lc=False)
    for x, q in enumerate(idx):
        bits = [ic.score_bits(tuple(int(v) for v in counts[y])) for y in range(int(c_off[x]), int(c_off[x + 1]))]
        scored = [b for b, ok in bits if ok]
        rows[q] = (max(scored) if scored else 0, len(scored))
    return rows


def _check_launch(holder, launch, ref):
    ctx = holder.hold(launch.refs)
    want = ic.rows(ref)
    ctx.count_identity(False)
    s_off = ctx.identity_inplace_stats()
    out0, pos0 = _align(ctx, launch)
    assert ctx.staged_identity() is None and ctx.identity_inplace_stats() == s_off, launch.name
    assert (out0["status"] == 0).all(), launch.name
    assert [int(a) for a in out0["assembled"]] == [int(r["must"]) for r in ref], launch.name
    ctx.count_identity(True)
    s0, c0 = ctx.identity_inplace_stats(), ctx.stats()["compare_launches"]
    out, pos = _align(ctx, launch)
    rows = ctx.staged_identity()
    s1 = ctx.identity_inplace_stats()
    ctx.count_identity(False)
    assert ctx.stats()["compare_launches"] == c0, launch.name           # no second trip
    assert rows is not None and rows.shape == (len(ref), 2), launch.name
    print(launch.name, "rows", [("%08x" % a, int(b)) for a, b in rows.tolist()])
    bad = np.flatnonzero((rows != want).any(axis=1))
    assert len(bad) == 0, (launch.name, "query %d" % bad[0], rows[bad[0]].tolist(), want[bad[0]].tolist())
    assert out.tobytes() == out0.tobytes() and pos.tobytes() == pos0.tobytes(), launch.name
    asm = [q for q in range(len(ref)) if out[q]["assembled"]]
    assert s1["launches"] - s0["launches"] == 1, (launch.name, s0, s1)
    assert s1["sequences"] - s0["sequences"] == len(asm), (launch.name, s0, s1)
    assert s1["pairs"] - s0["pairs"] == sum(len(launch.fam_ids[q]) for q in asm), (launch.name, s0, s1)
    assert s1["kernel_ms"] >= s0["kernel_ms"], launch.name
    again = _reupload_rows(ctx, launch, out, pos)
    assert (again == rows).all(), (launch.name, "the re-upload route differs", again.tolist(), rows.tolist())
    return rows


@pytest.mark.parametrize("name", ic.NAMED)
def test_rows_of_the_named_cases(oracle, holder, name):
    """Family sizes around the four waves, packed family lists, a member without a score, ambiguity codes and case,
    the overhang modes, unassembled queries (two zeros), the widest alignment."""
    for launch, ref in ic.group(name):
        _check_launch(holder, launch, ref)


@pytest.mark.parametrize("name", ("profiles", "wsets"))
def test_rows_through_the_other_entries(oracle, holder, name):
    """sina_hip_align_profiles (--fs-no-graph) and sina_hip_align_families_wsets (a weight vector per query)."""
    for launch, ref in ic.group(name):
        _check_launch(holder, launch, ref)


def test_ranges_and_chunks(oracle, holder, monkeypatch):
    """SINA_HIP_TEST=dp_range_q=3 (four launch ranges), fam_chunk_q=4 (three build chunks; queries 3 and 4 share a
    family across the boundary) and both (five ranges): every row at its query's index, identical to the unforced call."""
    (launch, ref), = ic.group("ranges")
    util.set_knobs(monkeypatch, dp_range_q=None, fam_chunk_q=None)
    whole = _check_launch(holder, launch, ref)
    ctx = holder.hold(launch.refs)
    out0, pos0 = _align(ctx, launch)
    n = len(ref)
    assert n == 10
    for knobs, n_launches in zip(ic.RANGES_KNOBS, (4, 3, 5)):
        util.set_knobs(monkeypatch, dp_range_q=knobs.get("dp_range_q"), fam_chunk_q=knobs.get("fam_chunk_q"))
        ctx.count_identity(True)
        s0 = ctx.identity_inplace_stats()
        out, pos = _align(ctx, launch)
        rows = ctx.staged_identity()
        s1 = ctx.identity_inplace_stats()
        ctx.count_identity(False)
        util.set_knobs(monkeypatch, dp_range_q=None, fam_chunk_q=None)
        assert s1["launches"] - s0["launches"] == n_launches, (knobs, s0, s1)
        assert s1["sequences"] - s0["sequences"] == n and s1["pairs"] - s0["pairs"] == sum(len(f) for f in launch.fam_ids), knobs
        assert (rows == whole).all() and (rows == ic.rows(ref)).all(), (knobs, rows.tolist())
        assert out.tobytes() == out0.tobytes() and pos.tobytes() == pos0.tobytes(), knobs


def test_nothing_counted(oracle):
    """NULL and no launch with the switch off, with assemble = 0, after align_graphs, on a fresh fork; an uncounted call
    after a counted one returns NULL, not the rows before."""
    (launch, ref), = ic.group("shared_family")
    want = ic.rows(ref)
    ctx = capi.Context(0)
    try:
        ctx.upload_refs(launch.refs.ab, launch.refs.off.astype(np.uint64), launch.refs.width)
        zero = ctx.identity_inplace_stats()
        assert zero == dict(kernel_ms=0.0, sequences=0, pairs=0, launches=0)
        assert ctx.staged_identity() is None                         # no align call yet
        _align(ctx, launch)                                          # off
        assert ctx.staged_identity() is None and ctx.identity_inplace_stats() == zero
        ctx.count_identity(True)                                     # on, assemble = 0
        _align(ctx, launch, assemble=0)
        assert ctx.staged_identity() is None and ctx.identity_inplace_stats() == zero
        _align(ctx, launch)                                          # counted ...
        assert (ctx.staged_identity() == want).all()
        one = ctx.identity_inplace_stats()
        assert one["launches"] == 1 and one["sequences"] == len(ref)
        # ... then a graphs entry: no family comes to the device, no stale rows
        cs = util.cseqs_from_refs(launch.refs, launch.fam_ids[0])
        gb = ctx.graph_batch([util.graph_dict(cs)], launch.width)
        qoff = np.array([0, len(launch.qmasks[0])], np.uint64)
        o, _ = ctx.align_graphs(gb, launch.qmasks[0], qoff, ctx.params(assemble=1))
        assert o[0]["status"] == 0 and o[0]["assembled"] == 1
        assert ctx.staged_identity() is None and ctx.identity_inplace_stats() == one
        _align(ctx, launch)
        assert (ctx.staged_identity() == want).all()
        _align(ctx, launch, assemble=0)                              # ... then not: no stale rows
        assert ctx.staged_identity() is None
        fork = ctx.fork()                                            # the parent is on: the fork is not
        try:
            assert fork.staged_identity() is None
            _align(fork, launch)
            assert fork.staged_identity() is None and fork.identity_inplace_stats() == zero
            fork.count_identity(True)
            _align(fork, launch)
            assert (fork.staged_identity() == want).all()
        finally:
            fork.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------- through the stages (the world of tests/test_gpu_pipeline.py)

FF = {"fs-min-len": 100, "fs-full-len": 250}
OFF = dict(fs_min_len=100, fs_full_len=250)


def _join(a, b):
    return synth.QuerySet(mask=np.concatenate([a.mask[:int(a.off[a.n])], b.mask[:int(b.off[b.n])]]),
                          off=np.concatenate([a.off[:a.n + 1], a.off[a.n] + b.off[1:b.n + 1]]).astype(np.int64),
                          src=np.concatenate([a.src, b.src]))


@pytest.fixture(scope="module")
def stage_world(oracle):
    """test_pipeline_calc_idty's queries in one set: 20 mutated ones, 6 exact copies (the copy shortcut), 8 with junk
    spliced in (the host finishes those)."""
    refs = synth.make_refs(500, length=320, width=3200, seed=51, amb_rate=0.01, lower_rate=0.02)
    cs = util.cseqs_from_refs(refs)
    idx = oracle.Index(cs, k=10)
    some = synth.make_queries(refs, 20, seed=58, amb_rate=0.01, lower_rate=0.05)
    exact = synth.make_queries(refs, 6, seed=59, sub=0.0, dele=0.0, ins=0.0)
    more = synth.make_queries(refs, 8, seed=60)
    rng = np.random.default_rng(61)
    parts = []
    for i in range(more.n):
        m = more.seq(i)
        parts.append(np.concatenate([m[:150], rng.choice([1, 2, 4, 8], size=25).astype(np.uint8), m[150:]]))
    off = np.zeros(more.n + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in parts])
    spliced = synth.QuerySet(mask=np.concatenate(parts), off=off, src=more.src)
    qs = _join(_join(some, exact), spliced)
    want = [gp._oracle_run(oracle, cs, idx, qs, qi, OFF) for qi in range(qs.n)]
    st = pipeline.Store(":mem:gpu-idty", refs)
    yield refs, st, qs, want
    st.close()


def _run(st, qs, aligner, batch=8, single=None):
    pl = pipeline.Pipeline(st, famfinder=FF, aligner=aligner)
    if single is None:
        pl.run(qs.mask, qs.off, batch=batch, inflight=2)
    else:
        failed, err = pl.run_single_trays(qs.mask, qs.off, threads=single, max_batch=single)
        assert not failed.any(), err
    res = [pl.result(q) for q in range(qs.n)]
    pl.close()
    return res


def test_stages_take_the_identity_in_place(stage_world):
    refs, st, qs, want = stage_world
    c0, i0 = st.stats()["compare_launches"], st.identity_inplace_stats()
    plain = _run(st, qs, {"calc-idty": True})
    c1, i1 = st.stats()["compare_launches"], st.identity_inplace_stats()
    got = _run(st, qs, {"calc-idty": True, "device-idty": True})
    c2, i2 = st.stats()["compare_launches"], st.identity_inplace_stats()
    n_dp = n_copy = 0
    for q in range(qs.n):
        a, b, w = plain[q], got[q], want[q]
        assert a["status"] == b["status"] == w["status"] and a["log"] == b["log"], q
        if w["status"] not in (0, 1):
            continue
        assert (a["packed"] == b["packed"]).all() and (b["packed"] == w["packed"]).all(), q
        assert util.f32_bits(b["idty"]) == util.f32_bits(w["idty"]) == util.f32_bits(a["idty"]), (q, b["idty"], w["idty"], a["idty"])
        n_dp += w["status"] == 0
        n_copy += w["status"] == 1
        if w["status"] == 1:
            assert b["idty"] == 100
    assert n_dp >= 24 and n_copy >= 5
    assert i1 == i0                                                  # option off: nothing in place
    trays = i2["trays"] - i1["trays"]
    print("in place %d trays of %d DP trays; compare launches %d without, %d with the option" % (trays, n_dp, c1 - c0, c2 - c1))
    assert 0 < trays <= n_dp and 2 * trays >= n_dp
    assert i2["sequences"] - i1["sequences"] == trays                # (distinct queries: one assembled slot per tray)
    assert i2["launches"] - i1["launches"] >= 1 and i2["pairs"] - i1["pairs"] >= trays
    assert c2 - c1 < c1 - c0                                         # fewer second trips
    assert trays < n_dp                                              # (the spliced queries: host-finished, the old route)


def test_device_idty_alone_launches_nothing(stage_world):
    refs, st, qs, want = stage_world
    c0, i0 = st.stats()["compare_launches"], st.identity_inplace_stats()
    got = _run(st, qs, {"device-idty": True})
    assert all(r["idty"] == -1 for r in got)
    assert st.stats()["compare_launches"] == c0 and st.identity_inplace_stats() == i0


def test_trays_of_one_slot_share_their_row(stage_world):
    """Every query twice in one batch: the device sees each once (host dedup), both trays take the slot's row."""
    refs, st, qs, want = stage_world
    n = 16
    first = synth.pick_queries(qs, list(range(n)))
    twice = synth.pick_queries(qs, list(range(n)) + list(range(n)))
    i0 = st.identity_inplace_stats()
    got = _run(st, twice, {"calc-idty": True, "device-idty": True}, batch=32)
    i1 = st.identity_inplace_stats()
    assert first.n == n
    for q in range(n):
        a, b = got[q], got[n + q]
        assert a["status"] == b["status"] == 0 and (a["packed"] == b["packed"]).all()
        assert util.f32_bits(a["idty"]) == util.f32_bits(b["idty"]) == util.f32_bits(want[q]["idty"]), q
    trays, slots = i1["trays"] - i0["trays"], i1["sequences"] - i0["sequences"]
    assert trays == 2 * slots and slots >= n // 2


def test_single_trays_give_the_same_values(stage_world):
    refs, st, qs, want = stage_world
    i0 = st.identity_inplace_stats()
    for threads in (8, 1):
        got = _run(st, qs, {"calc-idty": True, "device-idty": True}, single=threads)
        for q in range(qs.n):
            if want[q]["status"] in (0, 1):
                assert got[q]["status"] == want[q]["status"], q
                assert util.f32_bits(got[q]["idty"]) == util.f32_bits(want[q]["idty"]), (threads, q)
    assert st.identity_inplace_stats()["trays"] > i0["trays"]


def _fasta_records(path):
    recs = []
    for line in open(path).read().splitlines():
        if line.startswith(">"):
            recs.append([line[1:].split()[0], {}, ""])
        elif line.startswith(";"):
            k, _, v = line[1:].strip().partition("=")
            recs[-1][1][k] = v
        else:
            recs[-1][2] += line
    return recs


def test_run_fasta_with_min_idty_writes_the_same_records(stage_world, tmp_path):
    refs, st, qs, want = stage_world
    src = str(tmp_path / "in.fasta")
    with open(src, "w") as f:
        for q in range(qs.n):
            f.write(">q%d\n%s\n" % (q, synth.bases_string(qs.seq(q))))
    idtys = sorted(float(w["idty"]) for w in want if w["status"] in (0, 1))
    cut = idtys[len(idtys) // 3]                                     # a third of the records fall below it
    runs = {}
    for on in (0, 1):
        dst = str(tmp_path / ("out%d.fasta" % on))
        i0 = st.identity_inplace_stats()
        got = pipeline.run_fasta(st, src, dst, famfinder=FF, aligner={"calc-idty": 1, "device-idty": on},
                                 fasta={"meta-fmt": "comment", "min-idty": cut}, batch=16)
        recs = _fasta_records(dst)
        for r in recs:
            r[1].pop("aligned_slv", None)                           # (the date)
        runs[on] = (got, recs, st.identity_inplace_stats()["trays"] - i0["trays"])
    (g0, r0, t0), (g1, r1, t1) = runs[0], runs[1]
    assert r0 == r1 and g0 == g1
    assert 0 < len(r1) < sum(1 for w in want if w["status"] in (0, 1))       # the filter took some and left some
    assert t0 == 0 and t1 > 0
