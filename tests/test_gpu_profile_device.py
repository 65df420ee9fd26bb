"""--fs-no-graph with the family profile built on the device: sina_hip_debug_family_profile against the oracle's pseq +
base_profile::comp, sina_hip_align_profiles against sina_hip_align_graphs fed host-built tables and against
oracle.align(fs_no_graph=1), shared profiles, launch splitting, the pipeline's two routes, the refusals.  Every
comparison is bit for bit."""
import os

import numpy as np
import pytest

from sina_amd import capi, pipeline, synth
from tests import util, walk_cases as wc

pytestmark = pytest.mark.gpu

# More nodes than ANY tile of the build kernel can hold: a node's counters take 12 bytes of a workgroup's 160 KB of LDS
# (the kernel keeps at most 6144 at a time today, include/sina_hip.h: the bound below does not follow that number)
TILE_NODES = 160 * 1024 // 12
# the scheme's arguments (-match_score, -mismatch_score, pen_gap, pen_gapext); the second set is not representable
SCORES = [(-2.0, 1.0, 5.0, 2.0), (-1.7, 0.9, 3.3, 0.7), (-3.0, 2.0, 4.0, 1.5), (-0.7, 0.1, 0.3, 0.1)]


def _refset(seqs, width):
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    ab = np.concatenate(seqs).astype(np.uint32) if len(seqs) else np.zeros(0, np.uint32)
    return synth.RefSet(ab=ab, off=off, width=int(width))


def _trimmed(refs, seed, drop_col0=True):
    """Members that start late and end early; with drop_col0 nobody keeps a base in column 0."""
    rng = np.random.default_rng(seed)
    seqs = []
    for i in range(refs.n):
        s = refs.seq(i)
        lo, hi = int(rng.integers(0, len(s) // 3)), len(s) - int(rng.integers(0, len(s) // 3))
        s = s[lo:hi]
        if drop_col0:
            s = s[(s & 0xFFFFFF) != 0]
        seqs.append(s)
    return _refset(seqs, refs.width)


_oracle_tables = util.profile_oracle_tables   # (shared with test_gpu_graph.py)
_check_hook = util.check_profile_hook


def _uploaded(refs):
    ctx = capi.Context(0)
    ctx.upload_refs(refs.ab, refs.off, refs.width)
    return ctx


@pytest.mark.parametrize("world", ["col0", "no-col0-late-early"])
def test_profile_hook_equals_oracle(oracle, world):
    """Families of 1, 2, 40 and 128 members under four score sets; ambiguity codes and lower case; column 0 occupied
    (every member starts there) and not (members start late and end early)."""
    refs = synth.make_refs(200, length=300, width=3000, seed=43, amb_rate=0.03, lower_rate=0.03, long_del_prob=0.3)
    if world != "col0":
        refs = _trimmed(refs, 7)
    cs = util.cseqs_from_refs(refs)
    col0 = any(len(refs.seq(i)) and (refs.seq(i)[0] & 0xFFFFFF) == 0 for i in range(refs.n))
    assert col0 == (world == "col0")
    rng = np.random.default_rng(2)
    ctx = _uploaded(refs)
    try:
        for scores in SCORES:
            for F in (1, 2, 40, 128):
                ids = rng.choice(refs.n, size=F, replace=False).astype(np.uint32)
                _check_hook(oracle, ctx, cs, ids, scores)
    finally:
        ctx.close()


def test_profile_hook_bases_without_base_bits(oracle):
    """A base whose iupac code has none of the four bits is consumed and changes nothing: neither points nor the
    member's gap state (a gap behind it opens or extends by what came before it)."""
    refs = synth.make_refs(60, length=200, width=800, seed=47, amb_rate=0.03, del_rate=0.08, long_del_prob=0.5)
    rng = np.random.default_rng(3)
    ab = refs.ab.copy()
    ab[rng.random(len(ab)) < 0.15] &= np.uint32(0xF0FFFFFF)
    refs = synth.RefSet(ab=ab, off=refs.off, width=refs.width)
    cs = util.cseqs_from_refs(refs)
    ctx = _uploaded(refs)
    try:
        for F in (5, 40):
            for _ in range(3):
                ids = rng.choice(refs.n, size=F, replace=False).astype(np.uint32)
                o = oracle.pseq_build([cs[int(i)] for i in ids])
                assert np.isfinite(np.asarray(o["prof"], np.float32)).all()   # (no column of such bases alone)
                _check_hook(oracle, ctx, cs, ids, SCORES[1])
    finally:
        ctx.close()


def test_profile_hook_widest_store(oracle):
    """A 524 288-column store: the occupied-column bitmap and its ranks take 96 KB of the workgroup's LDS."""
    refs = synth.make_refs(48, length=1500, width=524288, seed=49, amb_rate=0.01, lower_rate=0.02)
    cs = util.cseqs_from_refs(refs)
    ctx = _uploaded(refs)
    try:
        ids = np.random.default_rng(4).choice(refs.n, size=40, replace=False).astype(np.uint32)
        n = _check_hook(oracle, ctx, cs, ids, SCORES[1])
        assert n > 1500
    finally:
        ctx.close()


def test_profile_hook_more_nodes_than_one_tile(oracle):
    """Dense families of 14 000 and 20 000 columns, more nodes than a workgroup's LDS could hold counters for: several
    sweeps of the tile, every member's cursor moves, gaps that began in an earlier tile extend into the next."""
    for length, F in ((14000, 40), (20000, 6)):
        refs = synth.make_refs(48, length=length, width=2 * length, seed=50, long_del_prob=0.8, amb_rate=0.01)
        cs = util.cseqs_from_refs(refs)
        ctx = _uploaded(refs)
        try:
            ids = np.random.default_rng(5).choice(refs.n, size=F, replace=False).astype(np.uint32)
            n = _check_hook(oracle, ctx, cs, ids, SCORES[1])
            assert n > TILE_NODES
            # ... and a family of the same store that fits one tile, after the long one
            short = _refset([refs.seq(int(i))[:3000] for i in ids], refs.width)
        finally:
            ctx.close()
        ctx = _uploaded(short)
        try:
            n = _check_hook(oracle, ctx, util.cseqs_from_refs(short), np.arange(F, dtype=np.uint32), SCORES[0])
            assert n <= 4096
        finally:
            ctx.close()


def test_profile_of_more_than_65535_nodes_is_refused(oracle):
    refs = synth.make_refs(3, length=70000, width=140000, seed=51, del_rate=0.0, long_del_prob=0.0)
    cs = util.cseqs_from_refs(refs)
    assert oracle.pseq_build([cs[0], cs[1]])["n"] > 65535
    ctx = _uploaded(refs)
    try:
        with pytest.raises(capi.SinaHipError, match="65535"):
            ctx.debug_family_profile(np.array([0, 1], np.uint32), *SCORES[0])
        qm = (refs.seq(2)[:200] >> 24).astype(np.uint8) & 0x0f
        with pytest.raises(capi.SinaHipError, match="65535"):
            ctx.align_profiles(np.array([0, 1], np.uint32), np.array([0, 2], np.uint64), qm, np.array([0, 200], np.uint64))
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", range(int(os.environ.get("SINA_FUZZ_SEEDS", "12"))))
def test_profile_hook_fuzz(oracle, seed):
    """The plane fuzz's worlds and family draws (1 to 60 members, long deletions, ambiguity codes, lower case)."""
    rng, pick, refs, cs, usable = util.fuzz_world(seed)
    ctx = _uploaded(refs)
    try:
        for _ in range(3):
            nfam = int(pick([1, 2, 7, 40, 60]))
            ids = np.asarray(rng.permutation(usable)[:nfam], np.uint32)
            _check_hook(oracle, ctx, cs, ids, SCORES[int(rng.integers(0, len(SCORES)))])
    finally:
        ctx.close()


# ---------------------------------------------------------------- align_profiles against align_graphs and the oracle

def _small_world():
    refs, qs, cs, idx = wc.world_small()
    fam_ids = []
    for qi in range(qs.n):
        ids, _, _ = idx.famfinder(util.query_cseq(qs, qi))
        assert len(ids) > 0
        fam_ids.append(np.asarray(ids, np.uint32))
    return refs, qs, cs, fam_ids


def _both_routes(ctx, width, fams, fam_ids, qmasks, opts, asm):
    """(out, pos) of align_graphs on host-built tables and of align_profiles on the ids, the same launch."""
    tabs = [wc.profile_tables(f, opts) for f in fams]
    gb = ctx.graph_batch([t[0] for t in tabs], width, node_score16=np.concatenate([t[1] for t in tabs]),
                         self_score16=tabs[0][2])
    qoff = np.zeros(len(qmasks) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(m) for m in qmasks])
    qmask = np.concatenate(qmasks)
    foff = np.zeros(len(fam_ids) + 1, np.uint64)
    foff[1:] = np.cumsum([len(f) for f in fam_ids])
    popts = {k: v for k, v in opts.items() if k not in ("fs_no_graph", "weights")}
    want = ctx.align_graphs(gb, qmask, qoff, ctx.params(assemble=asm, **popts))
    got = ctx.align_profiles(np.concatenate(fam_ids), foff, qmask, qoff, ctx.params(assemble=asm, **popts))
    return want, got, qoff


_OPT_SETS = [dict(overhang=oh, lowercase=lc, insertion=(oh + lc) % 2) for oh in (0, 1, 2) for lc in (0, 1, 2)] + \
    [dict(overhang=0, lowercase=2, insertion=1), dict(overhang=1, lowercase=0, insertion=0),
     dict(match_score=1.7, mismatch_score=-0.9, gap_penalty=3.3, gap_ext_penalty=0.7, overhang=2, lowercase=1)]


@pytest.mark.parametrize("geom", [None, "64,8", "128,4"])
@pytest.mark.parametrize("which", range(len(_OPT_SETS)))
def test_align_profiles_equals_align_graphs_and_oracle(oracle, monkeypatch, which, geom):
    """Shift and forbid, the three overhang and the three lowercase modes, assemble 0 and 1, one strip (64 lanes x 8
    columns) and two (128 lanes x 4: strips of 256 columns for queries of ~300 bases): the same bytes as
    align_graphs gives for the host-built tables, and the oracle's alignment."""
    refs, qs, cs, fam_ids = _small_world()
    case = wc.Case("profiles-%d" % which, refs.width, [[cs[int(i)] for i in ids] for ids in fam_ids],
                   [qs.seq(qi) for qi in range(qs.n)], fs_no_graph=1, **_OPT_SETS[which])
    util.set_knobs(monkeypatch, geom=geom)
    ctx = _uploaded(refs)
    try:
        res = {asm: _both_routes(ctx, refs.width, case.fams, fam_ids, case.qmasks, case.opts, asm) for asm in (0, 1)}
    finally:
        ctx.close()
    for asm in (0, 1):
        (wout, wpos), (gout, gpos), qoff = res[asm]
        assert (gout["status"] == 0).all()
        assert gout.tobytes() == wout.tobytes(), (case.name, asm)
        assert (gpos == wpos).all(), (case.name, asm)
    (_, _), (plain, ppos), qoff = res[0]
    (_, _), (fin, fpos), _ = res[1]
    n_asm = 0
    for q in range(len(case.qmasks)):
        om = case.oracle_masks(q)
        qm = case.qmasks[q]                                  # (as given: the aligner upper-cases it unless --lowercase=original)
        qc = oracle.Cseq.from_packed("q%d" % q, np.arange(len(qm), dtype=np.uint32) | (qm.astype(np.uint32) << 24), len(qm))
        want = oracle.align(case.fams[q], qc, oracle.align_opts(realign=1, **case.opts))
        assert want["status"] == 0
        o = plain[q]
        assert (o["cutoff_head"], o["cutoff_tail"]) == (want["head"], want["tail"])
        assert util.f32_bits(np.float32(o["raw"]) / np.float32(o["sum_weight"])) == util.f32_bits(want["score"])
        lo = int(qoff[q])
        packed, _ = util.finish_alignment(om, o, ppos[lo:lo + int(o["n_out"])], refs.width,
                                          lowercase_unaligned=case.opts["lowercase"] == 2, want_packed=True)
        assert packed is not None and (packed == want["packed"]).all(), (case.name, q)
        if fin[q]["assembled"]:
            n_asm += 1
            assert (fpos[lo:lo + int(fin[q]["n_out"])] == want["packed"]).all(), (case.name, q)
    assert n_asm > 0


def _sixteen_s_batch(n_rep):
    refs, qs, cs, idx = wc.world_16s()
    fam_ids, qmasks = [], []
    for rep in range(n_rep):
        for qi in range(qs.n):
            ids, _, _ = idx.famfinder(util.query_cseq(qs, qi))
            fam_ids.append(np.asarray(ids, np.uint32))
            qmasks.append(qs.seq((qi + rep) % qs.n))       # (every repeat pairs the families with other queries)
    return refs, fam_ids, qmasks


def _run_profiles(ctx, fam_ids, qmasks, **kw):
    qoff = np.zeros(len(qmasks) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(m) for m in qmasks])
    foff = np.zeros(len(fam_ids) + 1, np.uint64)
    foff[1:] = np.cumsum([len(f) for f in fam_ids])
    return ctx.align_profiles(np.concatenate(fam_ids), foff, np.concatenate(qmasks), qoff, ctx.params(**kw)), qoff


def test_queries_with_the_same_ordered_family_share_a_profile(oracle):
    """49 queries over a handful of distinct ordered families (one of them a family in another order: a profile of
    its own -- the counts do not care, but the key is the ordered list, like the DAG's): one build per distinct
    family, the results of one query per call."""
    refs, fam_ids, qmasks = _sixteen_s_batch(6)
    fam_ids.append(fam_ids[0][::-1].copy())
    qmasks.append(qmasks[0])
    distinct = len({f.tobytes() for f in fam_ids})
    assert 2 <= distinct < len(fam_ids)
    ctx = _uploaded(refs)
    try:
        s0 = ctx.stats()
        (out, pos), qoff = _run_profiles(ctx, fam_ids, qmasks, assemble=1)
        s1 = ctx.stats()
        assert s1["dags_built"] - s0["dags_built"] == distinct
        assert s1["dags_used"] - s0["dags_used"] == len(qmasks)
        assert s1["graph_launches"] > s0["graph_launches"] and s1["graph_ms"] > s0["graph_ms"]
        assert (out["status"] == 0).all()
        for q in range(len(qmasks)):
            (o1, p1), _ = _run_profiles(ctx, [fam_ids[q]], [qmasks[q]], assemble=1)
            assert o1[0].tobytes() == out[q].tobytes(), q
            assert (p1 == pos[int(qoff[q]):int(qoff[q + 1])]).all(), q
        # (the reversed family's profile is the first one's: the same alignment)
        assert out[-1].tobytes() == out[0].tobytes()
    finally:
        ctx.close()


def test_launch_splitting_under_a_small_traceback_budget(oracle, monkeypatch):
    """The same batch under SINA_HIP_TB_GB=0.25 (a plane holds some thirty of these queries): several DP launches
    over one build, identical bytes."""
    refs, fam_ids, qmasks = _sixteen_s_batch(12)
    distinct = len({f.tobytes() for f in fam_ids})
    runs = []
    for gb in (None, "0.25"):
        if gb:
            monkeypatch.setenv("SINA_HIP_TB_GB", gb)
        else:
            monkeypatch.delenv("SINA_HIP_TB_GB", raising=False)
        ctx = _uploaded(refs)                               # (the budget is decided once per store)
        try:
            s0 = ctx.stats()
            (out, pos), _ = _run_profiles(ctx, fam_ids, qmasks, assemble=1)
            s1 = ctx.stats()
            runs.append((out.tobytes(), pos.tobytes(), s1["dp_launches"] - s0["dp_launches"],
                         s1["dags_built"] - s0["dags_built"]))
            assert (out["status"] == 0).all()
        finally:
            ctx.close()
    assert runs[0][2] == 1 and runs[1][2] >= 2
    assert runs[0][3] == runs[1][3] == distinct
    assert runs[0][:2] == runs[1][:2]


# ---------------------------------------------------------------- the pipeline's two routes

def _oracle_run(oracle, cs, idx, qs, qi, ff, al):
    q = util.query_cseq(qs, qi, upper=False)
    ids, sc, fflog = idx.famfinder(q, oracle.ff_opts(**ff))
    if len(ids) == 0:
        return dict(status=2, log=fflog, ids=ids, sc=sc)
    r = oracle.align([cs[i] for i in ids], q, oracle.align_opts(**al))
    r["log"] = fflog + r["log"]
    r["ids"], r["sc"] = ids, sc
    return r


_TRAY = ("status", "head", "tail", "qual", "width", "log", "family")


@pytest.mark.parametrize("geom", [None, "128,12", "128,4"])
@pytest.mark.parametrize("al,oal", [
    ({}, {}),
    ({"insertion": "forbid", "overhang": "remove"}, dict(insertion=1, overhang=1)),
    ({"lowercase": "unaligned", "overhang": "edge", "pen-gap": 4, "pen-gapext": 1.5, "match-score": 3,
      "mismatch-score": -2}, dict(lowercase=2, overhang=2, gap_penalty=4, gap_ext_penalty=1.5, match_score=3,
                                  mismatch_score=-2)),
])
def test_pipeline_fs_no_graph_device_and_host_routes(oracle, monkeypatch, geom, al, oal):
    """The inputs of test_pipeline_fs_no_graph_profile with the profile built on the device (device-graph and
    device-profile on), on the host (device-graph off; and the default, device-profile off), and on the device through
    the batched shim: trays and logs identical and the oracle's; only the device route builds profiles on the device."""
    refs = synth.make_refs(500, length=320, width=3200, seed=51, amb_rate=0.01, lower_rate=0.02)
    cs = util.cseqs_from_refs(refs)
    idx = oracle.Index(cs, k=10)
    if geom:
        util.set_knobs(monkeypatch, geom=geom)
    qs = synth.make_queries(refs, 24, seed=57, window=(0.3, 120), ins=0.02, dele=0.02, lower_rate=0.05, amb_rate=0.02)
    ff = {"fs-min-len": 100, "fs-full-len": 250}
    st = pipeline.Store(":mem:gpu-profile-routes", refs)
    try:
        trays, built = {}, {}
        for route in ("device", "host", "default", "shim"):
            sw = {"fs-no-graph": True, "device-graph": route != "host"}
            if route != "default":
                sw["device-profile"] = True
            pl = pipeline.Pipeline(st, famfinder=ff, aligner=dict(al, **sw))
            b0 = st.stats()["dags_built"]
            if route == "shim":
                failed, err = pl.run_single_trays(qs.mask, qs.off, threads=8, max_batch=24)
                assert not failed.any(), err
            else:
                pl.run(qs.mask, qs.off, batch=24, inflight=1)
            built[route] = st.stats()["dags_built"] - b0
            trays[route] = [pl.result(qi) for qi in range(qs.n)]
            pl.close()
        assert built["device"] > 0 and built["shim"] > 0 and built["host"] == 0 and built["default"] == 0
        n_dp = 0
        for qi in range(qs.n):
            d = trays["device"][qi]
            for other in ("host", "default", "shim"):
                o = trays[other][qi]
                assert all(d[k] == o[k] for k in _TRAY), (other, qi)
                assert (d["packed"] == o["packed"]).all(), (other, qi)
            want = _oracle_run(oracle, cs, idx, qs, qi, dict(fs_min_len=100, fs_full_len=250), dict(oal, fs_no_graph=1))
            if want["status"] == 2:
                assert d["status"] == 2 and d["log"] == want["log"]
                continue
            assert d["family"] == "".join("ref%d.0:%.2f " % (i, s) for i, s in zip(want["ids"], want["sc"]))
            assert d["status"] == want["status"], (qi, d["log"], want["log"])
            assert (d["packed"] == want["packed"]).all()
            assert (d["head"], d["tail"], d["qual"]) == (want["head"], want["tail"], want["qual"])
            if want["status"] == 0:
                assert d["log"] == want["log"]
                n_dp += 1
        assert n_dp >= 20
    finally:
        st.close()


# ---------------------------------------------------------------- refusals

def test_align_profiles_refusals(oracle):
    refs, qs, cs, fam_ids = _small_world()
    ctx = _uploaded(refs)
    try:
        qm = qs.seq(0)
        qoff = np.array([0, len(qm)], np.uint64)
        one = lambda ids, **kw: ctx.align_profiles(np.asarray(ids, np.uint32), np.array([0, len(ids)], np.uint64), qm,   # noqa: E731
                                                   kw.pop("qoff", qoff), ctx.params(**kw))
        out, _ = one(np.arange(128))
        assert out[0]["status"] == 0
        with pytest.raises(capi.SinaHipError, match="family size"):
            one(np.arange(129))
        with pytest.raises(capi.SinaHipError, match="out of range"):
            one([0, 1, refs.n])
        with pytest.raises(capi.SinaHipError, match="positional weights"):
            ctx.align_profiles(fam_ids[0], np.array([0, len(fam_ids[0])], np.uint64), qm, qoff,
                               ctx.params(weights=np.ones(refs.width, np.float32)))
        with pytest.raises(capi.SinaHipError, match="query length"):
            one(fam_ids[0], qoff=np.array([0, 0], np.uint64))
        out, _ = one(fam_ids[0], fs_weight=123.0)            # (ignored)
        ref, _ = one(fam_ids[0])
        assert out.tobytes() == ref.tobytes()
    finally:
        ctx.close()
    bare = capi.Context(0)
    try:
        with pytest.raises(capi.SinaHipError, match="upload references first"):
            bare.align_profiles(np.array([0], np.uint32), np.array([0, 1], np.uint64), qs.seq(0), np.array([0, len(qs.seq(0))], np.uint64))
    finally:
        bare.close()
