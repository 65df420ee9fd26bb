"""famfinder's device-cascade end to end, through Pipeline.run_aligned on the leave-out world and the queries of
tests/msc_cases.py: with the option on every tray is what the host cascade gives (device-msc off and on, one batch and
batches of 3, repeats grouped and not); the families are the plain loop's (tests/cascade_ref.py) over the device's own
lists; every query but the one with equal columns took the device path; the same bases under two names do not share a
family; default options on a small store; the FASTA driver."""
import numpy as np
import pytest

from sina_amd import capi, pipeline, synth
from tests import cascade_ref as cr
from tests import compare_cases as cc
from tests import msc_cases as mc

pytestmark = pytest.mark.gpu

RULE = cr.Rule(fs_min=mc.LO_FS_MIN, fs_max=mc.LO_FS_MAX, fs_req_full=1, fs_full_len=mc.LO_FULL_LEN, fs_min_len=mc.LO_MIN_LEN,
               fs_cover_gene=0, fs_msc=mc.LO_FS_MSC, fs_msc_max=float(mc.LO_MSC_MAX))


def _run(st, ff, names, seqs, batch, dedup=True):
    pl = pipeline.Pipeline(st, famfinder=ff, dedup=dedup)
    try:
        f0, m0 = st.family_stats(), st.match_stats()
        pl.run_aligned(cc.flat(seqs), cc.offsets(seqs), names, batch=batch, inflight=1)
        out = [pl.result(q) for q in range(len(names))]
    finally:
        pl.close()
    f1, m1 = st.family_stats(), st.match_stats()
    return out, {k: f1[k] - f0[k] for k in f1}, {k: m1[k] - m0[k] for k in m1}


def _same_trays(base, got, tag):
    assert len(base) == len(got)
    for q, (a, b) in enumerate(zip(base, got)):
        t = (tag, q)
        assert a["status"] == b["status"] and a["family"] == b["family"] and a["log"] == b["log"], t
        assert a["packed"].tobytes() == b["packed"].tobytes() and a["qual"] == b["qual"], t
        assert (a["head"], a["tail"], a["width"]) == (b["head"], b["tail"], b["width"]), t


def _family(text):
    """'ref12.0:35.00 ref7.0:33.00 ' -> ([12, 7], [35.0, 33.0])"""
    items = text.split()
    return [int(i.split(".")[0][3:]) for i in items], [float(i.split(":")[1]) for i in items]


@pytest.fixture(scope="module")
def world():
    refs, dense, clade = mc.leaveout_world()
    st = pipeline.Store(":mem:gpu-cascade", refs)
    yield st, refs, dense, clade
    st.close()


@pytest.fixture(scope="module")
def runs(world):
    """device-cascade off and on, each with device-msc off and on, in one batch and in batches of 3."""
    st = world[0]
    names, seqs, _ = mc.leaveout_queries()
    out = {}
    for cascade in (0, 1):
        for msc in (0, 1):
            for batch in (len(names), 3):
                out[cascade, msc, batch] = _run(st, dict(mc.LEAVEOUT_FF, **{"device-cascade": cascade, "device-msc": msc}), names, seqs, batch)
    return out


@pytest.fixture(scope="module")
def plain(world):
    """Per query of the leave-out list: (family ids, family scores, rounds) of the plain loop over the device's own
    lists and match counts; None for the query whose columns do not ascend."""
    st, refs, dense, clade = world
    names, seqs, kinds = mc.leaveout_queries()
    meta = cr.meta_of([refs.seq(i) for i in range(refs.n)])
    ctx = capi.Context(0)
    out = []
    try:
        ctx.upload_refs(refs.ab, refs.off.astype(np.uint64), refs.width)
        ctx.build_index(10, False)
        for name, ab, kind in zip(names, seqs, kinds):
            if kind == "equal_columns":
                out.append(None)
                continue
            selfs = [int(name[3:])] if name.startswith("ref") else []
            match = {}

            def lists(M):
                ids, sc, n, mt = ctx.kmer_topk_match(ab, np.array([0, len(ab)], np.uint64), M)
                match["row"] = mt[0, :n[0]]
                return ids[0, :n[0]], sc[0, :n[0]]

            out.append(cr.escalate(lists, refs.n, RULE, lambda i, s: cr.candidates(meta, i, s, match["row"], len(ab), selfs)))
    finally:
        ctx.close()
    return out


def test_on_equals_off(runs):
    names, _, kinds = mc.leaveout_queries()
    base = runs[0, 0, len(names)][0]
    for key, (got, _, _) in runs.items():
        _same_trays(base, got, key)
    assert all(len(r["family"]) for r in base)


def test_families_are_the_plain_loops(runs, plain):
    names, _, kinds = mc.leaveout_queries()
    for key, (got, _, _) in runs.items():
        for q, want in enumerate(plain):
            if want is None:
                continue
            ids, scores = _family(got[q]["family"])
            assert ids == want[0].tolist() and scores == [float(s) for s in want[1]], (key, names[q], kinds[q])


def test_who_took_the_device_path(runs, plain):
    """With the option on, per escalation round every query still looking -- but the one with equal columns, which
    alone keeps the host path -- is one query of a cascade launch; with it off nothing is launched."""
    names, _, kinds = mc.leaveout_queries()
    assert kinds.count("equal_columns") == 1
    want_queries = sum(len(p[2]) for p in plain if p is not None)
    assert want_queries > 2 * (len(names) - 1)                       # (they escalate)
    for (cascade, msc, batch), (_, f, m) in runs.items():
        if not cascade:
            assert f["queries"] == 0 and f["launches"] == 0, (cascade, msc, batch, f)
            assert (m["launches"] > 0) == bool(msc)
            continue
        assert f["queries"] == want_queries and f["launches"] > 0, (msc, batch, f, want_queries)
        assert f["candidates_scanned"] <= f["candidates_listed"]
        assert m["launches"] == f["launches"] and m["pairs"] == f["candidates_listed"]       # the identity limit: counted in place


def test_repeated_queries(world, runs):
    """The query list twice in one batch, grouped and not: every tray is the single list's; grouped, the device sees the
    single list's queries."""
    st = world[0]
    names, seqs, _ = mc.leaveout_queries()
    base = runs[0, 0, len(names)][0]
    single = runs[1, 0, len(names)][1]["queries"]
    for dedup in (True, False):
        got, f, _ = _run(st, dict(mc.LEAVEOUT_FF, **{"device-cascade": 1}), names * 2, seqs * 2, 2 * len(names), dedup=dedup)
        _same_trays(base + base, got, ("repeats", dedup))
        assert f["queries"] == (single if dedup else 2 * single), (dedup, f, single)


def test_same_bases_under_two_names(world, plain):
    """One batch holds a member's bases under its own name and under a name no reference has: the first family leaves
    the member out, the second has it -- grouped and not."""
    st, refs, dense, clade = world
    names, seqs, kinds = mc.leaveout_queries()
    me = int(names[0][3:])
    own = _run(st, dict(mc.LEAVEOUT_FF, **{"device-cascade": 0}), [names[0], "nobody"], [seqs[0], seqs[0]], 2)[0]
    for dedup in (True, False):
        got, f, _ = _run(st, dict(mc.LEAVEOUT_FF, **{"device-cascade": 1}), [names[0], "nobody"], [seqs[0], seqs[0]], 2, dedup=dedup)
        _same_trays(own, got, ("two names", dedup))
        # (under the other name the member itself is a candidate like any other -- and far above the identity limit)
        for r in got:
            assert _family(r["family"])[0] == plain[0][0].tolist() and me not in _family(r["family"])[0]
        assert f["queries"] >= 2 * 2                                 # two rows per round, also where repeats are grouped
    # without the identity limit the member is its own best relative under the other name only
    ff = dict(mc.LEAVEOUT_FF, **{"fs-msc-max": 2, "device-cascade": 1})
    for dedup in (True, False):
        got, f, m = _run(st, ff, [names[0], "nobody"], [seqs[0], seqs[0]], 2, dedup=dedup)
        off = _run(st, dict(ff, **{"device-cascade": 0}), [names[0], "nobody"], [seqs[0], seqs[0]], 2, dedup=dedup)[0]
        _same_trays(off, got, ("two names, no limit", dedup))
        a, b = _family(got[0]["family"])[0], _family(got[1]["family"])[0]
        assert me not in a and me in b and a != b
        assert f["queries"] == 2 and m["launches"] == 0


def test_defaults_on_a_small_store():
    """Default options (fs-msc-max 2, no leave-out) but the lengths, on a small store: the same trays with the option on
    and off, one cascade query per tray, no match launch."""
    refs = synth.make_refs(400, length=300, width=3000, seed=11, amb_rate=0.01, lower_rate=0.02)
    qs = synth.make_queries(refs, 24, seed=12)
    ff = {"fs-min-len": 100, "fs-full-len": 250}
    st = pipeline.Store(":mem:gpu-cascade-small", refs)
    try:
        out = {}
        for on in (0, 1):
            pl = pipeline.Pipeline(st, famfinder=dict(ff, **{"device-cascade": on}))
            try:
                f0, m0 = st.family_stats(), st.match_stats()
                pl.run(qs.mask, qs.off, batch=10, inflight=1)
                out[on] = [pl.result(q) for q in range(qs.n)]
            finally:
                pl.close()
            f1, m1 = st.family_stats(), st.match_stats()
            assert m1["launches"] == m0["launches"]
            assert (f1["queries"] - f0["queries"] >= qs.n) if on else (f1["queries"] == f0["queries"])
        _same_trays(out[0], out[1], "defaults")
        assert sum(1 for r in out[1] if r["status"] == 0 and len(r["family"])) >= qs.n - 2
    finally:
        st.close()


def test_run_fasta_writes_the_same_file(world, tmp_path):
    st, refs, dense, clade = world
    names, seqs, kinds = mc.leaveout_queries()
    src = str(tmp_path / "in.fasta")
    with open(src, "w") as f:
        for name, ab in zip(names, seqs):
            if (np.diff(cc.cols(ab)) > 0).all():
                f.write(">%s\n%s\n" % (name, synth.aligned_string(ab, refs.width)))
    files = {}
    for on in (0, 1):
        dst = str(tmp_path / ("out%d.fasta" % on))
        f0 = st.family_stats()
        got = pipeline.run_fasta(st, src, dst, famfinder=dict(mc.LEAVEOUT_FF, **{"device-cascade": on}), batch=4)
        files[on] = (open(dst, "rb").read(), got, st.family_stats()["queries"] - f0["queries"])
    assert files[0][0] == files[1][0] and files[0][1] == files[1][1] and len(files[0][0]) > 1000
    assert files[0][2] == 0 and files[1][2] > 0
