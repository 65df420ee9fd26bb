"""A leave-out run end to end (fs-leave-query-out, fs-msc-max 0.9), through Pipeline.run_aligned on the leave-out world of
tests/msc_cases.py, with famfinder's device-msc off (the host walk per candidate) and on (the device's match counts):
status, family, log, alignment and quality of every query are the same, the family holds neither the query itself nor
anything above 0.9, and it is the family the cascade gives when rerun in Python from the device's own ids and scores
with the plain walk's identities.  tests/test_msc_cpu.py asserts on the CPU that these queries must widen their lists
41 -> 410 -> the whole store."""
import numpy as np
import pytest

from sina_amd import capi, pipeline
from tests import compare_cases as cc
from tests import msc_cases as mc

pytestmark = pytest.mark.gpu


def _run(st, ff, batch, copies=1, dedup=True):
    names, seqs, _ = mc.leaveout_queries()
    names, seqs = names * copies, seqs * copies
    pl = pipeline.Pipeline(st, famfinder=ff, dedup=dedup)
    try:
        s0 = st.match_stats()
        pl.run_aligned(cc.flat(seqs), cc.offsets(seqs), names, batch=batch, inflight=1)
        out = [pl.result(q) for q in range(len(names))]
    finally:
        pl.close()
    s1 = st.match_stats()
    return out, {k: s1[k] - s0[k] for k in s1}


def _family_ids(text):
    """'ref12.0:35.00 ref7.0:33.00 ' -> [12, 7]"""
    return [int(item.split(".")[0][3:]) for item in text.split()]


@pytest.fixture(scope="module")
def world():
    refs, dense, clade = mc.leaveout_world()
    st = pipeline.Store(":mem:gpu-leaveout", refs)
    yield st, refs, dense, clade
    st.close()


@pytest.fixture(scope="module")
def runs(world):
    """The four runs every test below looks at: device-msc off and on, one batch and batches of 3."""
    st = world[0]
    names, _, _ = mc.leaveout_queries()
    out = {}
    for on in (0, 1):
        for batch in (len(names), 3):
            out[on, batch] = _run(st, dict(mc.LEAVEOUT_FF, **{"device-msc": on}), batch)
    return out


def test_results_are_the_same_off_and_on(runs):
    names, _, kinds = mc.leaveout_queries()
    base, _ = runs[0, len(names)]
    for key, (got, _) in runs.items():
        for q, (a, b) in enumerate(zip(base, got)):
            tag = (key, q, names[q], kinds[q])
            assert a["status"] == b["status"] and a["family"] == b["family"] and a["log"] == b["log"], tag
            assert a["packed"].tobytes() == b["packed"].tobytes() and a["qual"] == b["qual"], tag
            assert (a["head"], a["tail"], a["width"]) == (b["head"], b["tail"], b["width"]), tag
    assert all(len(r["family"]) for r in base)


def test_the_device_counted_exactly_when_switched_on(runs):
    names, _, _ = mc.leaveout_queries()
    for (on, batch), (_, d) in runs.items():
        if on:
            assert d["pairs"] > 0 and d["launches"] > 0 and d["cand_bases"] > d["pairs"], (on, batch, d)
        else:
            assert d["pairs"] == 0 and d["launches"] == 0, (on, batch, d)


def test_family_is_the_cascades(world, runs):
    """No member is the query itself or above 0.9 by the plain walk, and the family is what the cascade keeps of the
    device's own candidate lists."""
    st, refs, dense, clade = world
    names, seqs, kinds = mc.leaveout_queries()
    sizes = np.diff(refs.off)
    got, _ = runs[1, len(names)]
    ctx = capi.Context(0)
    try:
        ctx.upload_refs(refs.ab, refs.off.astype(np.uint64), refs.width)
        ctx.build_index(10, False)
        for q, (name, ab, kind) in enumerate(zip(names, seqs, kinds)):
            self_id = int(name[3:]) if name.startswith("ref") else -1
            ident = np.array([mc.walk_identity(ab, refs.seq(i)) for i in range(refs.n)], np.float32)
            if kind != "equal_columns":
                assert ident.tobytes() == mc.identities(dense, ab).tobytes()

            def lists(M):
                mask = (ab >> 24).astype(np.uint8)
                ids, sc, n = ctx.kmer_topk_any(mask, np.array([0, len(mask)], np.uint64), M)
                return ids[0, :n[0]], sc[0, :n[0]]

            want = mc.leaveout_cascade(lists, sizes, ident, self_id, refs.n)
            fam = _family_ids(got[q]["family"])
            assert fam == want, (name, kind, fam[:8], want[:8])
            assert self_id not in fam and (ident[fam] <= mc.LO_MSC_MAX).all(), (name, kind)
            if kind != "shifted":
                assert (clade[fam] == 1).all() and len(fam) == mc.LO_FS_MAX
    finally:
        ctx.close()
    # equal bases at other columns: the shifted copy keeps its near relatives, the member it was made from may not
    twin, shifted = got[1], got[kinds.index("shifted")]
    assert names[1] != "shifted" and twin["family"] != shifted["family"]
    assert (clade[_family_ids(shifted["family"])] == 0).all()


def test_nothing_is_launched_without_an_identity_limit(world):
    """fs-msc-max 2 (its default) with device-msc on: no identity is asked for, the search runs through the entry
    without counts."""
    st = world[0]
    ff = dict(mc.LEAVEOUT_FF, **{"fs-msc-max": 2, "device-msc": 1})
    got, d = _run(st, ff, 3)
    assert d["pairs"] == 0 and d["launches"] == 0
    assert all(len(r["family"]) for r in got)


def test_repeated_queries_are_searched_once(world, runs):
    """The query list followed by a second copy of itself, same names, in one batch: every tray is what the single list
    gave -- the shifted query (equal mask bytes at other columns) does not merge with the member it was made from, the
    query with equal columns takes the pass without counts -- with device-msc off and on, the batch's repeats grouped
    and not.  Grouped, the device counts the pairs of the single list; not grouped, twice that: the same set of
    distinct queries is in every escalation round."""
    st = world[0]
    names, seqs, kinds = mc.leaveout_queries()
    assert isinstance(names, list) and isinstance(seqs, list) and {"shifted", "equal_columns"} <= set(kinds)
    base, _ = runs[0, len(names)]
    single = runs[1, len(names)][1]["pairs"]
    assert single > 0
    for on in (0, 1):
        for dedup in (True, False):
            got, d = _run(st, dict(mc.LEAVEOUT_FF, **{"device-msc": on}), 2 * len(names), copies=2, dedup=dedup)
            assert len(got) == 2 * len(names)
            for t, b in enumerate(got):
                a = base[t % len(names)]
                tag = (on, dedup, t, names[t % len(names)], kinds[t % len(names)])
                assert a["status"] == b["status"] and a["family"] == b["family"] and a["log"] == b["log"], tag
                assert a["packed"].tobytes() == b["packed"].tobytes() and a["qual"] == b["qual"], tag
                assert (a["head"], a["tail"], a["width"]) == (b["head"], b["tail"], b["width"]), tag
            assert d["pairs"] == (0 if not on else single if dedup else 2 * single), (on, dedup, d, single)
