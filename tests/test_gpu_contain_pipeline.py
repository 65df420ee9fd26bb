"""The aligner's device-copy in the stages: the exact-relative test of a batch answered by one sina_hip_find_bases call
instead of the host's substring searches.  The world, the queries and the floors are those of
tests/test_gpu_pipeline.py's test_pipeline_copy_shortcut_and_realign and
test_pipeline_exact_relatives_among_mutated_queries; every tray with the option on is the tray with it off -- sequence
and case bits, head, tail, quality, family, identity, the whole log -- and both are the oracle's: plain, under realign,
with every other device option on, through the FASTA driver byte for byte, and when the device call is refused (the
host walk is kept, silently).  A batch of mutated queries launches nothing."""
import re

import numpy as np
import pytest

from sina_amd import pipeline, synth
from tests import util

pytestmark = pytest.mark.gpu

FF = {"fs-min-len": 100, "fs-full-len": 250}
ORACLE_FF = dict(fs_min_len=100, fs_full_len=250)
FF_SHORT = {"fs-min-len": 40, "fs-full-len": 250}
ORACLE_FF_SHORT = dict(fs_min_len=40, fs_full_len=250)


@pytest.fixture(scope="module")
def world(oracle):
    refs = synth.make_refs(500, length=320, width=3200, seed=51, amb_rate=0.01, lower_rate=0.02)
    cs = util.cseqs_from_refs(refs)
    idx = oracle.Index(cs, k=10)
    st = pipeline.Store(":mem:gpu-contain", refs)
    yield refs, cs, idx, st
    st.close()


@pytest.fixture(scope="module")
def queries(world):
    refs = world[0]
    exact = synth.make_queries(refs, 16, seed=54, sub=0.0, dele=0.0, ins=0.0)
    half = synth.make_queries(refs, 16, seed=54, sub=0.0, dele=0.0, ins=0.0, window=(0.25, 150))
    full = synth.make_queries(refs, 60, seed=91, sub=[0.0, 0.03, 0.03], dele=[0.0, 0.005, 0.005], ins=[0.0, 0.003, 0.003])
    wins = synth.make_queries(refs, 60, seed=92, sub=[0.03, 0.0, 0.03], dele=[0.005, 0.0, 0.005], ins=[0.003, 0.0, 0.003],
                              window=(0.3, 60))
    # (name, queries, famfinder options, the oracle's, batch, the floor of copied trays the existing tests assert)
    return {"exact": (exact, FF, ORACLE_FF, 0, 12), "half": (half, FF, ORACLE_FF, 0, 12),
            "full": (full, FF_SHORT, ORACLE_FF_SHORT, 32, 18), "wins": (wins, FF_SHORT, ORACLE_FF_SHORT, 32, 15)}


def _tray(pl, q):
    r = pl.result(q)
    d = dict(r)
    d["packed"] = r["packed"].tobytes()
    d["idty"], d["bps"] = int(util.f32_bits(r["idty"])), int(util.f32_bits(r["bps"]))
    if r.get("search_ids") is not None:
        d["search_ids"] = r["search_ids"].tolist()
        d["search_scores"] = util.f32_bits(r["search_scores"]).tolist()
    return d


def _run(st, qs, ff, al, batch, search=None, check=None):
    before = st.copy_stats()
    pl = pipeline.Pipeline(st, famfinder=ff, aligner=al, search=search)
    try:
        pl.run(qs.mask, qs.off, batch=batch, inflight=2)
        trays = [_tray(pl, q) for q in range(qs.n)]
        if check is not None:
            check(pl)
    finally:
        pl.close()
    after = st.copy_stats()
    return trays, {k: after[k] - before[k] for k in after}


def _same_trays(off, on, tag):
    assert len(off) == len(on)
    for q, (a, b) in enumerate(zip(off, on)):
        assert sorted(a) == sorted(b), (tag, q)
        for k in a:
            assert a[k] == b[k], (tag, "query %d" % q, k, a[k], b[k])


def _strip(text):
    """(the aligned_slv time stamp: its line in logs and meta comments)"""
    return re.sub(r"\d\d:\d\d:\d\d", "hh:mm:ss", "\n".join(x for x in text.splitlines() if "aligned_slv" not in x))


def _idle(d, tag):
    assert d["pairs"] == 0 and d["launches"] == 0 and d["trays"] == 0 and d["fallback_trays"] == 0, (tag, d)


@pytest.mark.parametrize("which", ("exact", "half", "full", "wins"))
@pytest.mark.parametrize("realign", (False, True))
def test_trays_are_the_same_off_and_on(oracle, world, queries, which, realign):
    refs, cs, idx, st = world
    qs, ff, off_ff, batch, floor = queries[which]
    al = {"realign": True} if realign else {}
    n_dp = []
    check = lambda pl: n_dp.append(util.check_trays(oracle, qs, pl, cs, idx, off_ff, dict(realign=1) if realign else None))  # noqa: E731
    off, d_off = _run(st, qs, ff, al, batch, check=check)
    on, d_on = _run(st, qs, ff, dict(al, **{"device-copy": 1}), batch, check=check)
    _same_trays(off, on, (which, realign))
    _idle(d_off, (which, "off"))
    print(which, "realign" if realign else "plain", d_on, "dp", n_dp)
    assert n_dp[0] == n_dp[1]
    copied = sum(t["status"] == 1 for t in on)
    if realign:
        assert copied == 0 and any("containing exact candidate removed from family" in t["log"] for t in on)
    else:
        assert copied >= floor and copied == qs.n - n_dp[1] - sum(t["status"] == 2 for t in on)
        assert all("copied alignment from" in t["log"] for t in on if t["status"] == 1)
    assert d_on["pairs"] > 0 and d_on["launches"] >= 1 and d_on["fallback_trays"] == 0 and d_on["kernel_ms"] > 0
    assert floor <= d_on["trays"] <= qs.n and d_on["pairs"] >= d_on["trays"]


def test_the_same_with_every_other_device_option_on(oracle, world, queries):
    """device-msc and device-cascade on famfinder, device-bps, device-idty, device-shift and device-search on the aligner,
    device-rank on the search stage, a helix map and calc-idty: with them all on, device-copy off and on."""
    refs, cs, idx, st = world
    qs, ff, off_ff, batch, floor = queries["wins"]
    helix = np.zeros(refs.width, np.uint32)          # (neighbouring base columns of reference 0, two by two)
    cols = (refs.ab[int(refs.off[0]):int(refs.off[1])] & 0xFFFFFF)[1:]      # (not column 0: a partner of 0 says unpaired)
    n_pairs = len(cols) // 2
    a, b = cols[0:2 * n_pairs:2], cols[1:2 * n_pairs:2]
    helix[a], helix[b] = b, a
    st.set_pairs(helix)
    try:
        ff_on = dict(ff, **{"device-msc": 1, "device-cascade": 1})
        al_on = {"calc-idty": 1, "device-bps": 1, "device-idty": 1, "device-shift": 1, "device-search": 1}
        search = {"search-max-result": 7, "device-rank": True}
        n_dp = []
        check = lambda pl: n_dp.append(util.check_trays(oracle, qs, pl, cs, idx, off_ff))  # noqa: E731
        plain, _ = _run(st, qs, ff, {"calc-idty": 1}, batch, search={"search-max-result": 7}, check=check)
        off, d_off = _run(st, qs, ff_on, al_on, batch, search=search, check=check)
        on, d_on = _run(st, qs, ff_on, dict(al_on, **{"device-copy": 1}), batch, search=search, check=check)
        _same_trays(plain, off, "host paths against every device option")
        _same_trays(off, on, "every device option, device-copy off and on")
        _idle(d_off, "off")
        assert sum(t["status"] == 1 for t in on) >= floor and n_dp[0] == n_dp[1] == n_dp[2] >= 20
        assert d_on["pairs"] > 0 and d_on["fallback_trays"] == 0 and d_on["trays"] >= floor
        print("bp_score", [t["bp_score"] for t in on][:12], "searched", sum(t.get("search_ids") is not None for t in on))
        assert any(t["bp_score"] != 0 for t in on)
        assert all(t.get("search_ids") is not None for t in on if t["status"] != 2) and any(t.get("search_ids") for t in on)
    finally:
        st.set_pairs(np.zeros(0, np.uint32))


def test_run_fasta_writes_the_same_file(world, queries, tmp_path):
    refs, cs, idx, st = world
    qs, ff, _, _, floor = queries["wins"]
    src = str(tmp_path / "in.fasta")
    with open(src, "w") as f:
        for q in range(qs.n):
            f.write(">q%d\n%s\n" % (q, synth.bases_string(qs.seq(q))))
    runs = {}
    for on in (False, True):
        dst, log = str(tmp_path / ("out%d.fasta" % on)), str(tmp_path / ("log%d.txt" % on))
        before = st.copy_stats()
        got = pipeline.run_fasta(st, src, dst, famfinder=ff, aligner={"device-copy": int(on)}, fasta={"meta-fmt": "comment"},
                                 log_path=log, batch=16)
        after = st.copy_stats()
        runs[on] = (got, _strip(open(dst).read()), _strip(open(log).read()), {k: after[k] - before[k] for k in after})
    assert runs[False][0] == runs[True][0] and runs[False][1] == runs[True][1] and runs[False][2] == runs[True][2]
    assert runs[True][1].count("\n") > 2 * qs.n
    assert (runs[True][1] + runs[True][2]).count("copied alignment from") >= floor
    _idle(runs[False][3], "run_fasta off")
    assert runs[True][3]["pairs"] > 0 and runs[True][3]["fallback_trays"] == 0 and runs[True][3]["trays"] >= floor


def test_mutated_queries_launch_nothing(world):
    """The score prefilter leaves no suspect of a mutated query: no call, no launch, no tray counted."""
    refs, cs, idx, st = world
    qs = synth.make_queries(refs, 40, seed=52, amb_rate=0.01, lower_rate=0.05)
    off, _ = _run(st, qs, FF, {}, 16)
    on, d = _run(st, qs, FF, {"device-copy": 1}, 16)
    _same_trays(off, on, "mutated")
    assert all(t["status"] != 1 for t in on) and sum(t["status"] == 0 for t in on) >= 35
    _idle(d, "mutated")


def test_a_refused_call_keeps_the_host_walk(oracle, world, queries, monkeypatch):
    """SINA_HIP_TEST=contain_fail=1 makes sina_hip_find_bases refuse: no error of the batch, the trays are the host
    walk's and are counted as fallen back."""
    refs, cs, idx, st = world
    qs, ff, off_ff, batch, floor = queries["wins"]
    off, _ = _run(st, qs, ff, {}, batch)
    util.set_knobs(monkeypatch, contain_fail=1)
    n_dp = []
    on, d = _run(st, qs, ff, {"device-copy": 1}, batch,
                 check=lambda pl: n_dp.append(util.check_trays(oracle, qs, pl, cs, idx, off_ff)))
    util.set_knobs(monkeypatch, contain_fail=None)
    _same_trays(off, on, "refused")
    print("refused", d)
    assert d["pairs"] == 0 and d["launches"] == 0 and d["trays"] == 0 and d["fallback_trays"] >= floor
    assert sum(t["status"] == 1 for t in on) >= floor and n_dp[0] >= 20
