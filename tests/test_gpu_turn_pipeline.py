"""famfinder's device-turn in the stages: the orientation of a batch chosen by one sina_hip_kmer_topk_turn call instead
of the host's variants and their searches.  The shape is tests/test_gpu_scale.py's test_turn_orientations_equal_oracle:
500 references, 12 queries handed in all four orientations.  Every tray with the option on is the tray with it off --
turn attribute, family, log, alignment -- and both are the oracle's, for turn = none, revcomp and all: plain (the first
round's rows come with the orientation), with device-cascade and with device-msc under fs-msc-max 0.9 (only the
orientation is taken), through the FASTA driver byte for byte, and when the device call is refused (the host's searches
are kept, silently)."""
import re

import numpy as np
import pytest

from sina_amd import pipeline, synth
from tests import turn_ref as tr
from tests import util

pytestmark = pytest.mark.gpu

FF = {"fs-min-len": 100, "fs-full-len": 250}
MODES = (("none", None), ("revcomp", False), ("all", True))


@pytest.fixture(scope="module")
def world(oracle):
    refs = synth.make_refs(500, length=320, width=3200, seed=51)
    cs = util.cseqs_from_refs(refs)
    idx = oracle.Index(cs, k=10)
    base = synth.make_queries(refs, 12, seed=57)
    masks = [tr.variant(base.seq(qi), qi % 4) for qi in range(base.n)]
    qoff = np.zeros(base.n + 1, np.int64)
    qoff[1:] = np.cumsum([len(m) for m in masks])
    qs = synth.QuerySet(mask=np.concatenate(masks), off=qoff, src=base.src)
    st = pipeline.Store(":mem:gpu-turn", refs)
    yield refs, cs, idx, st, qs
    st.close()


def _tray(pl, q):
    r = pl.result(q)
    d = dict(r)
    d["packed"] = r["packed"].tobytes()
    d["idty"], d["bps"] = int(util.f32_bits(r["idty"])), int(util.f32_bits(r["bps"]))
    d["turn"] = pl.attr(q, "turn")
    return d


def _run(st, qs, ff, check=None):
    before = st.turn_stats()
    pl = pipeline.Pipeline(st, famfinder=ff)
    try:
        pl.run(qs.mask, qs.off, batch=5, inflight=2)
        trays = [_tray(pl, q) for q in range(qs.n)]
        if check is not None:
            check(pl)
    finally:
        pl.close()
    after = st.turn_stats()
    return trays, {k: after[k] - before[k] for k in after}


def _same_trays(off, on, tag):
    assert len(off) == len(on)
    for q, (a, b) in enumerate(zip(off, on)):
        assert sorted(a) == sorted(b), (tag, q)
        for k in a:
            assert a[k] == b[k], (tag, "query %d" % q, k, a[k], b[k])


def _idle(d, tag):
    assert all(d[k] == 0 for k in d), (tag, d)


def _equals_oracle(oracle, world, pl, all_o, ff_opts):
    """Every tray is what the oracle makes of the sequence its own turn_check picks."""
    refs, cs, idx, st, qs = world
    n_turned = 0
    for qi in range(qs.n):
        q = util.query_cseq(qs, qi, upper=False)
        got = pl.result(qi)
        if all_o is None:
            assert pl.attr(qi, "turn") == "turn-check disabled"
            o = 0
        else:
            o, sc4 = idx.turn_check(q, all_o)
            assert pl.attr(qi, "turn") == oracle.Index.TURN_NAMES[o], (qi, sc4)
            if all_o:
                assert o == qi % 4
            n_turned += o != 0
        if o & 1:
            oracle.lib().so_cseq_reverse(q.h)
        if o & 2:
            oracle.lib().so_cseq_complement(q.h)
        ids, sc, fflog = idx.famfinder(q, oracle.ff_opts(fs_min_len=100, fs_full_len=250, **ff_opts))
        if len(ids) == 0:
            assert got["status"] == 2 and got["log"] == fflog
            continue
        want = oracle.align([cs[i] for i in ids], q, oracle.align_opts())
        assert got["family"] == "".join("ref%d.0:%.2f " % (i, s) for i, s in zip(ids, sc)), qi
        assert got["status"] == want["status"], qi
        assert (got["packed"] == want["packed"]).all(), qi
        assert (got["head"], got["tail"], got["qual"]) == (want["head"], want["tail"], want["qual"])
    if all_o is not None:
        assert n_turned >= (9 if all_o else 3)
    return n_turned


@pytest.mark.parametrize("route", ("plain", "cascade", "msc"))
@pytest.mark.parametrize("mode", MODES, ids=[m for m, _ in MODES])
def test_trays_are_the_same_off_and_on(oracle, world, mode, route):
    refs, cs, idx, st, qs = world
    name, all_o = mode
    extra = {"plain": {}, "cascade": {"device-cascade": 1}, "msc": {"device-msc": 1, "fs-msc-max": 0.9}}[route]
    ff_opts = dict(fs_msc_max=0.9) if route == "msc" else {}
    ff = dict(FF, turn=name, **extra)
    turned = []
    check = lambda pl: turned.append(_equals_oracle(oracle, world, pl, all_o, ff_opts))  # noqa: E731
    off, d_off = _run(st, qs, ff, check=check)
    on, d_on = _run(st, qs, dict(ff, **{"device-turn": 1}), check=check)
    _same_trays(off, on, (name, route))
    _idle(d_off, (name, route, "off"))
    print(name, route, d_on)
    if all_o is None:
        _idle(d_on, (name, route, "turn none"))
        return
    assert d_on["fallback_trays"] == 0 and d_on["kernel_ms"] > 0
    assert d_on["turned"] == turned[1] and 0 < d_on["queries"] <= qs.n                   # (repeated queries go up once)
    if route == "plain":
        assert d_on["rows_trays"] == qs.n and d_on["orient_trays"] == 0
    else:
        assert d_on["rows_trays"] == 0 and d_on["orient_trays"] == qs.n


def _strip(text):
    """(the aligned_slv time stamp: its line in logs and meta comments)"""
    return re.sub(r"\d\d:\d\d:\d\d", "hh:mm:ss", "\n".join(x for x in text.splitlines() if "aligned_slv" not in x))


def test_run_fasta_writes_the_same_file(world, tmp_path):
    refs, cs, idx, st, qs = world
    src = str(tmp_path / "in.fasta")
    with open(src, "w") as f:
        for q in range(qs.n):
            f.write(">q%d\n%s\n" % (q, synth.bases_string(qs.seq(q))))
    runs = {}
    for on in (False, True):
        dst, log = str(tmp_path / ("out%d.fasta" % on)), str(tmp_path / ("log%d.txt" % on))
        before = st.turn_stats()
        got = pipeline.run_fasta(st, src, dst, famfinder=dict(FF, turn="all", **{"device-turn": int(on)}), fasta={"meta-fmt": "comment"},
                                 log_path=log, batch=16)
        after = st.turn_stats()
        runs[on] = (got, _strip(open(dst).read()), _strip(open(log).read()), {k: after[k] - before[k] for k in after})
    assert runs[False][0] == runs[True][0] and runs[False][1] == runs[True][1] and runs[False][2] == runs[True][2]
    assert runs[True][1].count("\n") > 2 * qs.n and "reversed and complemented" in runs[True][1] + runs[True][2]
    _idle(runs[False][3], "run_fasta off")
    assert runs[True][3]["rows_trays"] == qs.n and runs[True][3]["turned"] >= 9 and runs[True][3]["fallback_trays"] == 0


def test_a_refused_call_keeps_the_host_searches(oracle, world, monkeypatch):
    """SINA_HIP_TEST=turn_fail=1 makes sina_hip_kmer_topk_turn refuse: no error of the batch, nothing in a tray's log, the
    trays are the host route's and are counted as fallen back."""
    refs, cs, idx, st, qs = world
    ff = dict(FF, turn="all")
    off, _ = _run(st, qs, ff)
    util.set_knobs(monkeypatch, turn_fail=1)
    turned = []
    on, d = _run(st, qs, dict(ff, **{"device-turn": 1}), check=lambda pl: turned.append(_equals_oracle(oracle, world, pl, True, {})))
    util.set_knobs(monkeypatch, turn_fail=None)
    _same_trays(off, on, "refused")
    print("refused", d)
    assert d["fallback_trays"] == qs.n and d["rows_trays"] == 0 and d["orient_trays"] == 0 and d["queries"] == 0 and d["launches"] == 0
    assert turned[0] >= 9
