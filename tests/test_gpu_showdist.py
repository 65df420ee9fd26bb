"""show_dist_kernel and its entry point against tests/showdist_ref.py, word for word: every case of
tests/showdist_cases.py (also cut into launch ranges of 1 and 7 queries), seeded fuzz worlds, the refusals and the
kernel's counters; then the aligner's device-dist in the stages: the FASTA driver of test_fasta_pipeline_and_show_dist_
metrics with the option off and on, with a search stage, the trays that keep the host walk, every other device option
beside it, and the leave-out driver's result(q)["dist"].  tests/test_showdist_cpu.py pins showdist_ref to the oracle and
to the host's show_dist_report, and checks that every case reaches its edge.  All comparisons are exact: the device
returns integers, the floats are the host's own function of them."""
import contextlib
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from sina_amd import capi, pipeline, synth
from tests import compare_cases as cc
from tests import rank_ref
from tests import showdist_cases as sc
from tests import showdist_ref as sr
from tests import util

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _range_knob(n):
    old = os.environ.get("SINA_HIP_TEST")
    if n:
        os.environ["SINA_HIP_TEST"] = "showdist_range=%d" % n
    try:
        yield
    finally:
        if n:
            if old is None:
                del os.environ["SINA_HIP_TEST"]
            else:
                os.environ["SINA_HIP_TEST"] = old


def _upload(ctx, case):
    ctx.upload_refs(cc.flat(case["refs"]), cc.offsets(case["refs"]), case["width"])
    ctx.upload_name_order(rank_ref.name_order(case["names"]))


def _same_rows(got, want, tag):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (tag, "query %d" % bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())


# ---------------------------------------------------------------- rows

@pytest.mark.parametrize("name", sc.NAMES)
def test_rows_of_the_named_cases(gpu_ctx, name):
    case, want = sc.case(name), sc.expected(name)
    _upload(gpu_ctx, case)
    args = sc.flat_call(case)
    nq = len(want)
    before = gpu_ctx.show_dist_stats()
    _same_rows(gpu_ctx.show_dist(*args), want, name)
    after = gpu_ctx.show_dist_stats()
    # the kernel's own counters: every query once, every (query, member) pair once, one launch
    assert after["sequences"] - before["sequences"] == nq
    assert after["pairs"] - before["pairs"] == sum(len(x) for x in case["lists"])
    assert after["launches"] - before["launches"] == 1 and after["kernel_ms"] > before["kernel_ms"]
    for n in (1, 7):
        with _range_knob(n):
            _same_rows(gpu_ctx.show_dist(*args), want, (name, "ranges of %d" % n))
        now = gpu_ctx.show_dist_stats()
        assert now["launches"] - after["launches"] == (nq + n - 1) // n and now["sequences"] - after["sequences"] == nq
        after = now


@pytest.mark.parametrize("seed", sc.FUZZ_SEEDS)
def test_rows_of_fuzz_worlds(gpu_ctx, seed):
    case, want = sc.fuzz(seed)
    _upload(gpu_ctx, case)
    _same_rows(gpu_ctx.show_dist(*sc.flat_call(case)), want, ("fuzz", seed))
    with _range_knob(3):
        _same_rows(gpu_ctx.show_dist(*sc.flat_call(case)), want, ("fuzz", seed, "ranges of 3"))


def test_subrange_of_larger_arrays(gpu_ctx):
    """Offsets that do not start at zero: queries 1 .. 3 of `list_sizes` addressed inside the full arrays."""
    case, want = sc.case("list_sizes"), sc.expected("list_sizes")
    _upload(gpu_ctx, case)
    o_ab, o_off, a_ab, a_off, ids, l_off = sc.flat_call(case)
    rows = np.full((3, 20), 77, np.uint32)
    L = gpu_ctx.L
    p = capi._ptr
    gpu_ctx._check(L.sina_hip_show_dist(gpu_ctx.h, p(o_ab, capi.u32p), p(o_off[1:].copy(), capi.u64p), p(a_ab, capi.u32p),
                                        p(a_off[1:].copy(), capi.u64p), 3, p(ids, capi.u32p), p(l_off[1:].copy(), capi.u64p),
                                        p(rows, capi.u32p)))
    assert o_off[1] != 0 and l_off[2] != 0
    _same_rows(rows, want[1:4], "subrange")


# ---------------------------------------------------------------- refusals

def test_refusals_leave_rows_untouched(gpu_ctx):
    case = sc.case("search_result")
    _upload(gpu_ctx, case)
    o_ab, o_off, a_ab, a_off, ids, l_off = sc.flat_call(case)
    nq = len(o_off) - 1
    rows = np.full((nq, 20), 0xABCD, np.uint32)
    L, h, p = gpu_ctx.L, gpu_ctx.h, capi._ptr

    def call(o_ab=o_ab, o_off=o_off, a_ab=a_ab, a_off=a_off, ids=ids, l_off=l_off, out=rows, n=nq):
        q = lambda x, t: None if x is None else p(x, t)  # noqa: E731
        return L.sina_hip_show_dist(h, q(o_ab, capi.u32p), q(o_off, capi.u64p), q(a_ab, capi.u32p), q(a_off, capi.u64p), n,
                                    q(ids, capi.u32p), q(l_off, capi.u64p), q(out, capi.u32p))

    def refused(rc, text, limit=False):
        assert rc != 0 and text in L.sina_hip_last_error().decode(), L.sina_hip_last_error()
        assert (L.sina_hip_last_error_is_limit() == 1) == limit
        assert (rows == 0xABCD).all()

    for missing in ("o_ab", "o_off", "a_ab", "a_off", "ids", "l_off", "out"):
        refused(call(**{missing: None}), "null argument")
    bad = ids.copy()
    bad[-1] = len(case["refs"])
    refused(call(ids=bad), "reference id out of range")
    for which in ("o_off", "a_off", "l_off"):
        desc = {"o_off": o_off, "a_off": a_off, "l_off": l_off}[which].copy()
        desc[-1] = desc[-2] - 1                     # (the last query ends before it begins: nothing beyond the arrays is read)
        refused(call(**{which: desc}), "offsets descend")
    for which, arr in (("o_ab", o_ab), ("a_ab", a_ab)):
        swapped = arr.copy()
        swapped[[3, 4]] = swapped[[4, 3]]
        refused(call(**{which: swapped}), "columns do not ascend strictly")
        same = arr.copy()
        same[4] = same[3]
        refused(call(**{which: same}), "columns do not ascend strictly")
    long_ab = (np.arange(65536, dtype=np.uint32) | np.uint32(1 << 24))
    long_off = np.array([0, 65536], np.uint64)
    one = np.full((1, 20), 0xABCD, np.uint32)
    short_off = np.array([0, 4], np.uint64)
    rc = call(o_ab=long_ab, o_off=long_off, a_off=short_off, l_off=np.array([0, 2], np.uint64), out=one, n=1)
    refused(rc, "longer than 65535 bases")
    rc = call(a_ab=long_ab, a_off=long_off, o_off=short_off, l_off=np.array([0, 2], np.uint64), out=one, n=1)
    refused(rc, "longer than 65535 bases")
    assert (one == 0xABCD).all()
    # nq == 0 succeeds and touches nothing
    assert call(n=0) == 0 and (rows == 0xABCD).all()
    # no name order: a fresh upload of the references forgets it
    gpu_ctx.upload_refs(cc.flat(case["refs"]), cc.offsets(case["refs"]), case["width"])
    refused(call(), "upload the name order first")
    # a store too wide for the tables: a limit
    gpu_ctx.upload_refs(cc.flat(case["refs"]), cc.offsets(case["refs"]), 900000)
    gpu_ctx.upload_name_order(rank_ref.name_order(case["names"]))
    refused(call(), "too wide", limit=True)
    _upload(gpu_ctx, case)
    _same_rows(gpu_ctx.show_dist(o_ab, o_off, a_ab, a_off, ids, l_off), sc.expected("search_result"), "after the refusals")


# ---------------------------------------------------------------- the FASTA driver

FFO = {"fs-min-len": 100, "fs-full-len": 250, "fs-leave-query-out": True}


def _strip(text):
    """(the aligned_slv time stamp: its line in logs and meta comments)"""
    return re.sub(r"\d\d:\d\d:\d\d", "hh:mm:ss", "\n".join(x for x in text.splitlines() if "aligned_slv" not in x))


def _fasta_run(st, tmp_path, tag, src, aligner, search=None, famfinder=FFO, batch=7):
    dst, logp = str(tmp_path / (tag + ".fasta")), str(tmp_path / (tag + ".log"))
    before = st.show_dist_stats()
    got = pipeline.run_fasta(st, src, dst, famfinder=famfinder, aligner=aligner, search=search, show_dist=True, batch=batch, log_path=logp)
    after = st.show_dist_stats()
    return dict(got=got, fasta=_strip(open(dst).read()), log=_strip(open(logp).read()), trays=after["trays"] - before["trays"],
                sequences=after["sequences"] - before["sequences"], launches=after["launches"] - before["launches"])


def _oracle_averages(refs, cs, idx, pick, search):
    """avg_sps, avg_cpm, avg_idty as the reference's accuracy protocol gives them (test_fasta_pipeline_and_show_dist_metrics)."""
    tot_sps = tot_cpm = tot_idty = 0.0
    for i in pick:
        orig = cs[i]
        ids, _, _ = idx.famfinder(orig, po.ff_opts(fs_min_len=100, fs_full_len=250, fs_leave_query_out=1))
        al = po.align([cs[j] for j in ids], orig, po.align_opts(realign=1))
        assert al["status"] == 0
        aligned = po.Cseq.from_packed("ref%d" % i, al["packed"], al["width"])
        rel = ids
        if search:
            rel, _, _ = po.search(idx, aligned, po.search_opts())
            assert rel is not None and len(rel) > 0
        scored = sorted((float(po.compare(orig, cs[int(j)], "optimistic", "none", "query")), b"ref%d" % j, int(j)) for j in rel)
        before = np.float32(scored[-1][0])
        after = po.compare(aligned, cs[scored[-1][2]], "optimistic", "none", "query")
        tot_sps += float(po.compare(orig, aligned, "exact", "none", "query"))
        tot_idty += float(before)
        tot_cpm += float(np.float32(before - after))
    n = len(pick)
    return tot_sps / n, tot_cpm / n, tot_idty / n


@pytest.fixture(scope="module")
def fasta_world(tmp_path_factory):
    refs = synth.make_refs(300, length=320, width=3200, seed=481, amb_rate=0.01)
    pick = list(range(0, 300, 12))
    src = str(tmp_path_factory.mktemp("showdist") / "in.fasta")
    with open(src, "w") as f:
        for i in pick:
            f.write(">ref%d\n%s\n" % (i, synth.aligned_string(refs.seq(i), refs.width)))
    cs = util.cseqs_from_refs(refs)
    return refs, pick, src, cs, po.Index(cs, k=10)


@pytest.mark.parametrize("search", [None, {}], ids=["family", "search"])
def test_fasta_driver_off_and_on(fasta_world, tmp_path, search):
    refs, pick, src, cs, idx = fasta_world
    st = pipeline.Store(":mem:gpu-showdist-%s" % ("search" if search is not None else "family"), refs)
    try:
        off = _fasta_run(st, tmp_path, "off", src, {"realign": True}, search)
        on = _fasta_run(st, tmp_path, "on", src, {"realign": True, "device-dist": True}, search)
        assert off["got"]["read"] == len(pick) == off["got"]["aligned"]
        assert on["fasta"] == off["fasta"] and on["log"] == off["log"]
        assert "orig_closest_idty: " in off["log"] and off["log"].count("cpm: ") == len(pick)
        for k in ("avg_sps", "avg_cpm", "avg_idty"):
            assert on["got"][k] == off["got"][k], k
        assert on["got"] == off["got"]
        want = _oracle_averages(refs, cs, idx, pick, search is not None)
        assert (off["got"]["avg_sps"], off["got"]["avg_cpm"], off["got"]["avg_idty"]) == want
        assert off["trays"] == 0 and off["sequences"] == 0 and off["launches"] == 0
        assert on["trays"] == on["got"]["aligned"] == on["sequences"] and on["launches"] == (len(pick) + 6) // 7
    finally:
        st.close()


def test_repeated_names_keep_the_host_walk(fasta_world, tmp_path):
    """A store whose names repeat: the closest relative among equals is the sort's business, so every tray walks."""
    refs, pick, src, _, _ = fasta_world
    db = str(tmp_path / "db.fasta")
    with open(db, "w") as f:
        for i in range(refs.n):
            f.write(">%s\n%s\n" % ("twin" if i in (7, 8) else "ref%d" % i, synth.aligned_string(refs.seq(i), refs.width)))
    st = pipeline.Store.open(db)
    try:
        off = _fasta_run(st, tmp_path, "off", src, {"realign": True})
        on = _fasta_run(st, tmp_path, "on", src, {"realign": True, "device-dist": True})
        assert on["fasta"] == off["fasta"] and on["log"] == off["log"] and on["got"] == off["got"]
        assert off["log"].count("cpm: ") == len(pick) and on["trays"] == 0 and on["launches"] == 0
    finally:
        st.close()


def test_a_tray_of_another_width_keeps_its_line(fasta_world, tmp_path):
    refs, pick, _, _, _ = fasta_world
    src = str(tmp_path / "in.fasta")
    with open(src, "w") as f:
        for n, i in enumerate(pick[:9]):
            f.write(">ref%d\n%s%s\n" % (i, synth.aligned_string(refs.seq(i), refs.width), "-----" if n == 4 else ""))
    st = pipeline.Store(":mem:gpu-showdist-width", refs)
    try:
        off = _fasta_run(st, tmp_path, "off", src, {"realign": True})
        on = _fasta_run(st, tmp_path, "on", src, {"realign": True, "device-dist": True})
        assert on["fasta"] == off["fasta"] and on["log"] == off["log"] and on["got"] == off["got"]
        assert off["log"].count("Cannot show dist - ") == 1 and off["log"].count("cpm: ") == 8
        assert on["got"]["aligned"] == 9 and on["trays"] == 8
    finally:
        st.close()


def test_beside_every_other_device_option(fasta_world, tmp_path):
    """device-bps, device-idty, device-shift, device-search and device-dist all on against the run with all of them off."""
    refs, pick, src, _, _ = fasta_world
    st = pipeline.Store(":mem:gpu-showdist-all", refs)
    helix = np.zeros(refs.width, np.uint32)
    cols = np.arange(5, refs.width // 2 - 5)
    helix[cols] = refs.width - 1 - cols
    helix[refs.width - 1 - cols] = cols
    st.set_pairs(helix)
    device = ("device-bps", "device-idty", "device-shift", "device-search", "device-dist")
    try:
        runs = {}
        for on in (False, True):
            al = dict({"realign": True, "calc-idty": 1}, **{k: int(on) for k in device})
            runs[on] = _fasta_run(st, tmp_path, "all-on" if on else "all-off", src, al, search={})
        assert runs[True]["fasta"] == runs[False]["fasta"] and runs[True]["log"] == runs[False]["log"]
        assert runs[True]["got"] == runs[False]["got"] and runs[True]["got"]["avg_bps"] != 0
        assert runs[True]["trays"] == runs[True]["got"]["aligned"] == len(pick) and runs[False]["trays"] == 0
    finally:
        st.close()


# ---------------------------------------------------------------- the leave-out driver's metric

def test_run_aligned_gives_the_metric(fasta_world):
    refs, pick, _, _, _ = fasta_world
    parts = [refs.seq(i) for i in pick]
    q_ab, q_off = cc.flat(parts), cc.offsets(parts)
    names = ["ref%d" % i for i in pick]
    all_refs = [np.asarray(refs.seq(i), np.uint32) for i in range(refs.n)]
    st = pipeline.Store(":mem:gpu-showdist-aligned", refs)
    try:
        dist = {}
        for on in (False, True):
            before = st.show_dist_stats()["trays"]
            pl = pipeline.Pipeline(st, famfinder=FFO, aligner={"realign": True, "device-dist": on}, show_dist=True)
            pl.run_aligned(q_ab, q_off, names, batch=7, inflight=2)
            res = [pl.result(q) for q in range(len(pick))]
            assert all(r["status"] == 0 and r["dist"] is not None for r in res)
            pl.run(np.zeros(4, np.uint8) + 1, np.array([0, 4], np.uint64))
            assert pl.result(0)["dist"] is None                     # run() has no alignment to compare with
            pl.close()
            assert st.show_dist_stats()["trays"] - before == (len(pick) if on else 0)
            dist[on] = res
            plain = pipeline.Pipeline(st, famfinder=FFO, aligner={"realign": True})
            plain.run_aligned(q_ab[:q_off[2]], q_off[:3], names[:2], batch=7, inflight=1)
            assert plain.result(0)["dist"] is None                  # not asked for
            plain.close()
        for q, (a, b) in enumerate(zip(dist[False], dist[True])):
            fam = [int(x) for x in re.findall(r"ref(\d+)\.", a["family"])]
            assert fam and pick[q] not in fam
            want = sr.report(sr.row(parts[q], a["packed"], all_refs, fam, sr.names_of(refs.n)), len(fam))
            for d in (a["dist"], b["dist"]):
                assert isinstance(d["sps"], np.float32) and isinstance(d["idty"], np.float32) and isinstance(d["cpm"], np.float32)
                assert (d["sps"].tobytes(), d["idty"].tobytes(), d["cpm"].tobytes(), d["closest"]) == \
                    (want["sps"].tobytes(), want["idty"].tobytes(), want["cpm"].tobytes(), want["closest"]), (q, d, want)
            assert (a["packed"] == b["packed"]).all()
    finally:
        st.close()
