"""The helix base-pair score (align_bp_score_slv) on the device: sina_hip_pair_counts against the plain restatement of
tests/bps_ref.py on the hand-built cases of tests/bps_cases.py and on seeded random batches; map replacement, buffer
reuse, refusals; and the score through the pipeline, the FASTA drivers and the single-tray shim."""
import os
import re

import numpy as np
import pytest

from sina_amd import capi, pairs, pipeline, synth
from tests import bps_cases as bc
from tests import bps_ref as br

pytestmark = pytest.mark.gpu


def _want(q_ab, q_off, m):
    return np.array([br.counts(s, m) for s in bc.sequences(q_ab, q_off)], np.uint32).reshape(-1, 6)


def _check(ctx, q_ab, q_off, m, what):
    ctx.upload_pairs(m)
    got = ctx.pair_counts(q_ab, q_off)
    want = _want(q_ab, q_off, m)
    assert got.shape == want.shape and (got == want).all(), (what, np.argwhere(got != want)[:5], got[:3], want[:3])


@pytest.mark.parametrize("name", bc.NAMES)
def test_pair_counts_on_cases(gpu_ctx, name):
    q_ab, q_off, m = bc.case(name)
    before = gpu_ctx.pair_stats()
    _check(gpu_ctx, q_ab, q_off, m, name)
    after = gpu_ctx.pair_stats()
    nq = len(q_off) - 1
    assert after["launches"] - before["launches"] == 1 and after["sequences"] - before["sequences"] == nq
    assert after["entries_visited"] - before["entries_visited"] == nq * int(np.count_nonzero(m))


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("seed", range(int(os.environ.get("SINA_FUZZ_SEEDS", "3"))))
def test_pair_counts_on_random_batches(gpu_ctx, seed, symmetric):
    q_ab, q_off, m = bc.random_batch(seed, n=200, width=1000, symmetric=symmetric)
    _check(gpu_ctx, q_ab, q_off, m, ("random", seed, symmetric))


def test_a_second_map_replaces_the_first(gpu_ctx):
    q_ab, q_off, _ = bc.case("table")
    _check(gpu_ctx, q_ab, q_off, bc.TABLE_MAP, "first")
    other = np.zeros(12, np.uint32)
    other[1], other[4] = 4, 8
    _check(gpu_ctx, q_ab, q_off, other, "second")
    assert (gpu_ctx.pair_counts(q_ab, q_off) != _want(q_ab, q_off, bc.TABLE_MAP)).any()
    fork = gpu_ctx.fork()                                   # a forked context sees the store's map ...
    try:
        assert (fork.pair_counts(q_ab, q_off) == _want(q_ab, q_off, other)).all()
        with pytest.raises(capi.SinaHipError, match="forked"):
            fork.upload_pairs(bc.TABLE_MAP)                 # ... and cannot change it
        gpu_ctx.upload_pairs(bc.TABLE_MAP)
        assert (fork.pair_counts(q_ab, q_off) == _want(q_ab, q_off, bc.TABLE_MAP)).all()
    finally:
        fork.close()


def test_buffers_are_reused_across_growing_and_shrinking_calls(gpu_ctx, monkeypatch):
    q_ab, q_off, m = bc.random_batch(7, n=200, width=1000, symmetric=True)
    gpu_ctx.upload_pairs(m)
    want = _want(q_ab, q_off, m)
    for n in (3, 200, 1, 64, 200, 65, 0, 5):
        got = gpu_ctx.pair_counts(q_ab, q_off[:n + 1])
        assert (got == want[:n]).all(), n
    # ... and a call cut into several launch ranges gives what one launch gives
    before = gpu_ctx.pair_stats()["launches"]
    monkeypatch.setenv("SINA_HIP_TEST", "pair_words=2000")
    got = gpu_ctx.pair_counts(q_ab, q_off)
    monkeypatch.delenv("SINA_HIP_TEST")
    assert (got == want).all()
    assert gpu_ctx.pair_stats()["launches"] - before > 5


def test_refusals_launch_nothing(gpu_ctx):
    q_ab, q_off, m = bc.case("table")
    for clear in (np.zeros(0, np.uint32), np.zeros(40, np.uint32)):       # no map: an empty one, an all-zero one
        gpu_ctx.upload_pairs(m)
        gpu_ctx.upload_pairs(clear)
        before = gpu_ctx.pair_stats()
        out = np.full((4, 6), 77, np.uint32)
        with pytest.raises(capi.SinaHipError, match="helix map"):
            gpu_ctx.pair_counts(q_ab, q_off, out=out)
        assert (out == 77).all() and gpu_ctx.pair_stats() == before
    gpu_ctx.upload_pairs(m)
    before = gpu_ctx.pair_stats()
    bad = q_ab.copy()
    bad[int(q_off[1]) + 2], bad[int(q_off[1]) + 3] = bad[int(q_off[1]) + 3], bad[int(q_off[1]) + 2]   # columns descend
    out = np.full((4, 6), 77, np.uint32)
    with pytest.raises(capi.SinaHipError, match="descend"):
        gpu_ctx.pair_counts(bad, q_off, out=out)
    assert (out == 77).all() and gpu_ctx.pair_stats() == before
    assert not gpu_ctx.last_error_is_limit()
    # nq == 0 succeeds and touches nothing
    got = gpu_ctx.pair_counts(q_ab, q_off[:1], out=out[:0])
    assert got.shape == (0, 6) and (out == 77).all() and gpu_ctx.pair_stats() == before


# ---------------------------------------------------------------- through the stages

FF = {"fs-min-len": 100, "fs-full-len": 250}


def _bracket_line(width, n_pairs, seed):
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.choice(np.arange(1, width), size=2 * n_pairs + 4, replace=False))
    text = ["."] * width
    inner = cols[2:-2]
    for k in range(n_pairs):
        text[int(inner[k])], text[int(inner[2 * n_pairs - 1 - k])] = "(", ")"
    text[int(cols[0])], text[int(cols[-2])] = "<", ">"      # a second kind, crossing the first
    text[int(cols[1])], text[int(cols[-1])] = "[", "]"
    return "".join(text)


@pytest.fixture(scope="module")
def world():
    refs = synth.make_refs(500, length=320, width=3200, seed=51, amb_rate=0.01, lower_rate=0.02)
    st = pipeline.Store(":mem:gpu-bps", refs)
    some = synth.make_queries(refs, 63, seed=3052, amb_rate=0.01, lower_rate=0.05, ins=0.01, dele=0.01)
    exact = synth.make_queries(refs, 1, seed=3059, sub=0.0, dele=0.0, ins=0.0)
    mask = np.concatenate([some.mask[:int(some.off[some.n])], exact.mask[:int(exact.off[1])]])
    off = np.concatenate([some.off[:some.n + 1], some.off[some.n] + exact.off[1:2]]).astype(np.uint64)
    helix = pairs.pairs_from_brackets(_bracket_line(refs.width, 300, 77))
    yield refs, st, mask, off, helix
    st.close()


def _expect(packed, helix):
    sc = br.score(br.counts(packed, helix))
    return sc, br.attr(sc)


def test_pipeline_scores_every_aligned_query(world):
    refs, st, mask, off, helix = world
    nq = len(off) - 1
    assert nq == 64
    st.set_pairs(helix)
    try:
        before = st.pair_stats()
        pl = pipeline.Pipeline(st, famfinder=FF)
        pl.run(mask, off, batch=16, inflight=2)
        n_dp = n_copy = nonzero = 0
        for q in range(nq):
            r = pl.result(q)
            if r["status"] == 2:
                assert r["bp_score"] == 0 and r["bps"] == 0
                continue
            n_dp += r["status"] == 0
            n_copy += r["status"] == 1
            sc, attr = _expect(r["packed"], helix)
            assert br.bits(r["bps"]) == br.bits(sc) and r["bp_score"] == attr, (q, r["bps"], sc)
            nonzero += attr != 0
        pl.close()
        assert n_dp >= 55 and n_copy >= 1 and nonzero >= 55
        after = st.pair_stats()
        assert after["launches"] - before["launches"] == 4          # one per batch
        assert after["sequences"] - before["sequences"] == n_dp + n_copy
    finally:
        st.set_pairs(np.zeros(0, np.uint32))


def test_pipeline_without_a_map_launches_nothing(world):
    refs, st, mask, off, helix = world
    before = st.pair_stats()
    pl = pipeline.Pipeline(st, famfinder=FF)
    pl.run(mask, off, batch=16, inflight=2)
    for q in range(len(off) - 1):
        r = pl.result(q)
        assert r["bp_score"] == 0 and r["bps"] == 0
    pl.close()
    assert st.pair_stats() == before


def test_single_trays_take_the_host_walk(world):
    refs, st, mask, off, helix = world
    nq = 24
    st.set_pairs(helix)
    try:
        pl = pipeline.Pipeline(st, famfinder=FF)
        pl.run(mask, off[:nq + 1], batch=8, inflight=1)
        batch = [(pl.result(q)["status"], pl.result(q)["bp_score"], br.bits(pl.result(q)["bps"])) for q in range(nq)]
        before = st.pair_stats()
        failed, err = pl.run_single_trays(mask, off[:nq + 1], threads=8, max_batch=8)
        assert not failed.any(), err
        single = [(pl.result(q)["status"], pl.result(q)["bp_score"], br.bits(pl.result(q)["bps"])) for q in range(nq)]
        assert single == batch and sum(1 for s in single if s[1] != 0) >= 20
        for q in range(nq):
            r = pl.result(q)
            if r["status"] != 2:
                assert r["bp_score"] == _expect(r["packed"], helix)[1]
        assert st.pair_stats() == before                            # no launch: the host walk
        pl.close()
    finally:
        st.set_pairs(np.zeros(0, np.uint32))


def _fasta_records(path):
    """[(name, {key: value} of the '; key=value' lines, sequence text)]"""
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


@pytest.mark.parametrize("serial", [False, True])
def test_run_fasta_writes_the_score(world, tmp_path, serial):
    refs, st, mask, off, helix = world
    nq = 40
    src, dst, logp = str(tmp_path / "in.fasta"), str(tmp_path / "out.fasta"), str(tmp_path / "log.txt")
    with open(src, "w") as f:
        for q in range(nq):
            f.write(">q%d\n%s\n" % (q, synth.bases_string(mask[int(off[q]):int(off[q + 1])])))
    st.set_pairs(helix)
    try:
        before = st.pair_stats()
        got = pipeline.run_fasta(st, src, dst, famfinder=FF, fasta={"meta-fmt": "comment"}, batch=16, log_path=logp,
                                 serial=serial)
        after = st.pair_stats()
    finally:
        st.set_pairs(np.zeros(0, np.uint32))
    recs = _fasta_records(dst)
    assert got["read"] == nq and got["written"] == len(recs) == got["aligned"] and len(recs) >= 35
    total, attrs = 0.0, []
    for name, meta, text in recs:
        sc, attr = _expect(bc.words_of(text), helix)
        assert int(meta["align_bp_score_slv"]) == attr, name
        attrs.append(attr)
        total += float(sc)                                          # (a double sum of the float scores, in tray order)
    assert sum(1 for a in attrs if a != 0) >= 30
    assert [int(v) for v in re.findall(r"^align_bp_score_slv: (-?\d+)$", open(logp).read(), re.M)] == attrs
    assert got["avg_bps"] == total / len(recs)
    assert after["launches"] - before["launches"] == 3              # batches of 16, 16 and 8
    # ... and with no map: today's zeros
    got = pipeline.run_fasta(st, src, dst, famfinder=FF, fasta={"meta-fmt": "comment"}, batch=16, log_path=logp, serial=serial)
    assert got["avg_bps"] == 0.0 and all(int(m["align_bp_score_slv"]) == 0 for _, m, _ in _fasta_records(dst))
    assert st.pair_stats() == after
