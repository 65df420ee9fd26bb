"""The device assembly with shifted insertions (sina_hip_align_params::assemble == 2, assemble_kernel<true>) on the GPU.

  1. sina_hip_debug_assemble runs every hand-built case of tests/shift_cases.py under the three lowercase modes and the
     three overhang modes: `assembled` equals shift_ref.must_assemble_shift exactly; an assembled query's words, shift
     log and three facts are the plain restatement's (tests/test_shift_cpu.py pins that to the oracle and the host); a
     query left alone has its input back.  The same inputs under assemble = 1 give what walk_ref.must_assemble says,
     and the bytes of assemble = 2 where both assemble.
  2. Through the DP: sina_hip_align_families over a store laid out in blocks, under both walks -- words, events and
     totals equal pyoracle.align's, sina_hip_assemble_stats counts what the oracle's logs count.
  3. The in-place pair count and family identity over shifted queries equal sina_hip_pair_counts and sina_hip_compare
     over the same finished words.
"""
import numpy as np
import pytest

from sina_amd import capi
from tests import identity_cases as ic, shift_cases as sc, shift_ref as sr, util, walk_ref

pytestmark = pytest.mark.gpu

_FACTS = ("nast_total", "nast_longest", "nast_last_run")


def _out(o):
    out = np.zeros(1, capi.ALIGN_OUT_DTYPE)
    for k, v in o.items():
        out[0][k] = v
    return out


def _run_case(ctx, case, overhang, lowercase):
    qmask, o = sc.inputs(case, overhang)
    qoff = np.array([0, len(qmask)], np.uint64)
    pos_in = np.zeros(len(qmask), np.uint32)
    pos_in[:case.n] = case.emitted
    want = sr.finish(case.emitted, qmask, o, case.width, overhang, lowercase)
    tag = (case.name, "overhang=%d" % overhang, "lowercase=%d" % lowercase)
    got = {}
    for asm in (2, 1):
        out, pos = ctx.debug_assemble(ctx.params(overhang=overhang, lowercase=lowercase, assemble=asm), case.width, qmask, qoff,
                                      _out(o), pos_in)
        got[asm] = (out[0].copy(), pos[:case.n].copy(), ctx.staged_shift_log())
    a, pos, log = got[2]
    assert int(a["assembled"]) == int(want["must"]), tag + ("assembled", int(a["assembled"]), "must", want["must"])
    assert log is not None and len(log) == 1, tag
    if want["must"]:
        fx = want["fx"]
        bad = np.flatnonzero(pos != want["words"])
        assert len(bad) == 0, tag + ("base %d of %d: %08x, want %08x" % (bad[0], case.n, pos[bad[0]], want["words"][bad[0]]),)
        assert log[0] == fx["events"], tag + (log[0], fx["events"])
        assert tuple(int(a[f]) for f in _FACTS) == (fx["total"], fx["longest"], fx["last_run"]), tag
        cols = pos & 0xFFFFFF
        assert (np.diff(cols.astype(np.int64)) > 0).all() and int(cols[-1]) < case.width, tag   # (what the in-place counts assume)
    else:
        assert (pos == pos_in[:case.n]).all() and log[0] == [], tag
        assert all(int(a[f]) == 0 for f in _FACTS), tag
    # assemble = 1: today's kernel, today's rule
    b, pos1, log1 = got[1]
    facts = walk_ref.container_facts(case.emitted, case.width)
    must1 = walk_ref.must_assemble(case.n, facts)
    assert log1 is None and int(b["assembled"]) == int(must1), tag + ("assemble=1", int(b["assembled"]), must1)
    if must1:
        assert want["must"], tag
        assert b.tobytes() == a.tobytes() and (pos1 == pos).all(), tag
        assert tuple(int(b[f]) for f in _FACTS) == (facts["nast_total"], facts["nast_longest"], facts["nast_last_run"]), tag
    else:
        assert (pos1 == pos_in[:case.n]).all(), tag
    return want["must"], must1


@pytest.mark.parametrize("overhang", (sr.OVERHANG_ATTACH, sr.OVERHANG_REMOVE, sr.OVERHANG_EDGE))
@pytest.mark.parametrize("lowercase", (sr.LOWERCASE_NONE, sr.LOWERCASE_ORIGINAL, sr.LOWERCASE_UNALIGNED))
def test_debug_assemble_cases(gpu_ctx, overhang, lowercase):
    n2 = n1 = 0
    for case in sc.CASES:
        m2, m1 = _run_case(gpu_ctx, case, overhang, lowercase)
        n2 += m2
        n1 += m1
    assert n2 == sum(not c.cap for c in sc.CASES) and 0 < n1 < n2    # (most cases are the new mode's alone)


def test_debug_assemble_many_queries_in_one_launch(gpu_ctx):
    """150 seeded random lists as the queries of one launch (one wave each, lengths 1 to 199), common width."""
    rng = np.random.default_rng(99)
    lists = [sc.random_cols(rng)[0] for _ in range(150)]
    width = max(c[-1] for c in lists) + 2
    qmasks, outs, emitted, wants = [], [], [], []
    for i, cols in enumerate(lists):
        case = sc.Case("random %d" % i, width, cols=cols)
        qm, o = sc.inputs(case, sr.OVERHANG_ATTACH, seed=i)
        qmasks.append(qm)
        outs.append(_out(o))
        emitted.append(np.array(case.emitted, np.uint32))
        wants.append(sr.finish(case.emitted, qm, o, width, sr.OVERHANG_ATTACH, sr.LOWERCASE_UNALIGNED))
    qoff = np.zeros(len(lists) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(m) for m in qmasks])
    out, pos = gpu_ctx.debug_assemble(gpu_ctx.params(lowercase=2, assemble=2), width, np.concatenate(qmasks), qoff,
                                      np.concatenate(outs), np.concatenate(emitted))
    log = gpu_ctx.staged_shift_log()
    n_shift = 0
    for q, w in enumerate(wants):
        got = pos[int(qoff[q]):int(qoff[q + 1])]
        assert int(out[q]["assembled"]) == int(w["must"]), q
        if w["must"]:
            assert (got == w["words"]).all() and log[q] == w["fx"]["events"], q
            assert tuple(int(out[q][f]) for f in _FACTS) == (w["fx"]["total"], w["fx"]["longest"], w["fx"]["last_run"]), q
            n_shift += bool(log[q])
        else:
            assert (got == emitted[q]).all() and log[q] == [], q
    assert n_shift >= 60


def test_debug_assemble_refuses_what_it_cannot_index(gpu_ctx):
    case = sc.BY_NAME["fits"]
    qmask, o = sc.inputs(case, sr.OVERHANG_ATTACH)
    qoff = np.array([0, len(qmask)], np.uint64)
    pos = np.array(case.emitted, np.uint32)
    for bad in (dict(n_out=case.n + 1), dict(end_s=case.n), dict(end_s=0)):
        with pytest.raises(capi.SinaHipError):
            gpu_ctx.debug_assemble(gpu_ctx.params(assemble=2), case.width, qmask, qoff, _out(dict(o, **bad)), pos)
    with pytest.raises(capi.SinaHipError):
        gpu_ctx.debug_assemble(gpu_ctx.params(assemble=0), case.width, qmask, qoff, _out(o), pos)


@pytest.fixture(scope="module")
def dp_ctx(oracle):
    w = sc.dp_world()
    ctx = capi.Context(0)
    ctx.upload_refs(w["refs"].ab, w["refs"].off, w["refs"].width)
    yield ctx, w
    ctx.close()


@pytest.mark.parametrize("lanes", (0, 1))
def test_align_families_equals_the_oracle(dp_ctx, monkeypatch, lanes):
    ctx, w = dp_ctx
    util.set_knobs(monkeypatch, bt_lanes=lanes)
    s0 = ctx.assemble_stats()
    out, pos = ctx.align_families(w["fam_ids"], w["fam_off"], w["qmask"], w["qoff"], ctx.params(lowercase=2, assemble=2))
    log = ctx.staged_shift_log()
    s1 = ctx.assemble_stats()
    want_events = [sc.log_events(r["log"]) for r in w["want"]]
    for q, r in enumerate(w["want"]):
        o = out[q]
        assert o["status"] == 0 and o["assembled"] == 1, q
        got = pos[int(w["qoff"][q]):int(w["qoff"][q]) + int(o["n_out"])]
        assert len(got) == len(r["packed"]) and (got == r["packed"]).all(), q
        assert log[q] == want_events[q], (q, log[q], want_events[q])
        assert tuple(int(o[f]) for f in _FACTS) == sc.log_totals(r["log"]), q
    nq = len(w["want"])
    assert s1["queries"] - s0["queries"] == nq and s1["assembled"] - s0["assembled"] == nq
    assert s1["shifted_queries"] - s0["shifted_queries"] == sum(bool(e) for e in want_events)
    assert s1["shifted_runs"] - s0["shifted_runs"] == sum(len(e) for e in want_events)
    # assemble = 1 leaves the shifted queries to the host, and the others' bytes are the same
    out1, pos1 = ctx.align_families(w["fam_ids"], w["fam_off"], w["qmask"], w["qoff"], ctx.params(lowercase=2, assemble=1))
    assert ctx.staged_shift_log() is None
    assert [int(a) for a in out1["assembled"]] == [int(not e) for e in want_events]
    for q in range(nq):
        if out1[q]["assembled"]:
            assert out1[q].tobytes() == out[q].tobytes(), q
            assert (pos1[int(w["qoff"][q]):int(w["qoff"][q + 1])] == pos[int(w["qoff"][q]):int(w["qoff"][q + 1])]).all(), q


def test_in_place_counts_over_shifted_queries(dp_ctx):
    ctx, w = dp_ctx
    width = w["refs"].width
    helix = np.zeros(width, np.uint32)
    cols = np.arange(5, width // 2 - 5)
    helix[cols] = width - 1 - cols                      # (column i pairs with its mirror image)
    helix[width - 1 - cols] = cols
    ctx.upload_pairs(helix)
    ctx.count_pairs(True)
    ctx.count_identity(True)
    try:
        out, pos = ctx.align_families(w["fam_ids"], w["fam_off"], w["qmask"], w["qoff"], ctx.params(lowercase=2, assemble=2))
        pairs, idty, log = ctx.staged_pair_counts(), ctx.staged_identity(), ctx.staged_shift_log()
    finally:
        ctx.count_pairs(False)
        ctx.count_identity(False)
    assert pairs is not None and idty is not None and (out["assembled"] == 1).all()
    nq = len(out)
    assert sum(bool(e) for e in log) * 2 >= nq
    parts = [pos[int(w["qoff"][q]):int(w["qoff"][q]) + int(out[q]["n_out"])] for q in range(nq)]
    q_off = np.zeros(nq + 1, np.uint64)
    q_off[1:] = np.cumsum([len(p) for p in parts])
    words = np.concatenate(parts).astype(np.uint32)
    again = ctx.pair_counts(words, q_off)
    assert (pairs == again).all() and int(again[:, 0].sum()) > 0
    counts = ctx.compare(words, q_off, w["fam_ids"], w["fam_off"], iupac=0, filter_lc=False)
    for q in range(nq):
        bits = [ic.score_bits(tuple(int(v) for v in counts[y])) for y in range(int(w["fam_off"][q]), int(w["fam_off"][q + 1]))]
        scored = [b for b, ok in bits if ok]
        assert tuple(int(x) for x in idty[q]) == (max(scored) if scored else 0, len(scored)), q


# ---------------------------------------------------------------- stage level: the aligner's device-shift
FF = {"fs-min-len": 50, "fs-full-len": 150}
AL = {"lowercase": "unaligned", "calc-idty": 1, "device-bps": 1, "device-idty": 1}
_TRAY_FIELDS = ("status", "head", "tail", "qual", "width", "log", "family", "bp_score")


@pytest.fixture(scope="module")
def stage(oracle):
    from sina_amd import pipeline
    refs, qs, caps = sc.stage_world()
    cs = util.cseqs_from_refs(refs)
    idx = oracle.Index(cs, k=10)
    want = []
    for qi in range(qs.n):
        q = util.query_cseq(qs, qi, upper=False)
        ids, _, _ = idx.famfinder(q, oracle.ff_opts(fs_min_len=50, fs_full_len=150))
        want.append(oracle.align([cs[i] for i in ids], q, oracle.align_opts(lowercase=2)))
    st = pipeline.Store(":mem:gpu-shift", refs)
    helix = np.zeros(refs.width, np.uint32)
    cols = np.arange(5, refs.width // 2 - 5)
    helix[cols] = refs.width - 1 - cols
    helix[refs.width - 1 - cols] = cols
    st.set_pairs(helix)
    yield st, qs, caps, want
    st.close()


def _run_stage(st, qs, shift):
    from sina_amd import pipeline
    pl = pipeline.Pipeline(st, famfinder=FF, aligner=dict(AL, **{"device-shift": shift}))
    pl.run(qs.mask, qs.off, batch=8, inflight=2)
    res = [pl.result(q) for q in range(qs.n)]
    pl.close()
    return res


def test_stages_with_and_without_device_shift(stage):
    """Pipeline with device-shift off and on, device-bps and device-idty on in both: identical trays -- sequence, every
    attribute, log text --, the oracle's sequences, and with the option on only the queries beyond the caps are left
    to the host, so the in-place scores cover the shifted trays too."""
    st, qs, caps, want = stage
    a0, p0, i0 = st.assemble_stats(), st.pair_inplace_stats(), st.identity_inplace_stats()
    off = _run_stage(st, qs, 0)
    a1, p1, i1 = st.assemble_stats(), st.pair_inplace_stats(), st.identity_inplace_stats()
    on = _run_stage(st, qs, 1)
    a2, p2, i2 = st.assemble_stats(), st.pair_inplace_stats(), st.identity_inplace_stats()
    events = [len(sc.log_events(w["log"])) for w in want]
    assert [q for q in range(qs.n) if events[q] > sr.SHIFT_LOG] == list(caps)
    for q in range(qs.n):
        a, b, w = off[q], on[q], want[q]
        assert a["status"] == b["status"] == w["status"] == 0, q
        for f in _TRAY_FIELDS:
            assert a[f] == b[f], (q, f, a[f], b[f])
        assert (a["packed"] == b["packed"]).all() and (b["packed"] == w["packed"]).all(), q
        assert util.f32_bits(a["idty"]) == util.f32_bits(b["idty"]) == util.f32_bits(w["idty"]), q
        assert util.f32_bits(a["bps"]) == util.f32_bits(b["bps"]), q
        assert sc.log_events(b["log"]) == sc.log_events(w["log"]) and sc.log_totals(b["log"]) == sc.log_totals(w["log"]), q
    shifted = sum(e > 0 for e in events)
    host_off, host_on = a1["trays_host"] - a0["trays_host"], a2["trays_host"] - a1["trays_host"]
    print("host-finished trays: %d without device-shift, %d with it; %d of %d queries shift" % (host_off, host_on, shifted, qs.n))
    assert host_off == shifted and host_on == len(caps)
    assert a1["shifted_queries"] == a0["shifted_queries"]                       # option off: no shifted run on the device
    assert a2["shifted_queries"] - a1["shifted_queries"] == shifted - len(caps)
    assert a2["shifted_runs"] - a1["shifted_runs"] == sum(e for e in events if e <= sr.SHIFT_LOG)
    # the in-place scores follow the assembly: no code of their own
    assert p1["trays"] - p0["trays"] == qs.n - shifted and p2["trays"] - p1["trays"] == qs.n - len(caps)
    assert i1["trays"] - i0["trays"] == qs.n - shifted and i2["trays"] - i1["trays"] == qs.n - len(caps)


def test_run_fasta_with_and_without_device_shift(stage, tmp_path):
    from sina_amd import pipeline, synth
    st, qs, caps, want = stage
    src = str(tmp_path / "in.fasta")
    with open(src, "w") as f:
        for q in range(qs.n):
            f.write(">q%d\n%s\n" % (q, synth.bases_string(qs.seq(q))))
    runs = {}
    for on in (0, 1):
        dst = str(tmp_path / ("out%d.fasta" % on))
        a0 = st.assemble_stats()
        got = pipeline.run_fasta(st, src, dst, famfinder=FF, aligner=dict(AL, **{"device-shift": on}),
                                 fasta={"meta-fmt": "comment"}, batch=8)
        text = [l for l in open(dst).read().splitlines() if not l.lstrip("; ").startswith("aligned_slv")]   # (the date)
        runs[on] = (got, text, st.assemble_stats()["trays_host"] - a0["trays_host"])
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and len(runs[1][1]) > 2 * qs.n
    assert runs[1][2] == len(caps) < runs[0][2]
