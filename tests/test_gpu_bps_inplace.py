"""The helix base-pair count where the device assembles the alignment (pair_count_assembled_kernel):
sina_hip_align_count_pairs / sina_hip_staged_pair_counts / sina_hip_pair_inplace_stats through sina_hip_align_graphs on
the trace-back tests' launches (tests/walk_cases.py), and the aligner's device-bps through the stages.

The yardstick is tests/bps_ref.py over the oracle's finished sequences; the re-upload route (sina_hip_pair_counts over
the words the launch returned) is asked for the same rows.  tests/test_bps_inplace_cpu.py checks on the CPU that these
inputs are worth running: ascending columns, counters that are not all zero, assembled and unassembled queries."""
import functools
import re
import zlib

import numpy as np
import pytest

from sina_amd import capi, pairs, pipeline, synth
from tests import bps_cases as bc, bps_ref as br, util, walk_cases as wc

pytestmark = pytest.mark.gpu

# walk_cases groups: `matrix` for its lowercase modes (a lower-case base weighs nothing), `capacity` for 4095 / 4096 /
# 4097 bases, `load_alignment` for sequences of one base and ragged launches, `grid_tail` for more waves than one
# workgroup row, `insertion_scan` for queries the device does not assemble
GROUPS = ("matrix", "insertion_scan", "capacity", "grid_tail", "load_alignment")
# compacted entries per map: one, the 64-lane stride's tail on either side of one whole pass, and many passes
ENTRY_COUNTS = (1, 63, 64, 65, 900)


def helix_map(width, n_entries, seed, occupied=()):
    """A nested random helix map over `width` columns with exactly n_entries paired columns (pairs[i] != 0): 2 P sorted
    columns, the k-th paired with the k-th from the end; an odd count drops the outermost closing column's entry (the
    map need not be symmetric).  Column 0 never takes part (partner 0 means unpaired).  occupied: columns drawn first,
    so that a small map lies where the sequences have bases."""
    rng = np.random.default_rng(seed)
    n_cols = 2 * ((n_entries + 1) // 2)
    occ = np.unique(np.asarray(occupied, np.int64))
    occ = occ[(occ > 0) & (occ < width)]
    take = min(n_cols, len(occ))
    cols = rng.choice(occ, size=take, replace=False) if take else np.zeros(0, np.int64)
    if take < n_cols:
        rest = np.setdiff1d(np.arange(1, width), occ)
        cols = np.concatenate([cols, rng.choice(rest, size=n_cols - take, replace=False)])
    cols = np.sort(cols)
    m = np.zeros(width, np.uint32)
    for k in range(n_cols):
        m[cols[k]] = cols[n_cols - 1 - k]
    if n_entries % 2:
        m[cols[-1]] = 0
    assert int((m != 0).sum()) == n_entries
    return m


def case_maps(case, ref):
    """{entries: map} of one launch, seeded by the case's name."""
    occ = np.concatenate([np.asarray(r["orc"]["packed"], np.uint32) & 0xFFFFFF for r in ref if r["must"]] or
                         [np.zeros(0, np.uint32)])
    return {n: helix_map(case.width, n, zlib.crc32(("%s/%d" % (case.name, n)).encode()), occ) for n in ENTRY_COUNTS}


@functools.lru_cache(maxsize=None)
def expected(group):
    """[(case, ref, {entries: (map, rows [nq, 6])})] of a walk_cases group: bps_ref over the oracle's finished sequence
    where the device must assemble it, six zeros elsewhere.  Computed once per process."""
    out = []
    for case, ref in wc.group(group):
        per = {}
        for n, m in case_maps(case, ref).items():
            rows = np.zeros((len(ref), 6), np.uint32)
            for q, r in enumerate(ref):
                if r["must"]:
                    rows[q] = br.counts(r["orc"]["packed"], m)
            per[n] = (m, rows)
        out.append((case, ref, per))
    return out


def _launch_args(ctx, case, ref):
    graphs = [r["graph"] for r in ref]
    tabs = dict(node_score16=np.concatenate([r["score16"] for r in ref]), self_score16=ref[0]["self16"]) \
        if case.opts["fs_no_graph"] else {}
    gb = ctx.graph_batch(graphs, case.width, **tabs)
    qoff = np.zeros(len(ref) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(m) for m in case.qmasks])
    popts = {k: v for k, v in case.opts.items() if k not in ("fs_no_graph", "weights")}
    return gb, np.concatenate(case.qmasks), qoff, popts


def _align(ctx, case, args, assemble=1):
    gb, qmask, qoff, popts = args
    return ctx.align_graphs(gb, qmask, qoff, ctx.params(weights=case.opts["weights"], assemble=assemble, **popts))


def _finished_words(out, pos, qoff):
    """(q_ab, q_off) of the launch's assembled queries, for the re-upload route."""
    idx = [q for q in range(len(out)) if out[q]["assembled"]]
    parts = [pos[int(qoff[q]):int(qoff[q]) + int(out[q]["n_out"])] for q in idx]
    off = np.zeros(len(idx) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return idx, np.concatenate(parts + [np.zeros(0, np.uint32)]).astype(np.uint32), off


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _check_case(ctx, monkeypatch, case, ref, per):
    args = _launch_args(ctx, case, ref)
    qoff = args[2]
    for lanes in (0, 1):
        util.set_knobs(monkeypatch, bt_lanes=lanes)
        tag = (case.name, "bt_lanes=%d" % lanes)
        ctx.count_pairs(False)
        ctx.upload_pairs(per[ENTRY_COUNTS[0]][0])
        off_stats = ctx.pair_inplace_stats()
        out0, pos0 = _align(ctx, case, args)
        assert ctx.staged_pair_counts() is None and ctx.pair_inplace_stats() == off_stats, tag
        n_asm = int((out0["assembled"] != 0).sum())
        assert [int(a) for a in out0["assembled"]] == [int(r["must"]) for r in ref], tag
        for n in ENTRY_COUNTS:
            m, want = per[n]
            ctx.upload_pairs(m)
            ctx.count_pairs(True)
            s0, p0 = ctx.pair_inplace_stats(), ctx.pair_stats()
            out, pos = _align(ctx, case, args)
            rows = ctx.staged_pair_counts()
            s1 = ctx.pair_inplace_stats()
            assert ctx.pair_stats() == p0, tag                       # the re-upload route's counters stand still
            assert rows is not None and rows.shape == (len(ref), 6), tag
            bad = np.flatnonzero((rows != want).any(axis=1))
            assert len(bad) == 0, tag + ("entries=%d" % n, "query %d" % bad[0], rows[bad[0]].tolist(), want[bad[0]].tolist())
            assert out.tobytes() == out0.tobytes() and pos.tobytes() == pos0.tobytes(), tag + ("entries=%d" % n,)
            assert s1["launches"] - s0["launches"] == 1 and s1["sequences"] - s0["sequences"] == n_asm, tag + (s0, s1)
            assert s1["kernel_ms"] >= s0["kernel_ms"], tag
            idx, q_ab, q_off = _finished_words(out, pos, qoff)
            if idx:
                again = ctx.pair_counts(q_ab, q_off)
                assert (again == rows[idx]).all(), tag + ("entries=%d" % n, "re-upload route differs")
    ctx.count_pairs(False)


@pytest.mark.parametrize("which", range(len(wc.MATRIX_NAMES)), ids=wc.MATRIX_NAMES)
def test_counters_on_the_matrix(oracle, ctx, monkeypatch, which):
    """Every overhang and lowercase mode, shift and forbid, the simple, weighted and profile scheme."""
    case, ref, per = expected("matrix")[which]
    _check_case(ctx, monkeypatch, case, ref, per)


@pytest.mark.parametrize("group", [g for g in GROUPS if g != "matrix"])
def test_counters_on_the_directed_cases(oracle, ctx, monkeypatch, group):
    """Unassembled queries (six zeros), 4095 / 4096 / 4097 bases, 65 and 130 waves, sequences of 1 to 257 bases alone and
    in one ragged launch."""
    for case, ref, per in expected(group):
        _check_case(ctx, monkeypatch, case, ref, per)


def test_several_launch_ranges(oracle, ctx, monkeypatch):
    """SINA_HIP_TEST=dp_range_q=3: twelve queries in four ranges, 65 in 22; every row at its query's index."""
    for group, which in (("matrix", 0), ("grid_tail", 0)):
        case, ref, per = expected(group)[which]
        m, want = per[65]
        args = _launch_args(ctx, case, ref)
        ctx.upload_pairs(m)
        ctx.count_pairs(True)
        util.set_knobs(monkeypatch, dp_range_q=None)
        s0 = ctx.pair_inplace_stats()
        out0, pos0 = _align(ctx, case, args)
        whole = ctx.staged_pair_counts()
        s1 = ctx.pair_inplace_stats()
        assert s1["launches"] - s0["launches"] == 1
        util.set_knobs(monkeypatch, dp_range_q=3)
        out, pos = _align(ctx, case, args)
        rows = ctx.staged_pair_counts()
        s2 = ctx.pair_inplace_stats()
        util.set_knobs(monkeypatch, dp_range_q=None)
        n_ranges = (len(ref) + 2) // 3
        assert n_ranges >= 4
        assert s2["launches"] - s1["launches"] == n_ranges, (case.name, s1, s2)
        assert s2["sequences"] - s1["sequences"] == s1["sequences"] - s0["sequences"] == int((out0["assembled"] != 0).sum())
        assert (rows == want).all() and (whole == want).all(), case.name
        assert len({tuple(r) for r in want.tolist()}) >= 4, case.name  # (rows differ: a row at the wrong index would show)
        assert out.tobytes() == out0.tobytes() and pos.tobytes() == pos0.tobytes(), case.name
    ctx.count_pairs(False)


def test_nothing_counted(oracle, monkeypatch):
    """NULL and no launch with the switch off, with no map, with assemble = 0; a fork starts switched off; an uncounted
    call after a counted one returns NULL, not the rows before."""
    case, ref, per = expected("matrix")[0]
    m, want = per[64]
    ctx = capi.Context(0)
    try:
        args = _launch_args(ctx, case, ref)
        zero = ctx.pair_inplace_stats()
        assert zero == dict(kernel_ms=0.0, sequences=0, launches=0)
        assert ctx.staged_pair_counts() is None                      # no align call yet
        ctx.count_pairs(True)                                        # on, no map
        _align(ctx, case, args)
        assert ctx.staged_pair_counts() is None and ctx.pair_inplace_stats() == zero
        ctx.upload_pairs(m)
        ctx.count_pairs(False)                                       # map, off
        _align(ctx, case, args)
        assert ctx.staged_pair_counts() is None and ctx.pair_inplace_stats() == zero
        ctx.count_pairs(True)                                        # map, on, assemble = 0
        _align(ctx, case, args, assemble=0)
        assert ctx.staged_pair_counts() is None and ctx.pair_inplace_stats() == zero
        fork = ctx.fork()                                            # the parent is on: the fork is not
        try:
            fargs = _launch_args(fork, case, ref)
            _align(fork, case, fargs)
            assert fork.staged_pair_counts() is None and fork.pair_inplace_stats() == zero
            fork.count_pairs(True)                                   # ... and counts with the store's map once it is
            _align(fork, case, fargs)
            assert (fork.staged_pair_counts() == want).all()
        finally:
            fork.close()
        _align(ctx, case, args)                                      # counted ...
        assert (ctx.staged_pair_counts() == want).all()
        one = ctx.pair_inplace_stats()
        assert one["launches"] == 1 and one["sequences"] == sum(r["must"] for r in ref)
        _align(ctx, case, args, assemble=0)                          # ... then not: no stale rows
        assert ctx.staged_pair_counts() is None and ctx.pair_inplace_stats() == one
        _align(ctx, case, args)
        ctx.upload_pairs(np.zeros(0, np.uint32))                     # the map taken away
        _align(ctx, case, args)
        assert ctx.staged_pair_counts() is None
        assert ctx.pair_inplace_stats()["launches"] == 2
    finally:
        ctx.close()


# ---------------------------------------------------------------- through the stages (the world of tests/test_gpu_bps.py)

FF = {"fs-min-len": 100, "fs-full-len": 250}
STAGE_QUERY_SEED = 3052


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


def stage_world():
    """(refs, query masks, offsets, helix map): 500 references of 320 bases in 3200 columns, 63 mutated queries and one
    exact copy (the aligner's copy shortcut), a bracket-line map of 302 pairs."""
    refs = synth.make_refs(500, length=320, width=3200, seed=51, amb_rate=0.01, lower_rate=0.02)
    some = synth.make_queries(refs, 63, seed=STAGE_QUERY_SEED, amb_rate=0.01, lower_rate=0.05, ins=0.01, dele=0.01)
    exact = synth.make_queries(refs, 1, seed=3059, sub=0.0, dele=0.0, ins=0.0)
    mask = np.concatenate([some.mask[:int(some.off[some.n])], exact.mask[:int(exact.off[1])]])
    off = np.concatenate([some.off[:some.n + 1], some.off[some.n] + exact.off[1:2]]).astype(np.uint64)
    helix = pairs.pairs_from_brackets(_bracket_line(refs.width, 300, 77))
    return refs, mask, off, helix


@pytest.fixture(scope="module")
def world():
    refs, mask, off, helix = stage_world()
    st = pipeline.Store(":mem:gpu-bps-inplace", refs)
    yield refs, st, mask, off, helix
    st.close()


def _run_batch(st, mask, off, device_bps, batch):
    pl = pipeline.Pipeline(st, famfinder=FF, aligner={"device-bps": 1 if device_bps else 0})
    pl.run(mask, off, batch=batch, inflight=2)
    res = [pl.result(q) for q in range(len(off) - 1)]
    pl.close()
    return res


def _run(st, mask, off, device_bps):
    return _run_batch(st, mask, off, device_bps, 16)


def test_stages_score_in_place(world):
    refs, st, mask, off, helix = world
    nq = len(off) - 1
    assert nq == 64
    st.set_pairs(helix)
    try:
        p0, i0 = st.pair_stats(), st.pair_inplace_stats()
        plain = _run(st, mask, off, False)
        p1, i1 = st.pair_stats(), st.pair_inplace_stats()
        got = _run(st, mask, off, True)
        p2, i2 = st.pair_stats(), st.pair_inplace_stats()
    finally:
        st.set_pairs(np.zeros(0, np.uint32))
    n_dp = sum(1 for r in got if r["status"] == 0)
    n_copy = sum(1 for r in got if r["status"] == 1)
    assert n_dp >= 55 and n_copy >= 1
    nonzero = 0
    for q in range(nq):
        a, b = plain[q], got[q]
        assert a["status"] == b["status"] and a["log"] == b["log"], q
        if b["status"] == 2:
            assert b["bp_score"] == 0 and b["bps"] == 0
            continue
        assert (a["packed"] == b["packed"]).all(), q
        sc = br.score(br.counts(b["packed"], helix))
        assert br.bits(b["bps"]) == br.bits(sc) and b["bp_score"] == br.attr(sc), (q, b["bps"], sc)
        assert br.bits(a["bps"]) == br.bits(b["bps"]) and a["bp_score"] == b["bp_score"], q
        nonzero += b["bp_score"] != 0
    assert nonzero >= 55
    # option off: everything on the re-upload route, nothing in place
    assert i1 == i0 and p1["sequences"] - p0["sequences"] == n_dp + n_copy
    # option on: every scored tray is on exactly one of the two routes, and most of the DP's are in place
    trays = i2["trays"] - i1["trays"]
    again = p2["sequences"] - p1["sequences"]
    print("in place %d trays, re-uploaded %d sequences, n_dp %d, n_copy %d" % (trays, again, n_dp, n_copy))
    assert trays + again == n_dp + n_copy
    assert 2 * trays >= n_dp
    assert trays <= n_dp and again >= n_copy                        # the copy-shortcut tray never saw the DP: re-uploaded
    assert i2["sequences"] - i1["sequences"] == trays               # (64 distinct queries: one assembled slot per tray)
    assert i2["launches"] - i1["launches"] >= 4                     # one per DP launch range, a batch has one at least
    assert i2["kernel_ms"] >= i1["kernel_ms"]


def test_trays_of_one_slot_share_its_counters(world):
    """Every query twice in one batch: the device sees each once (host dedup), both trays take the slot's row."""
    refs, st, mask, off, helix = world
    n = 16
    end = int(off[n])
    mask2 = np.concatenate([mask[:end], mask[:end]])
    off2 = np.concatenate([off[:n + 1], off[1:n + 1] + np.uint64(end)]).astype(np.uint64)
    st.set_pairs(helix)
    try:
        i0, p0 = st.pair_inplace_stats(), st.pair_stats()
        got = _run_batch(st, mask2, off2, True, batch=32)
        i1, p1 = st.pair_inplace_stats(), st.pair_stats()
    finally:
        st.set_pairs(np.zeros(0, np.uint32))
    assert all(r["status"] == 0 for r in got)
    for q in range(n):
        a, b = got[q], got[n + q]
        assert (a["packed"] == b["packed"]).all() and br.bits(a["bps"]) == br.bits(b["bps"]) and a["bp_score"] == b["bp_score"]
        assert br.bits(a["bps"]) == br.bits(br.score(br.counts(a["packed"], helix))), q
    trays, slots = i1["trays"] - i0["trays"], i1["sequences"] - i0["sequences"]
    assert trays == 2 * slots and trays + (p1["sequences"] - p0["sequences"]) == 2 * n and slots >= n // 2


def test_stages_without_a_map_launch_nothing(world):
    refs, st, mask, off, helix = world
    p0, i0 = st.pair_stats(), st.pair_inplace_stats()
    got = _run(st, mask, off, True)
    assert all(r["bp_score"] == 0 and r["bps"] == 0 for r in got)
    assert st.pair_stats() == p0 and st.pair_inplace_stats() == i0


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


def test_run_fasta_gives_the_same_records(world, tmp_path):
    refs, st, mask, off, helix = world
    nq = 40
    src = str(tmp_path / "in.fasta")
    with open(src, "w") as f:
        for q in range(nq):
            f.write(">q%d\n%s\n" % (q, synth.bases_string(mask[int(off[q]):int(off[q + 1])])))
    st.set_pairs(helix)
    try:
        runs = {}
        for on in (0, 1):
            dst, logp = str(tmp_path / ("out%d.fasta" % on)), str(tmp_path / ("log%d.txt" % on))
            i0 = st.pair_inplace_stats()
            got = pipeline.run_fasta(st, src, dst, famfinder=FF, aligner={"device-bps": on}, fasta={"meta-fmt": "comment"},
                                     batch=16, log_path=logp)
            recs = _fasta_records(dst)
            for r in recs:
                r[1].pop("aligned_slv", None)                       # (the date)
            runs[on] = (got, recs, st.pair_inplace_stats()["trays"] - i0["trays"],
                        [int(v) for v in re.findall(r"^align_bp_score_slv: (-?\d+)$", open(logp).read(), re.M)])
    finally:
        st.set_pairs(np.zeros(0, np.uint32))
    (g0, r0, t0, a0), (g1, r1, t1, a1) = runs[0], runs[1]
    assert len(r0) >= 35 and r0 == r1 and a0 == a1
    assert all("align_bp_score_slv" in m for _, m, _ in r1)
    assert sum(1 for _, m, _ in r1 if int(m["align_bp_score_slv"]) != 0) >= 30
    for name, meta, text in r1:
        assert int(meta["align_bp_score_slv"]) == br.attr(br.score(br.counts(bc.words_of(text), helix))), name
    assert np.float64(g0["avg_bps"]).tobytes() == np.float64(g1["avg_bps"]).tobytes() and g1["avg_bps"] != 0
    assert {k: v for k, v in g0.items() if k != "avg_bps"} == {k: v for k, v in g1.items() if k != "avg_bps"}
    assert t0 == 0 and 2 * t1 >= len(r1) - 1
