"""CPU side of the combined riders' tests (tests/test_gpu_riders.py runs the launches): the conditions on the inputs of
tests/riders_cases.py, checked here with the oracle alone, so that the GPU test cannot pass on launches that do not
reach the edge they are there for."""
import numpy as np
import pytest

from tests import riders_cases as rdc, search_inplace_cases as sic


def test_the_table_is_the_one_the_gpu_test_runs(oracle):
    assert tuple(rdc.launches()) == rdc.NAMES and len(set(rdc.NAMES)) == len(rdc.NAMES)
    for name in rdc.NAMES:
        rd = rdc.launches()[name]
        assert rd.nq <= 16 and rd.helix.shape == (rd.launch.width,), name
        assert rd.launch.assemble == (2 if name == "all-shifted" else 1), name
    assert rdc.launches()["all-ranges"].knobs == dict(dp_range_q=3, fam_chunk_q=4, rank_chunk=16)
    assert rdc.launches()["all-shifted"].knobs == dict(dp_range_q=5, fam_chunk_q=6)
    assert rdc.launches()["all-no-name-order"].knobs == dict(dp_range_q=3) and not rdc.launches()["all-no-name-order"].name_order
    assert rdc.launches()["all-no-name-order"].launch.refs is rdc.launches()["all-ranges"].launch.refs
    assert all(not rd.knobs for n, rd in rdc.launches().items() if n not in ("all-ranges", "all-ranges-40", "all-shifted", "all-no-name-order"))


def test_the_cut_of_the_range_launches():
    """Restated here: chunks of fam_chunk_q queries, ranges of dp_range_q inside each."""
    def restated(nq, chunk, per):
        return [(q0, r0, min(r0 + per, min(chunk, nq - q0))) for q0 in range(0, nq, chunk) for r0 in range(0, min(chunk, nq - q0), per)]
    a, s = rdc.launches()["all-ranges"], rdc.launches()["all-shifted"]
    assert (a.nq, s.nq) == (10, 16)
    assert restated(10, 4, 3) == rdc.cut(10, 4, 3) == rdc.RANGES_CUT == [(0, 0, 3), (0, 3, 4), (4, 0, 3), (4, 3, 4), (8, 0, 2)]
    assert restated(16, 6, 5) == rdc.cut(16, 6, 5) == rdc.SHIFTED_CUT == [(0, 0, 5), (0, 5, 6), (6, 0, 5), (6, 5, 6), (12, 0, 4)]
    assert [b for b, _ in rdc.ranges(a)] == [0, 3, 4, 7, 8] and [b for b, _ in rdc.ranges(s)] == [0, 5, 6, 11, 12]
    assert sum(n for _, n in rdc.ranges(a)) == 10 and sum(n for _, n in rdc.ranges(s)) == 16
    # three build chunks each, bases 0, 4, 8 and 0, 6, 12: a non-zero chunk base under a non-zero range base
    assert sorted({q0 for q0, _, _ in rdc.RANGES_CUT}) == [0, 4, 8] and sorted({q0 for q0, _, _ in rdc.SHIFTED_CUT}) == [0, 6, 12]
    assert any(q0 and r0 for q0, r0, _ in rdc.RANGES_CUT) and any(q0 and r0 for q0, r0, _ in rdc.SHIFTED_CUT)
    # all-ranges' 160 candidates per query in chunks of 16: the ranking's merge launch
    assert a.launch.stride == 160 > a.knobs["rank_chunk"]
    assert rdc.ranges(rdc.launches()["all-no-name-order"]) == [(0, 3), (3, 3), (6, 3), (9, 1)]
    assert rdc.ranges(rdc.launches()["all-graphs"]) == [(0, rdc.launches()["all-graphs"].nq)]
    for name in ("all-any-mixed", "all-any-mixed-ranked"):
        rd = rdc.launches()[name]
        assert rd.slots() == [0, None, None, 1, 2, None, 3] and rdc.ranges(rd) == [(0, 1), (3, 2), (6, 1)], name
        assert [rdc.range_of(rd, q) for q in range(rd.nq)] == [0, None, None, 1, 1, None, 2], name


@pytest.mark.parametrize("name", rdc.NAMES)
def test_every_launch_has_rows_that_show_something(oracle, name):
    """A query whose pair row is not all zero and whose identity row is not zero, in every launch; rows that differ
    between queries, so that a row at another query's place shows."""
    rd, want = rdc.case(name)
    ref = want["ref"]
    idty = want["identity"]
    if idty is None:            # (the graphs entries count no identity: what it would be, for the predicate)
        from tests import identity_cases as ic
        l = rd.launch
        idty = np.array([ic.row_of(ref[s]["packed"], [l.refs.seq(int(i)) for i in l.fam_ids[s]])[:2] if s is not None and ref[s]["must"]
                         else (0, 0) for s in rd.slots()], np.uint32)
    both = [q for q in range(rd.nq) if want["pairs"][q].any() and idty[q].any()]
    print(name, "pairs", want["pairs"].tolist(), "identity", idty.tolist())
    assert both, name
    assert want["rank"].shape == (rd.nq, sic.ROW_WORDS) and want["pairs"].shape == (rd.nq, 6)
    if name not in ("all-unassembled",):
        assert want["rank"].any() or name == "all-lost-bases", name
    counted = [q for q in range(rd.nq) if want["pairs"][q].any()]
    if len(counted) > 1:
        assert len({tuple(want["pairs"][q].tolist()) for q in counted}) > 1, name
    for q, s in enumerate(rd.slots()):
        if s is None:
            assert not want["rank"][q].any() and not want["pairs"][q].any(), (name, q)


def test_all_ranges_rows_differ_across_chunks_and_ranges(oracle):
    """A row read at r0 instead of q0 + r0, or from the candidates of query r0, is another query's: it must differ."""
    rd, want = rdc.case("all-ranges")
    for rows in (want["rank"], want["identity"], want["pairs"]):
        assert len({tuple(r.tolist()) for r in rows}) == rd.nq
    ref = want["ref"]
    assert all(r["ranked"] for r in ref)
    # queries 3 and 4 share a family across the chunk boundary (identity_cases): the identity reads the chunk's packed lists
    assert rd.launch.fam_ids[3] is rd.launch.fam_ids[4]


def test_all_ranges_40_candidates_differ_between_queries(oracle):
    """all-ranges ranks every query against all 160 references, whichever candidate row the kernel reads; with 40
    candidates a query's set is its own: the row of query q - q_base (a ranking that forgot the range's base) and of
    query r0 (one that forgot the chunk's) hold other references."""
    rd, want = rdc.case("all-ranges-40")
    full = rdc.case("all-ranges")[0]
    assert rd.launch.refs is full.launch.refs and rd.knobs == full.knobs and rdc.ranges(rd) == rdc.ranges(full)
    assert full.launch.stride == full.launch.refs.n == 160 and rd.launch.stride == 40
    cand = [set(r["cand"].tolist()) for r in want["ref"]]
    assert all(len(c) == 40 for c in cand) and all(r["ranked"] for r in want["ref"])
    for q0, r0, r1 in rdc.RANGES_CUT:
        for q in range(q0 + r0, q0 + r1):
            if q0 + r0:
                assert cand[q] != cand[q - (q0 + r0)], q
            if q0:
                assert cand[q] != cand[q - q0], q
    assert len({tuple(r.tolist()) for r in want["rank"]}) == rd.nq
    assert rd.launch.stride > rd.knobs["rank_chunk"]                 # three chunks: the merge launch


def test_all_shifted_has_events_in_three_ranges(oracle):
    rd, want = rdc.case("all-shifted")
    ev = want["events"]
    with_events = sorted({rdc.range_of(rd, q) for q in range(rd.nq) if ev[q]})
    print("events per query", [len(e) for e in ev], "ranges with an event", with_events)
    assert len(with_events) >= 3
    assert any(not e for e in ev)
    assert want["shift"].shape == (16, 97) and (rdc.shift_rows(ev) == want["shift"]).all()
    assert all(r["must"] and r["kept"] for r in want["ref"])         # every query assembled on the device and ranked
    assert rd.launch.search["flc"] and rd.launch.opts["lowercase"] == 2
    # an event beyond the first chunk: its row lies at a non-zero chunk base
    assert any(ev[q] for q in range(6, 16))


def test_all_unassembled_and_lost_bases(oracle):
    rd, want = rdc.case("all-unassembled")
    must = [r["must"] for r in want["ref"]]
    assert any(must) and not all(must)
    for q, m in enumerate(must):
        if not m:
            assert not want["rank"][q].any() and not want["identity"][q].any() and not want["pairs"][q].any(), q
    rd, want = rdc.case("all-lost-bases")
    lost = [q for q, r in enumerate(want["ref"]) if r["must"] and not r["kept"]]
    assert lost
    for q in lost:
        assert not want["rank"][q].any() and want["identity"][q].any() and want["ref"][q]["full"].any(), q
    assert any(want["pairs"][q].any() for q in lost)


def test_the_ranking_edges_are_still_there(oracle):
    rd, want = rdc.case("all-nan")
    assert any(int(r[1]) & sic.NAN for r in want["rank"])
    rd, want = rdc.case("all-no-hit")
    n_refs, stride = rd.launch.refs.n, rd.launch.stride     # (no 10-mer hit: the candidates are the store's last references)
    assert int(want["rank"][0][1]) & sic.RANKED and int(want["rank"][0][0]) > 0
    assert sorted(want["ref"][0]["cand"].tolist()) == list(range(n_refs - stride, n_refs))
    rd, want = rdc.case("all-tie")
    n = int(want["rank"][0][0])
    assert n == rd.launch.search["n_best"] and 7 in want["rank"][0][2:2 + n].tolist()


def test_the_mixed_batches(oracle):
    from tests import wide_cases as wd
    a, b = rdc.launches()["all-any-mixed"], rdc.launches()["all-any-mixed-ranked"]
    assert a.launch is b.launch and a.launch.refs.n == 400
    assert max(len(m) for _, m, _ in a.batch) == 10241 > 10240          # SINA_HIP_MAX_QUERY_LEN: this call does not rank
    assert max(len(m) for _, m, _ in b.batch) <= 10240
    assert b.batch[2][0] is wd.long_chain().graph and b.batch[2][0]["n"] > 65535
    for rd in (a, b):
        assert rd.batch_width >= max(int(g["pos"].max()) + 1 for g, _, _ in rd.batch)
    assert set(rdc.RANK_OFF) == {"all-any-mixed", "all-no-name-order"}
    want = rdc.case("all-any-mixed-ranked")[1]
    assert all(r["ranked"] for r in want["ref"]) and want["identity"] is None
