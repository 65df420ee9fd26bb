"""The DP kernels across the scoring gates that pick them (tests/gate_cases.py): every case of the table -- signs, zeros
and either side of every threshold of the scoring parameters and the node weights -- against the oracle, whose planes
tests/test_gates_cpu.py pins to the reference's own, and against a plain model of the gates that says which kernel
must have run (sina_hip_dp_info::kernel), whether it skipped rows and whether its waves scouted.

Per case: (a) the full sweep, through the kernel the launch chooses and through the generic one; (b) the production
launch with its certified row skip, the guess left alone and forced too bold; (c) the finished alignments of
sina_hip_align_graphs and -- device DAG build, scout, walk, assembly -- sina_hip_align_families.  A closing test counts
what ran and compares the counts with the model's."""
import collections
import types

import numpy as np
import pytest

from sina_amd import capi
from tests import gate_cases as gc, util, walk_ref
from tests.prune_ref import _check_planes

pytestmark = pytest.mark.gpu

CASES = gc.all_cases()
# what ran, for the closing test: (stage, case id, geometry, variant) -> (kernel, skipped rows?)
_RAN = {}


@pytest.fixture(scope="module", params=CASES, ids=[c["id"] for c in CASES])
def ref(request, oracle):
    """A case with its reference, computed once for the case's tests: the family, the query, the oracle's DAG and planes,
    the cells of the optimal path and the finished alignment."""
    case = request.param
    cs, q = gc.family_cseqs(case["fam"]), gc.query_cseq(case["fam"])
    refs, ids, qm = gc.family(case["fam"])
    g = util.graph_dict(cs, case["fs_weight"])
    cells = oracle.mesh_compute(cs, q, gc.oracle_opts(case))
    cells.setflags(write=False)
    em, es = walk_ref.end_cell(g, cells["value"])
    return types.SimpleNamespace(case=case, cs=cs, q=q, qm=qm, refs=refs, ids=ids, g=g, cells=cells,
                                 optimum=np.float32(cells["value"][em, es]), path=gc.path_cells(g, cells),
                                 want=oracle.align(cs, q, gc.oracle_opts(case, realign=1)),
                                 simple=case["wvar"] is None and not case["forbid"],
                                 geoms=gc.FAMILIES[case["fam"]]["geoms"])


@pytest.fixture(scope="module")
def family_ctx():
    """One context per world with the world's references on the device (sina_hip_align_families)."""
    made = {}

    def get(fam):
        f = gc.FAMILIES[fam]
        key = (f["length"], f["width"], f["seed"])
        if key not in made:
            refs = gc.world(*key)
            ctx = capi.Context(0)
            ctx.upload_refs(refs.ab, refs.off, refs.width)
            made[key] = ctx
        return made[key]
    yield get
    for ctx in made.values():
        ctx.close()


def _assert_planes_equal(r, vm, vs, val, what):
    assert (util.f32_bits(val) == util.f32_bits(r.cells["value"])).all(), what
    assert (vm == r.cells["value_midx"]).all(), what
    assert (vs == r.cells["value_sidx"]).all(), what


def test_full_sweep_equals_oracle_through_both_kernels(ref, gpu_ctx, monkeypatch):
    """debug_mesh(prune=False) under every geometry of the case, with the default kernel choice and with generic=1 (the
    weighted and forbid cases once: they have no second kernel): value bits, value_midx and value_sidx equal the
    oracle's cell for cell, and the kernel that ran is the model's."""
    r = ref
    gb = gpu_ctx.graph_batch([r.g], r.refs.width)
    for geom in r.geoms:
        for generic in ((False, True) if r.simple else (False,)):
            util.set_knobs(monkeypatch, geom=geom, generic=1 if generic else None)
            vm, vs, val = gpu_ctx.debug_mesh(gb, r.qm, gc.device_params(gpu_ctx, r.case), prune=False)
            info = gpu_ctx.dp_info(0)
            want = gc.expected_path(r.case, "debug_mesh", geom, generic=generic, prune=False)
            assert capi.DP_KERNELS[info["kernel"]] == want["kernel"], (geom, generic)
            assert info["attempts"] == 0 and info["prune_step"] == 0
            _assert_planes_equal(r, vm, vs, val, (geom, generic))
            _RAN[("sweep", r.case["id"], geom, generic)] = (capi.DP_KERNELS[info["kernel"]], False)


def test_row_skip_equals_oracle_where_the_model_says_it_runs(ref, gpu_ctx, monkeypatch):
    """The production launch, debug_mesh(prune=True), on the two-strip geometries, with the guess left alone and with
    rho=2 (every query takes its second attempt).  Where the model says the skip is on: attempts >= 1, the cells at or
    below the bound are the oracle's and every other cell is above its bound, every cell of the oracle's optimal path is
    among the compared ones, and the optimum is the oracle's bit for bit.  Elsewhere -- every weighted and forbid case
    too -- attempts == 0 and the planes are the oracle's cell for cell.  Kernel and prune_step are the model's."""
    r = ref
    gb = gpu_ctx.graph_batch([r.g], r.refs.width)
    for geom in r.geoms:
        if int(geom.split(",")[0]) < 128:
            continue
        for rho in (None, "2"):
            want = gc.expected_path(r.case, "debug_mesh", geom, rho_fixed=rho is not None)
            if rho is not None and not want["skip"]:
                continue   # (no skip: the guess is never read)
            util.set_knobs(monkeypatch, geom=geom, rho=rho)
            vm, vs, val = gpu_ctx.debug_mesh(gb, r.qm, gc.device_params(gpu_ctx, r.case), prune=True)
            info = gpu_ctx.dp_info(0)
            assert capi.DP_KERNELS[info["kernel"]] == want["kernel"], (geom, rho)
            assert info["prune_step"] == want["prune_step"], (geom, rho)
            assert (info["attempts"] >= 1) == want["skip"], (geom, rho, info["attempts"])
            assert util.f32_bits(np.float32(info["raw"])) == util.f32_bits(r.optimum), (geom, rho)
            if want["skip"]:
                _, alive = _check_planes(gpu_ctx, r.cells, vm, vs, val)
                assert all(alive[m, s] for m, s in r.path), "a cell of the optimal path was not among the compared cells"
                if rho == "2":
                    assert info["attempts"] >= 2
            else:
                _assert_planes_equal(r, vm, vs, val, (geom, rho))
            _RAN[("skip", r.case["id"], geom, rho)] = (capi.DP_KERNELS[info["kernel"]], info["attempts"] >= 1)


def _assert_alignment(r, out, pos, what):
    assert (out["status"] == 0) == (r.want["status"] == 0), (what, out["status"], r.want["status"], r.want["log"])
    if r.want["status"] != 0:
        return
    with np.errstate(divide="ignore"):   # (all scores zero: the weight sum is 0, the reference divides all the same)
        score = np.float32(out["raw"]) / np.float32(out["sum_weight"])
    assert util.f32_bits(score) == util.f32_bits(r.want["score"]), what
    aligned, _ = util.finish_alignment(r.qm, out, pos[:len(r.qm)], r.refs.width)
    assert aligned == r.want["aligned"], what


def test_finished_alignments_equal_oracle(ref, gpu_ctx, family_ctx, monkeypatch):
    """sina_hip_align_graphs for every case, sina_hip_align_families (device DAG build with its bound, scout, walk,
    assembly) for the unweighted ones: status, the bits of raw / sum_weight and the finished alignment equal
    oracle.align(realign=1); the kernel is the model's, and the scout value is a number exactly where the model says the
    scout runs."""
    r = ref
    qoff = np.array([0, len(r.qm)], np.uint64)
    gb = gpu_ctx.graph_batch([r.g], r.refs.width)
    for geom in r.geoms:
        util.set_knobs(monkeypatch, geom=geom)
        out, pos = gpu_ctx.align_graphs(gb, r.qm, qoff, gc.device_params(gpu_ctx, r.case))
        info = gpu_ctx.dp_info(0)
        want = gc.expected_path(r.case, "align_graphs", geom)
        assert capi.DP_KERNELS[info["kernel"]] == want["kernel"], geom
        assert (info["attempts"] >= 1) == want["skip"] and info["prune_step"] == want["prune_step"], geom
        assert np.isnan(info["scout"])      # (a caller's DAG has no chain to scout along)
        _assert_alignment(r, out[0], pos, ("align_graphs", geom))
        _RAN[("graphs", r.case["id"], geom, None)] = (capi.DP_KERNELS[info["kernel"]], info["attempts"] >= 1)
        if r.case["wvar"] is not None:
            continue
        ctx = family_ctx(r.case["fam"])
        out, pos = ctx.align_families(r.ids, np.array([0, len(r.ids)], np.uint64), r.qm, qoff, gc.device_params(ctx, r.case))
        info = ctx.dp_info(0)
        want = gc.expected_path(r.case, "align_families", geom)
        assert capi.DP_KERNELS[info["kernel"]] == want["kernel"], geom
        assert (info["attempts"] >= 1) == want["skip"] and info["prune_step"] == want["prune_step"], geom
        assert np.isnan(info["scout"]) == (not want["scout"]), (geom, info["scout"])
        _assert_alignment(r, out[0], pos, ("align_families", geom))
        _RAN[("families", r.case["id"], geom, None)] = (capi.DP_KERNELS[info["kernel"]], info["attempts"] >= 1)


def test_counts_per_path_equal_the_model():
    """Over the whole table: how many launches ran each kernel kind and how many ran the skip, per stage -- exactly the
    model's numbers, so that a gate that silently sends cases elsewhere changes a count."""
    model = {}
    for case in CASES:
        simple = case["wvar"] is None and not case["forbid"]
        for geom in gc.FAMILIES[case["fam"]]["geoms"]:
            for generic in ((False, True) if simple else (False,)):
                p = gc.expected_path(case, "debug_mesh", geom, generic=generic, prune=False)
                model[("sweep", case["id"], geom, generic)] = (p["kernel"], False)
            if int(geom.split(",")[0]) >= 128:
                for rho in (None, "2"):
                    p = gc.expected_path(case, "debug_mesh", geom, rho_fixed=rho is not None)
                    if rho is None or p["skip"]:
                        model[("skip", case["id"], geom, rho)] = (p["kernel"], p["skip"])
            p = gc.expected_path(case, "align_graphs", geom)
            model[("graphs", case["id"], geom, None)] = (p["kernel"], p["skip"])
            if case["wvar"] is None:
                p = gc.expected_path(case, "align_families", geom)
                model[("families", case["id"], geom, None)] = (p["kernel"], p["skip"])
    assert set(_RAN) == set(model), "not every launch of the table ran before this test (run the whole module)"

    def counts(d):
        c = collections.Counter()
        for (stage, _, _, _), (kernel, skipped) in d.items():
            c[(stage, kernel)] += 1
            c[(stage, "rows skipped")] += int(skipped)
        return c
    got, want = counts(_RAN), counts(model)
    print("launches per stage and kernel:", dict(sorted(got.items())))
    assert got == want
    # every kernel kind and the skip are reached, in the numbers the table was laid out for
    per_kernel = collections.Counter(k for (_, k), n in want.items() for _ in range(n) if k != "rows skipped")
    assert set(per_kernel) == set(gc.KERNELS) - {"none"}
    assert want[("skip", "rows skipped")] > 0 and want[("families", "rows skipped")] > 0 and want[("graphs", "rows skipped")] > 0
