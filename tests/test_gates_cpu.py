"""The scoring gates on the CPU (tests/gate_cases.py): the oracle's planes of every case against the reference's own
(tests/golden/gate_vectors.npz: hashes recorded from the reference parts), the table's coverage, the model of the gates
against what the table is meant to reach, and the gate functions of sina_amd/csrc/dp_plan.h against the hand-written table
of tests/gate_check.cpp -- a stand-alone program, built with the address and undefined-behaviour sanitizers and run once
(and once more with the row skip switched off by its argument)."""
import collections
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import gate_cases as gc, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gate_vectors.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {str(i): (tuple(int(x) for x in s), h) for i, s, h in zip(z["case_id"], z["shape"], z["hash"])}


def test_golden_file_covers_the_table(golden):
    assert sorted(golden) == sorted(c["id"] for c in gc.all_cases())
    assert os.path.getsize(GOLDEN) < 64 * 1024


@pytest.mark.parametrize("fam", list(gc.FAMILIES))
def test_oracle_planes_equal_the_reference(oracle, golden, fam):
    """Every case's oracle planes -- value, the two gap values, the four trace-back indices -- hash to what the
    reference's cell loop gave; all values are finite."""
    cs, q = gc.family_cseqs(fam), gc.query_cseq(fam)
    n = 0
    for case in gc.all_cases():
        if case["fam"] != fam:
            continue
        cells = oracle.mesh_compute(cs, q, gc.oracle_opts(case))
        shape, want = golden[case["id"]]
        assert cells.shape == shape, case["id"]
        got = [util.plane_hash(cells[f]) for f in util.MESH_PLANES]
        assert [int(x) for x in got] == [int(x) for x in want], case["id"]
        assert all(np.isfinite(cells[f]).all() for f in ("value", "gapm_val", "gaps_val")), case["id"]
        n += 1
    assert n == sum(1 for c in gc.all_cases() if c["fam"] == fam) and n >= 48


def test_shapes_are_the_ones_the_geometries_need():
    for fam, f in gc.FAMILIES.items():
        refs, ids, qm = gc.family(fam)
        assert len(ids) == f["F"] and len(qm) == f["qlen"]
        for geom in f["geoms"]:
            t, b = (int(x) for x in geom.split(","))
            strip = 64 * b
            assert (len(qm) + strip - 1) // strip == t // 64, (fam, geom)   # every strip of the geometry holds query columns
    assert gc.FAMILIES["A12"]["qlen"] - 256 == 28                          # "128,4": the second strip's real columns
    # a chain whose weights are all equal
    n, wmax, wmin = gc.dag_facts("A1", 1.0)
    assert wmax == wmin == 1.5


def test_weight_vectors_are_the_three_of_the_table():
    """plain: all in [0.2, 2]; zeros: a fifth exactly 0; neg: a tenth negative; each weighted set runs with all three
    under both insertion rules."""
    for fam in ("A12", "A1"):
        w = {v: gc.positional_weights(fam, v) for v in gc.WEIGHT_VARIANTS}
        assert w["plain"].min() >= np.float32(0.2) and w["plain"].max() <= 2.0
        assert 0.15 < (w["zeros"] == 0).mean() < 0.25 and (w["zeros"] >= 0).all()
        assert 0.07 < (w["neg"] < 0).mean() < 0.13 and (np.abs(w["neg"]) == w["plain"]).all()
        refs, _, qm = gc.family(fam)
        assert all(len(x) >= refs.width + len(qm) for x in w.values())   # (position + offset never runs past the end)
    seen = collections.Counter((c["fam"], c["set"], c["wvar"], c["forbid"]) for c in gc.all_cases())
    assert set(seen.values()) == {1}
    weighted_sets = [name for name, _, w in gc.BASE_SETS if w]
    assert len(weighted_sets) == 9
    for fam in ("A12", "A1"):
        for name in weighted_sets:
            for v in gc.WEIGHT_VARIANTS:
                assert (fam, name, v, False) in seen and (fam, name, v, True) in seen


def test_threshold_pairs_sit_on_either_side():
    for fam in gc.FAMILIES:
        sets = {name: sc for name, sc, _ in gc.threshold_sets(fam)}
        n, wmax, _ = gc.dag_facts(fam, 1.0)
        assert gc.gain_units(wmax, gc.kappa64_of(sets["amax_250"][0], -1)) == 250
        assert gc.gain_units(wmax, gc.kappa64_of(sets["amax_251"][0], -1)) == 251
        assert np.nextafter(np.float32(sets["amax_250"][0]), np.float32(np.inf)) == np.float32(sets["amax_251"][0])
        g_in, g_out = np.float32(sets["below_init_in"][2]), np.float32(sets["below_init_out"][2])
        assert np.nextafter(g_in, np.float32(np.inf)) == g_out
        assert gc.below_init_sum(n, g_in, 2) < gc.BELOW_INIT_LIMIT <= gc.below_init_sum(n, g_out, 2)
        assert sets["extend_equals_open"][2] == sets["extend_equals_open"][3]
        assert np.float32(sets["extend_just_above_open"][3]) == np.nextafter(np.float32(5), np.float32(np.inf))


def test_model_reaches_every_path():
    """What the table is for: every kernel kind, the skip on and off for each documented reason, the scout on and off."""
    by = {c["id"]: c for c in gc.all_cases()}

    def path(cid, entry="debug_mesh", geom="128,4", **kw):
        return gc.expected_path(by[cid], entry, geom, **kw)
    assert path("A12-default-unweighted-shift") == dict(kernel="simple_skip", skip=True, prune_step=194, scout=False)
    assert path("A12-default-unweighted-shift", geom="64,8") == dict(kernel="simple", skip=False, prune_step=0, scout=False)
    assert path("A12-default-unweighted-shift", prune=False)["kernel"] == "simple"
    assert path("A12-default-unweighted-shift", generic=True)["kernel"] == "generic_below"
    assert path("A12-default-unweighted-shift", "align_families")["scout"] is True
    assert path("A12-default-unweighted-shift", "align_families", rho_fixed=True)["scout"] is False
    assert path("A12-both_cost-unweighted-shift")["prune_step"] == 1          # kappa == 0
    assert path("A12-all_zero_scores-unweighted-shift")["prune_step"] == 1
    assert path("A12-mismatch_above_match-unweighted-shift")["prune_step"] == 194
    assert path("A12-free_gaps-unweighted-shift")["skip"] is True
    assert path("A12-free_open-unweighted-shift") == dict(kernel="generic_below", skip=False, prune_step=194, scout=False)
    assert path("A12-negative_gaps-unweighted-shift") == dict(kernel="generic", skip=False, prune_step=0, scout=False)
    assert path("A12-negative_extend-unweighted-shift")["kernel"] == "generic"
    assert path("A12-open_1200-unweighted-shift")["kernel"] == "generic" and path("A1-open_1200-unweighted-shift")["kernel"] == "simple_skip"
    assert path("A12-gaps_1e30-unweighted-shift")["kernel"] == "generic"
    for fsw in ("-0.5", "-2", "5"):                                           # amax > 250, or weights below 0
        for entry in ("align_graphs", "align_families"):
            assert path("A12-fs_weight_%s-unweighted-shift" % fsw, entry) == dict(kernel="simple", skip=False, prune_step=0, scout=False)
    assert path("A12-large-unweighted-shift")["kernel"] == "simple"
    assert path("A12-tiny-unweighted-shift")["prune_step"] == 2
    assert path("A12-amax_250-unweighted-shift")["prune_step"] == 250 and path("A12-amax_251-unweighted-shift")["skip"] is False
    assert path("A12-below_init_in-unweighted-shift")["kernel"] == "simple_skip"
    assert path("A12-below_init_out-unweighted-shift")["kernel"] == "generic"
    assert path("A12-extend_equals_open-unweighted-shift")["kernel"] == "simple_skip"
    assert path("A12-extend_just_above_open-unweighted-shift")["kernel"] == "generic_below"
    assert path("A12-default-plain-shift")["kernel"] == "weighted" and path("A12-default-neg-forbid")["kernel"] == "weighted_forbid"
    assert path("A12-default-unweighted-forbid")["kernel"] == "forbid"
    assert path("B12-default-unweighted-shift", geom="128,8")["kernel"] == "simple_skip"


def _hip_include():
    for d in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime.h")):
            return os.path.join(d, "include")
    return None


def test_gate_functions_against_the_hand_written_table(tmp_path):
    cxx, hip = shutil.which("g++"), _hip_include()
    if not cxx or not hip:
        pytest.skip("needs g++ and the HIP headers")
    exe = str(tmp_path / "gate_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I" + hip, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "sina_amd", "csrc"),
                    os.path.join(ROOT, "tests", "gate_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for args in ([], ["0"]):   # (the second run: SINA_HIP_DP_PRUNE=0, handed in as an argument)
        run = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
        assert run.returncode == 0 and "gate_check: ok" in run.stdout, run.stdout[-4000:]
