"""The family DAG build's named cases and its plain restatement, on the CPU: every case of tests/graph_cases.py sits
on the edge it names; tests/graph_ref.py build equals the oracle's mseq and the host twin (build_family_graph,
family_graph.cpp) field for field on every case and on the fuzz worlds' families; its dp_words equal dp_plan.h's prep_range
(tests/dp_plan_check.cpp --words, under the address and undefined-behaviour sanitizers).  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sina_amd import capi, pipeline
from tests import graph_cases as gc, graph_ref as gr, util
from tests.test_dp_plan_cpu import _hip_include

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in gc.CASES]


def _same_graph(g, o, what):
    assert g["n"] == o["n"], what
    assert (g["pos"] == o["pos"]).all() and (g["mask"] == o["mask"]).all(), what
    assert (util.f32_bits(g["weight"]) == util.f32_bits(o["weight"])).all(), what
    assert (g["pred_off"] == o["pred_off"]).all() and (g["pred"] == o["pred"]).all(), what
    assert (g["succ_minpos"] == o["succ_minpos"]).all(), what
    if "snk" in o:
        assert (np.flatnonzero(g["sink"]) == np.sort(o["snk"])).all(), what


def _cseqs(oracle, members, width):
    return [oracle.Cseq.from_packed("m%d" % i, np.asarray(m, np.uint32), width) for i, m in enumerate(members)]


def test_case_names_are_unique_and_the_kernel_numbers_are_the_sources():
    assert len(set(IDS)) == len(IDS)
    src = open(os.path.join(ROOT, "sina_amd", "csrc", "graph_build.hip")).read()
    common = open(os.path.join(ROOT, "sina_amd", "csrc", "common.h")).read()
    assert re.search(r"#define SINA_GRAPH_KTC %d\b" % gc.TILE_COLS, src) and re.search(r"#define SINA_GRAPH_TNW %d\b" % gc.WINDOW_NODES, src)
    assert "if (d <= %du)" % gc.NEAR_BITS in src and "std::min<uint32_t>(65535, %d)" % gc.FIRST_NCAP in src
    assert re.search(r"constexpr int kFarLds = %d;" % gr.FAR_LDS, common) and "kMaxSpillRows = %d;" % gr.MAX_SPILL_ROWS in common
    assert "kRecDistShift = %d;" % gr.REC_DIST_SHIFT in common and "kRecDistFar = %du;" % gr.REC_DIST_FAR in common
    # (the LDS carve as graph_cases.graph_bitmap_off adds it up: 17 552 bytes of tables, 256 per member)
    assert gc.graph_bitmap_off(1) == 17808 and gc.graph_bitmap_off(128) == 17552 + 32768


@pytest.mark.parametrize("case", gc.CASES, ids=IDS)
def test_case_sits_on_its_edge(case):
    assert case.on_edge(), case.name
    g = case.graph()
    assert g["n"] <= 65535 and int(np.diff(g["pred_off"].astype(np.int64)).max(initial=0)) <= 255
    for ring in gc.RINGS:   # (no case may run into the one documented refusal of the build)
        assert case.words(ring)["n_spill"] <= gr.MAX_SPILL_ROWS, (case.name, ring)


def test_the_edges_asked_for_are_all_there():
    names = set(IDS)
    for k in (1, 63, 64, 65, 127, 128, 129, 256, 257):
        assert "columns-%d" % k in names
    assert {"pred-dist-64-65", "edge-192-193", "tile-512-nodes", "tile-513-nodes", "tile-31x128-nodes", "fan-in-128",
            "fan-in-straddles-64", "carry-far-across-tiles", "empty-member-first", "empty-member-middle", "single-base-member",
            "one-node", "same-reference-twice", "128-identical-members", "masks-0-then-16", "masks-16-then-0", "all-32-masks",
            "nodes-15000", "one-member-4000-lds", "one-member-6000-global", "rows-256-one-segment", "rows-257-two-segments",
            "width-4001"} <= names
    assert max(c.graph()["n"] for c in gc.CASES) == 15000
    assert gc.RINGS == (1, 3, 4, 5, 8) and gc.FS_WEIGHTS == (1.0, 0.0, 2.5)
    for fam in gc.NO_BASE_FAMILIES:
        assert gr.build(fam)["n"] == 0 and gr.dp_words(gr.build(fam), 4)["first_sink"] == gr.ROW_NONE


@pytest.mark.parametrize("case", gc.CASES, ids=IDS)
def test_plain_build_equals_oracle_mseq(oracle, case):
    cs = _cseqs(oracle, case.family(), case.width)
    for fsw in gc.FS_WEIGHTS:
        _same_graph(case.graph(fsw), util.graph_dict(cs, fsw), (case.name, fsw))


def test_the_cheap_cases_have_finite_profiles(oracle):
    """What test_gpu_graph.py sends through the profile kernel too: no column of bases without a base bit alone (its profile would be 0 / 0), and a member without a base or a base without a bit among them."""
    cheap = [c for c in gc.CASES if c.profile]
    assert len(cheap) >= 20 and all(c.graph()["n"] <= 600 for c in cheap)
    for case in cheap:
        o = oracle.pseq_build(_cseqs(oracle, case.family(), case.width))
        assert o["n"] >= gc.n_columns(case.graph()) and np.isfinite(np.asarray(o["prof"], np.float32)).all(), case.name
    assert any(min(len(m) for m in c.family()) == 0 for c in cheap)
    assert any(((np.concatenate(c.family()) >> 24) & 0x0F == 0).any() for c in cheap)


def test_plain_build_of_a_family_without_bases_equals_oracle_mseq(oracle):
    for fam in gc.NO_BASE_FAMILIES:
        assert oracle.mseq_build(_cseqs(oracle, fam, gc.WIDTH), 1.0)["n"] == 0 == gr.build(fam)["n"]


@pytest.mark.parametrize("seed", range(int(os.environ.get("SINA_FUZZ_SEEDS", "12"))))
def test_plain_build_equals_oracle_mseq_on_the_fuzz_worlds(oracle, seed):
    rng, pick, refs, cs, usable = util.fuzz_world(seed)
    for _ in range(2):
        ids = list(rng.permutation(usable)[:int(pick([1, 2, 7, 40, 60]))])
        fsw = float(pick(list(gc.FS_WEIGHTS)))
        g = gr.build([refs.seq(int(i)) for i in ids], fsw)
        _same_graph(g, util.graph_dict([cs[int(i)] for i in ids], fsw), (seed, len(ids)))
        first = refs.seq(int(ids[0]))
        assert (g["pos"][g["chain"]] == (first & 0xFFFFFF)).all()      # (the chain: member 0's bases, in their columns)


def test_plain_build_equals_the_host_twin():
    """build_family_graph (host/family_graph.cpp), what the aligner's host route hands to sina_hip_align_graphs."""
    for width, cases in gc.by_width():
        refs, fams = gc.refset(cases)
        st = pipeline.Store(":mem:graphcases%d" % width, refs)
        try:
            for case, ids in zip(cases, fams):
                for fsw in gc.FS_WEIGHTS if not case.big else (1.0,):
                    _same_graph(case.graph(fsw), st.build_graph(ids, fsw), (case.name, fsw))
        finally:
            st.close()


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx, hip = shutil.which("g++"), _hip_include()
    if not cxx or not hip:
        pytest.skip("needs g++ and the HIP headers")
    exe = str(tmp_path_factory.mktemp("plan") / "dp_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I" + hip, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "sina_amd", "csrc"),
                    os.path.join(ROOT, "tests", "dp_plan_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("name,rings", [("edge-192-193", (1, 8)), ("fan-in-128", (3, 4)), ("rows-257-two-segments", (1, 5)),
                                        ("carry-far-across-tiles", (4,))])
def test_dp_words_equal_prep_range(plan_check, tmp_path, name, rings):
    case = next(c for c in gc.CASES if c.name == name)
    g = case.graph()
    path = str(tmp_path / "dag.txt")
    with open(path, "w") as f:
        f.write("%d %d\n" % (g["n"], len(g["pred"])))
        for a in (g["pos"], g["mask"], util.f32_bits(g["weight"]), g["pred_off"], g["pred"]):
            f.write(" ".join(str(int(x)) for x in a) + "\n")
    for ring in rings:
        run = subprocess.run([plan_check, "--words", path, str(ring)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                             env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
        assert run.returncode == 0, run.stdout[-4000:]
        lines = run.stdout.split("\n")
        w = case.words(ring)
        assert lines[0] == "sizes %d %d %d" % (w["n"], w["n_spill"], w["first_sink"])
        rows = np.array([ln.split() for ln in lines[1:1 + g["n"]]], np.uint32)
        assert (rows[:, 0] == w["z"]).all() and (rows[:, 1] == w["store"]).all(), (name, ring)
        assert (np.array(lines[1 + g["n"]:1 + g["n"] + len(g["pred"])], np.uint32) == w["pred"]).all(), (name, ring)


def test_abi_has_the_raw_words_entry():
    hdr = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", hdr)     # (a function was added, no structure changed)
    assert "sina_hip_debug_family_graph_words" in hdr and "sina_hip_debug_family_graph_words" in capi.ABI_SYMBOLS
    L = capi.load()
    assert hasattr(L, "sina_hip_debug_family_graph_words") and L.sina_hip_abi_version() == 5
