"""The trace-back walk's per-row table of the first four predecessor ids (pred4: sina_amd/csrc/common.h) as the host
twin prep_range (dp_plan.h) fills it for caller-supplied and host-built DAGs, against the predecessor lists of
tests/graph_ref.build: tests/pred4_check.cpp, a stand-alone program under the address and undefined-behaviour
sanitizers.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import graph_ref as gr, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_CAP = 65535        # nodes of a DAG of the fast path: ids are 16 bits, api.hip refuses more


def _hip_include():
    for d in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime.h")):
            return os.path.join(d, "include")
    return None


@pytest.fixture(scope="module")
def pred4_check(tmp_path_factory):
    cxx, hip = shutil.which("g++"), _hip_include()
    if not cxx or not hip:
        pytest.skip("needs g++ and the HIP headers")
    exe = str(tmp_path_factory.mktemp("pred4") / "pred4_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I" + hip, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "sina_amd", "csrc"),
                    os.path.join(ROOT, "tests", "pred4_check.cpp"), "-o", exe], check=True)
    return exe


def _member(cols, masks):
    return np.asarray(cols, np.uint32) | (np.asarray(masks, np.uint32) << 24)


def fan_family():
    """Five members over six columns: a source (no predecessor), five nodes with one predecessor each, a node with FIVE,
    four nodes with one each, a node with FOUR, a node with one."""
    cols = [0, 5, 10, 15, 20, 25]
    return [_member(cols, m) for m in ([1, 1, 1, 1, 1, 1], [1, 2, 1, 2, 1, 1], [1, 4, 1, 4, 1, 1], [1, 8, 1, 8, 1, 1],
                                       [1, 3, 1, 8, 1, 1])]


def capacity_family():
    """65535 nodes, one per column; the last one (id 65534, the largest a 16-bit id holds below the capacity) has two
    predecessors, 65532 and 65533."""
    a = _member(np.arange(NODE_CAP), np.ones(NODE_CAP))
    cols = np.concatenate([np.arange(NODE_CAP - 2), [NODE_CAP - 1]])
    return [a, _member(cols, np.ones(len(cols)))]


def expected(g):
    """[3 + n, 4]: the chain pred4_check puts in front, then the first four of every row's list, zero where there is none."""
    out = np.zeros((3 + g["n"], 4), np.int64)
    out[1, 0], out[2, 0] = 0, 1
    for m in range(g["n"]):
        ps = g["pred"][g["pred_off"][m]:g["pred_off"][m + 1]][:4]
        out[3 + m, :len(ps)] = ps
    return out


def table(exe, tmp_path, g, kappa64):
    path = str(tmp_path / "dag.txt")
    with open(path, "w") as f:
        f.write("%d %d\n" % (g["n"], len(g["pred"])))
        for a in (g["pos"], g["mask"], util.f32_bits(g["weight"]), g["pred_off"], g["pred"]):
            f.write(" ".join(str(int(x)) for x in a) + "\n")
    run = subprocess.run([exe, path, str(kappa64)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert run.returncode == 0, run.stdout[-4000:]
    lines = run.stdout.strip().split("\n")
    return lines[0], np.array([ln.split() for ln in lines[1:]], np.int64)


def test_fan_in_of_0_1_4_and_5(pred4_check, tmp_path):
    g = gr.build(fan_family())
    counts = np.diff(g["pred_off"].astype(np.int64))
    assert g["n"] == 13 and counts[0] == 0 and sorted(set(counts)) == [0, 1, 4, 5]     # (the case is what it says)
    five = int(np.flatnonzero(counts == 5)[0])
    ok, got = table(pred4_check, tmp_path, g, 0)
    want = expected(g)
    assert got.shape == want.shape and (got == want).all(), (got, want)
    assert (got[3] == 0).all()                                                           # the source row
    assert list(got[3 + five]) == list(g["pred"][g["pred_off"][five]:][:4])              # only the first four of five
    assert int(g["pred"][g["pred_off"][five] + 4]) not in got[3 + five]


def test_last_row_at_the_node_capacity(pred4_check, tmp_path):
    g = gr.build(capacity_family())
    assert g["n"] == NODE_CAP
    ok, got = table(pred4_check, tmp_path, g, 0)
    want = expected(g)
    assert got.shape == want.shape and (got == want).all()
    assert list(got[-1]) == [NODE_CAP - 3, NODE_CAP - 2, 0, 0]


def test_dag_that_is_not_laid_out_by_columns(pred4_check, tmp_path):
    """The columns descend with the node ids: prep_range gives up the row-skip bound (rgain_ok 0) and still fills the
    table -- the ids depend on the edges alone."""
    g = dict(gr.build(fan_family()))
    g["pos"] = g["pos"][::-1].copy()
    ok, got = table(pred4_check, tmp_path, g, 128.0)
    assert ok == "rgain_ok 0"
    assert (got == expected(g)).all()
    ok, _ = table(pred4_check, tmp_path, gr.build(fan_family()), 128.0)
    assert ok == "rgain_ok 1"
