"""bench.py without a GPU: the launcher logic, the query pool, the output dump and the options."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_gpus_n_starts_its_own_ranks(monkeypatch):
    """`python bench.py --gpus N` with no launcher environment must start N ranks itself (children of
    torch.distributed.run, rendezvous on 127.0.0.1) instead of quietly measuring one GPU; the parent
    decides before it imports torch or touches a GPU."""
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    import torch
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    try:
        bench.main()
        raise AssertionError("bench.main() should leave with the children's exit code")
    except SystemExit as e:
        assert e.code == 7
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    at = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[at + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_bench_under_a_launcher_does_not_spawn():
    """With WORLD_SIZE set (the driver's torch.distributed.run) bench.py is a rank, not a launcher: it goes on
    to the GPU check (and fails it here, loudly -- there is no CPU fallback).  The child sees no GPU even on a
    machine that has one, so that it stops at that check instead of running the benchmark."""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29591")
    p = subprocess.run([sys.executable, "-c",
                        "import sys; sys.argv=['bench.py','--gpus','2'];\n"
                        "import bench, subprocess\n"
                        "def no(*a, **k): raise AssertionError('spawned')\n"
                        "subprocess.call = no\n"
                        "import sina_amd.dist as d; d.init=lambda backend=None:(0,0,2,None)\n"
                        "import torch; torch.cuda.is_available = lambda: False\n"
                        "bench.main()"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "needs a GPU" in p.stderr and "spawned" not in p.stderr


def test_bench_gpus_n_on_a_node_with_fewer_gpus_says_so(monkeypatch, capsys):
    """More ranks than the node has GPUs: a clear message and a non-zero exit before anything is spawned."""
    sys.path.insert(0, ROOT)
    import bench
    import torch

    def no_spawn(*a, **k):
        raise AssertionError("spawned")

    monkeypatch.setattr(subprocess, "call", no_spawn)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    try:
        bench.main()
        raise AssertionError("should have left")
    except SystemExit as e:
        assert e.code == 2
    assert "shows 1 GPU" in capsys.readouterr().err


def test_cycled_steps_walk_the_query_pool():
    """The steps cycle through a pool of distinct queries: query i of a run that starts at `first` is query
    (first + i) mod pool, and the offsets are what Pipeline.run takes (uint64, from 0, one more than queries)."""
    sys.path.insert(0, ROOT)
    import bench
    from sina_amd import synth
    refs = synth.make_refs(40, length=120, width=600, seed=5)
    qs = synth.make_queries(refs, 10, seed=6)
    for first, n in ((0, 10), (3, 4), (7, 26), (25, 1)):
        m, off = bench.cycled(qs, first, n)
        assert off.dtype == np.uint64 and len(off) == n + 1 and off[0] == 0 and off[-1] == len(m)
        for i in range(n):
            assert np.array_equal(m[off[i]:off[i + 1]], qs.seq((first + i) % qs.n)), (first, n, i)


def _fake_result(q):
    rng = np.random.default_rng(q)
    n = int(rng.integers(0, 30))
    ab = (np.sort(rng.choice(1000, size=n, replace=False)).astype(np.uint32)
          | (rng.integers(1, 32, size=n).astype(np.uint32) << 24))
    fam = "".join("ref%d.0:%.2f " % (int(i), s) for i, s in zip(rng.choice(500, size=q % 5, replace=False),
                                                                rng.random(q % 5)))
    return dict(status=q % 3, head=q % 7, tail=q % 11, qual=q % 13, packed=ab, family=fam, log="")


def test_dump_outputs_writes_the_step_as_float_arrays(tmp_path):
    """--dump-outputs: the results of one step as float64 .npy files under 64 MB -- per query status / head / tail /
    qual / base count / CRC-32 of the aligned bases / family, the full bases of a fixed sample -- identical when
    written twice, and a fixed seeded sample of the queries when the step is larger than the cap."""
    import zlib
    sys.path.insert(0, ROOT)
    import bench
    n = bench.DUMP_ALIGNMENTS + 44
    total = bench.dump_outputs(str(tmp_path / "a"), _fake_result, 1000, n)
    bench.dump_outputs(str(tmp_path / "b"), _fake_result, 1000, n)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and 0 < total <= 64 << 20
    d = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for f in files:
        assert d[f[:-4]].dtype == np.float64 and np.array_equal(d[f[:-4]], np.load(tmp_path / "b" / f))
    assert np.array_equal(d["query"], np.arange(n))
    for i in (0, 1, n - 1):
        r = _fake_result(1000 + i)
        assert (d["status"][i], d["head"][i], d["tail"][i], d["qual"][i]) == (r["status"], r["head"], r["tail"], r["qual"])
        assert d["n_bases"][i] == len(r["packed"]) and d["bases_crc32"][i] == zlib.crc32(r["packed"].tobytes())
        ids = [float(x.split(".")[0][3:]) for x in r["family"].split()]
        assert list(d["family_ids"][i, :len(ids)]) == ids and (d["family_ids"][i, len(ids):] == -1).all()
    assert len(d["sample_query"]) == bench.DUMP_ALIGNMENTS and len(d["sample_offsets"]) == bench.DUMP_ALIGNMENTS + 1
    for k, q in enumerate(d["sample_query"].astype(int)):
        ab = _fake_result(1000 + q)["packed"]
        lo, hi = int(d["sample_offsets"][k]), int(d["sample_offsets"][k + 1])
        assert np.array_equal(d["sample_columns"][lo:hi], ab & 0xFFFFFF) and np.array_equal(d["sample_masks"][lo:hi], ab >> 24)
    # a step larger than the cap: a sorted, fixed sample of its queries
    big = bench.DUMP_MAX_QUERIES + 100
    bench.dump_outputs(str(tmp_path / "c"), lambda q: _fake_result(q % 97), 0, big)
    bench.dump_outputs(str(tmp_path / "d"), lambda q: _fake_result(q % 97), 0, big)
    qa, qb = np.load(tmp_path / "c" / "query.npy"), np.load(tmp_path / "d" / "query.npy")
    assert len(qa) == bench.DUMP_MAX_QUERIES and np.array_equal(qa, qb) and (np.diff(qa) > 0).all() and qa[-1] < big


def test_bench_plain_run_needs_no_extra_legs(monkeypatch):
    """The options: --full (the CPU baseline, the oracle check, the isolated step and the confined leg) is off by
    default, --dump-outputs names a directory, and --steps below 1 is refused."""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "0"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 0 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    try:
        bench.parse()
        raise AssertionError("--steps 0 should be refused")
    except SystemExit as e:
        assert e.code == 2


def test_query_pool_is_its_seeded_batches():
    """The pool the steps cycle through: batch b is make_queries(seed=(seed, b)), whatever the threads that made it."""
    sys.path.insert(0, ROOT)
    import bench
    from sina_amd import synth
    refs = synth.make_refs(40, length=120, width=600, seed=5)
    qs = bench.query_pool(refs, 5, 7, 3)
    assert qs.n == 35 and qs.off[0] == 0 and qs.off[-1] == len(qs.mask)
    for b in range(5):
        want = synth.make_queries(refs, 7, seed=(3, b))
        for i in range(7):
            assert np.array_equal(qs.seq(7 * b + i), want.seq(i)) and qs.src[7 * b + i] == want.src[i]
