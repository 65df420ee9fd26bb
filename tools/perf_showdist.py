"""--show-dist on the bench's 16S shape: a leave-out FASTA run -- the store's own sequences as aligned
input, realign, fs-leave-query-out, show_dist on, as the reference's accuracy protocol runs it -- for three builds:

    python tools/perf_showdist.py --parent-tree DIR [--queries 2048] [--refs 20000] [--rounds 3] [--batch 1024] [--out FILE]

DIR: a checkout of the parent commit with its libraries built (sina_amd/libsina_hip.so, libsina_host.so).  Legs: that
build; this build with the aligner's device-dist off; this build with it on.  Every run is a process of its own, the
legs alternating round by round (measuring-on-mi355x: A B C A B C ...); a process makes the store, runs one warm-up pass
and one timed pass.  Per timed pass: sequences/s, busy host cores, the host phase profiler's time in the sink's report
step (sink.report: this build only, the parent has no such phase) and in the device step (sd.*), the trays scored on
the device and the show-dist kernel's launches, pairs, time by its own events and pairs/s.

Prints JSON lines; --out appends them to FILE (profiles/perf_showdist.txt)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTH, WIDTH = 1500, 50000


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def phase_ms(profile, prefix):
    """Sum of the wall times (ms) of the profile's lines whose phase name starts with prefix."""
    total = 0.0
    for line in profile.splitlines():
        m = re.match(r"(\S+)\s+([0-9.]+) s\s+\d+ calls", line)      # "<phase>   <seconds> s  <n> calls"
        if m and m.group(1).startswith(prefix):
            total += 1e3 * float(m.group(2))
    return total


def leg(a):
    """One process: the store, a warm-up pass, a timed pass; one JSON line on stdout."""
    sys.path.insert(0, a.tree)
    import numpy as np
    from sina_amd import pipeline, synth
    refs = synth.make_refs(a.refs, length=LENGTH, width=WIDTH, seed=2)
    store = pipeline.Store(":mem:perf-showdist", refs)
    store.build_index(10, False)
    if not os.path.exists(a.fasta):
        pick = np.linspace(0, refs.n - 1, a.queries).astype(int)
        with open(a.fasta + ".tmp", "w") as f:
            for i in pick:
                f.write(">ref%d\n%s\n" % (i, synth.aligned_string(refs.seq(int(i)), refs.width)))
        os.replace(a.fasta + ".tmp", a.fasta)
    al = {"realign": True}
    if a.device_dist:
        al["device-dist"] = True
    ffo = {"fs-leave-query-out": True}
    H = pipeline.load_host()

    def one(tag):
        has = hasattr(store, "show_dist_stats")
        d0 = store.show_dist_stats() if has else None
        H.sina_host_profile(1)
        c0, t0 = os.times(), time.perf_counter()
        got = pipeline.run_fasta(store, a.fasta, a.fasta + ".out", famfinder=ffo, aligner=al, show_dist=True, batch=a.batch)
        wall = time.perf_counter() - t0
        c1 = os.times()
        prof = H.sina_host_profile(1).decode()
        d1 = store.show_dist_stats() if has else None
        cpu = (c1.user - c0.user) + (c1.system - c0.system)
        rec = dict(tool="perf_showdist", build=a.name, tag=tag, device_dist=bool(a.device_dist), queries=got["read"], aligned=got["aligned"],
                   refs=refs.n, batch=a.batch, wall_s=wall, sequences_per_s=got["read"] / wall, busy_host_cores=cpu / wall,
                   avg_sps=got["avg_sps"], avg_cpm=got["avg_cpm"], avg_idty=got["avg_idty"],
                   report_phase_ms=phase_ms(prof, "sink.report"), device_step_phase_ms=phase_ms(prof, "sd."))
        if has:
            ms, pairs = d1["kernel_ms"] - d0["kernel_ms"], d1["pairs"] - d0["pairs"]
            rec.update(device_trays=d1["trays"] - d0["trays"], kernel_launches=d1["launches"] - d0["launches"], kernel_pairs=pairs,
                       kernel_ms=ms, kernel_pairs_per_s=pairs / (ms * 1e-3) if ms else 0.0)
        print(json.dumps(rec), flush=True)

    one("warm-up")
    one("timed")
    store.close()


def main(a):
    tmp = tempfile.mkdtemp(prefix="perf_showdist_")
    fasta = os.path.join(tmp, "in.fasta")
    legs = [("parent", a.parent_tree, 0), ("this, device-dist off", HERE, 0), ("this, device-dist on", HERE, 1)]
    if not a.parent_tree:
        legs = legs[1:]
    for rnd in range(a.rounds):
        for name, tree, on in legs:
            env = dict(os.environ, SINA_HOST_PROFILE="1")
            env.pop("SINA_HIP_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--tree", tree, "--name", name, "--device-dist", str(on),
                   "--fasta", fasta, "--queries", str(a.queries), "--refs", str(a.refs), "--batch", str(a.batch)]
            run = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=a.leg_timeout)
            if run.returncode != 0:
                raise SystemExit("leg %r failed with status %d" % (name, run.returncode))
            for line in run.stdout.splitlines():
                if line.startswith("{"):
                    emit(dict(json.loads(line), round=rnd), a.out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--refs", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--name", default="this")
    ap.add_argument("--device-dist", type=int, default=0)
    ap.add_argument("--fasta", default=None)
    a = ap.parse_args()
    leg(a) if a.leg else main(a)
