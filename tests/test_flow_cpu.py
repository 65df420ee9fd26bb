"""The staged runner of the host drivers and its hand-over queue (sina_amd/csrc/host/flow.h: delivery, order, the
bound on items in flight, one or two bodies that throw while the queues are full or empty, a sink error that stops
the sources) on the CPU: tests/flow_check.cpp, a stand-alone program, built with the thread sanitizer and run once.

Measured: the program runs for 0.5 s (its own figure; about 120 runs of at most 50 items with naps of up to 0.2 ms),
and building it takes 3 s; with four busy processes per core beside it, 5 s.  No case depends on which thread runs
first: where two throwers have to meet, the shapes are chosen so that the second can always arrive (flow_check.cpp,
two_throwers).  A run that deadlocks is ended at TIME_LIMIT_S and fails the test; the program prints each
case as it starts, so the output names the one that hung."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_LIMIT_S = 120  # (240 times the measured run time: a loaded machine passes, a deadlock still ends)


def test_flow_runner_under_the_thread_sanitizer(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "flow_check")
    subprocess.run([cxx, "-std=c++20", "-O1", "-g", "-fsanitize=thread", "-pthread",
                    "-I" + os.path.join(ROOT, "sina_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "flow_check.cpp"), "-o", exe], check=True)
    try:
        run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=TIME_LIMIT_S,
                             env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1"))
    except subprocess.TimeoutExpired as e:
        pytest.fail("flow_check did not end within %d s (a deadlock?):\n%s" % (TIME_LIMIT_S, (e.stdout or b"")[-4000:].decode(errors="replace")))
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and lines and lines[-1].startswith("flow_check: ok"), run.stdout[-4000:]
