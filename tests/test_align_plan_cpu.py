"""sina_amd/csrc/host/align_plan.h -- which DP jobs of a batch the aligner sends to the device in which call: routes,
groups and their order, weight sets, the in-place counting switches -- in a stand-alone program
(tests/align_plan_check.cpp) under the address and undefined-behaviour sanitizers: hand-written cases with their
expected groups, and every combination of the switches over every batch of up to four jobs against a transcription of
the loop the aligner had.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_plan_against_its_cases_and_the_restated_loop(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "align_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "sina_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "align_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert run.returncode == 0 and "align_plan_check: ok" in run.stdout, run.stdout[-4000:]
