"""sina_amd/csrc/host/distinct.h -- the bookkeeping behind "every distinct query of a batch goes to the device once" --
in a stand-alone program (tests/distinct_check.cpp) under the address and undefined-behaviour sanitizers: slots, first
occurrences, offsets and gathered bytes against an O(n^2) grouping, for 1-byte and 4-byte elements.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_distinct_items_against_a_plain_grouping(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = str(tmp_path / "distinct_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "sina_amd", "csrc"), os.path.join(ROOT, "tests", "distinct_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert run.returncode == 0 and "distinct_check: ok" in run.stdout, run.stdout[-4000:]
