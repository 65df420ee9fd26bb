"""The planning code of the DP driver (sina_amd/csrc/dp_plan.h: launch ranges, slot allocation, spill rows, the
row-skip bound, family sharing, the rho update, the launch geometry, the LDS ring, lanes or waves for the walk) against plain models, on the CPU: tests/dp_plan_check.cpp, a
stand-alone program, built with the address and undefined-behaviour sanitizers and run once."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_include():
    for d in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime.h")):
            return os.path.join(d, "include")
    return None


def test_dp_plan_against_plain_models(tmp_path):
    cxx, hip = shutil.which("g++"), _hip_include()
    if not cxx or not hip:
        pytest.skip("needs g++ and the HIP headers")
    exe = str(tmp_path / "dp_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I" + hip, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "sina_amd", "csrc"),
                    os.path.join(ROOT, "tests", "dp_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert run.returncode == 0 and "dp_plan_check: ok" in run.stdout, run.stdout[-4000:]
