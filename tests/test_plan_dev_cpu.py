"""The device side of a plan handle (pgmpy_amd/csrc/pgm_plan_dev.h: the allocations a FitHandle, SampleHandle
or GibbsHandle owns, its lazy stages, the device change, a failed allocation or copy) as a stand-alone CPU
program with stubbed device operations (tools/plan_dev_selftest.cpp), plain and under AddressSanitizer +
UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_plan_dev_selftest(tmp_path, flags):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "plan_dev_selftest")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", *flags, "-I", os.path.join(ROOT, "pgmpy_amd", "csrc"),
                            os.path.join(ROOT, "tools", "plan_dev_selftest.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "plan_dev_selftest ok" in run.stdout, run.stdout + run.stderr
