"""The code-object registry and kernarg slab of the direct-dispatch path (pgmpy_amd/csrc/pgm_share.h) as
a stand-alone CPU program with stubbed load / allocate callbacks (tools/share_selftest.cpp; its header
gives the sanitizer build line)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_share_selftest(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "share_selftest")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-I", os.path.join(ROOT, "pgmpy_amd", "csrc"),
                            os.path.join(ROOT, "tools", "share_selftest.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "share_selftest ok" in run.stdout, run.stdout + run.stderr
