"""The host side of the fused row plan (pgmpy_amd/csrc/pgmrows_plan.cpp: plan compiler, generator of the
plan-specialised kernel source, two-rows-per-thread predicates) as a stand-alone CPU program over
hand-built plans (tools/rows_plan_selftest.cpp; its header gives the sanitizer build line)."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("rows_plan") / "rows_plan_selftest")
    csrc = os.path.join(ROOT, "pgmpy_amd", "csrc")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                            os.path.join(ROOT, "tools", "rows_plan_selftest.cpp"),
                            os.path.join(csrc, "pgmrows_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def test_rows_plan_selftest(selftest):
    run = subprocess.run([selftest], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "rows_plan_selftest ok" in run.stdout, run.stdout + run.stderr


def test_selftest_sources_are_the_golden_ones(selftest):
    """The self-test's recorded source hashes and tests/golden/rows_jit_source.json say the same, and the
    generator still emits them."""
    with open(os.path.join(ROOT, "tests", "golden", "rows_jit_source.json")) as f:
        golden = {k[len("selftest/"):]: v for k, v in json.load(f)["plans"].items() if k.startswith("selftest/")}
    run = subprocess.run([selftest, "--print"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    seen = {}
    for m in re.finditer(r'\{"(\w+)", plan_\w+, \d+, "\w+", \d+, \d+, \d+, \d+, \d+, (\d+), "(\w*)"\}', run.stdout):
        if int(m.group(2)):  # table plans have no specialised source
            seen[m.group(1)] = {"length": int(m.group(2)), "sha256": m.group(3)}
    assert len(golden) == 11 and seen == golden
