"""The generators of the specialised batched-BP steps and contraction batches (pgmpy_amd/csrc/pgmpm_gen.cpp:
planner, specialisation choice, source of the fused / two-marginal / merged steps and of the batches) as a
stand-alone CPU program over hand-built descriptors (tools/pm_gen_selftest.cpp; its header gives the
sanitizer build line).  tests/golden/pm_source.json pins every emission branch's source."""
import hashlib
import json
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("pm_gen") / "pm_gen_selftest")
    csrc = os.path.join(ROOT, "pgmpy_amd", "csrc")
    # no HIP include path, and no warning from the generator unit: it stays plain C++17
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                            "-I", csrc, os.path.join(ROOT, "tools", "pm_gen_selftest.cpp"),
                            os.path.join(csrc, "pgmpm_gen.cpp"), os.path.join(csrc, "pgmrows_plan.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0 and "pgmpm_gen.cpp" not in built.stderr, built.stderr
    return exe


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "pm_source.json")) as f:
        return json.load(f)["cases"]


def test_pm_gen_selftest(selftest):
    run = subprocess.run([selftest], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "pm_gen_selftest ok" in run.stdout, run.stdout + run.stderr


def test_generator_unit_has_no_hip_include():
    for name in ("pgmpm_gen.cpp", "pgm_pm.h"):
        with open(os.path.join(ROOT, "pgmpy_amd", "csrc", name)) as f:
            assert "hip/" not in f.read(), name


def test_sources_are_the_golden_ones(selftest, golden, tmp_path):
    """The self-test's recorded hashes and tests/golden/pm_source.json say the same, the generator still
    emits them, and the dumped files are those sources."""
    run = subprocess.run([selftest, "--dump", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    seen = {m.group(1): {"length": int(m.group(2)), "sha256": m.group(3)}
            for m in re.finditer(r'\{"(\w+)", (\d+), "([\w-]+)"\}', run.stdout)}
    assert len(golden) == 30 and seen == golden
    with open(os.path.join(ROOT, "tools", "pm_gen_selftest.cpp")) as f:
        table = f.read().split("kGolden[] = {")[1].split("};")[0]
    recorded = {m.group(1): {"length": int(m.group(2)), "sha256": m.group(3)}
                for m in re.finditer(r'\{"(\w+)", (\d+), "([\w-]+)"\}', table)}
    assert recorded == golden
    for name, g in golden.items():
        path = tmp_path / (name + ".hip")
        assert path.exists() == (g["length"] > 0), name
        if g["length"]:
            assert hashlib.sha256(path.read_bytes()).hexdigest() == g["sha256"], name


def test_every_golden_source_compiles(selftest, golden, tmp_path):
    """Each distinct source of the golden file compiles for gfx950 (device only), as hipRTC would on the GPU."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    run = subprocess.run([selftest, "--dump", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    distinct = {}
    for name, g in golden.items():
        if g["length"]:
            distinct.setdefault(g["sha256"], name)
    assert len(distinct) == 22

    def compile_one(name):
        f = tmp_path / (name + "_cc.hip")
        f.write_text("#include <hip/hip_runtime.h>\n" + (tmp_path / (name + ".hip")).read_text())
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "--cuda-device-only", "-c", str(f), "-o",
                            str(tmp_path / (name + ".o"))], capture_output=True, text=True, timeout=300)
        return name, r.returncode, r.stderr[-3000:]

    with ThreadPoolExecutor(max_workers=4) as pool:
        for name, rc, err in pool.map(compile_one, sorted(distinct.values())):
            assert rc == 0, name + "\n" + err
