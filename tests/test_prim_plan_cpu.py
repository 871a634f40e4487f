"""The host side of the primitive factor operations (pgmpy_amd/csrc/pgmprim_plan.cpp: the dim coalescer, the
choice of kernel and geometry, the batch job assembly) without a device: its stand-alone program
(tools/prim_plan_selftest.cpp, plain and under AddressSanitizer + UndefinedBehaviorSanitizer), and the frozen
plan table tests/golden/prim_plan.json, recorded with the library from before the planner moved out of
pgmhip.hip, which the current library has to reproduce field by field."""
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_prim_plan_selftest(tmp_path, flags):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "prim_plan_selftest")
    csrc = os.path.join(ROOT, "pgmpy_amd", "csrc")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "include"), "-I", csrc,
                            os.path.join(ROOT, "tools", "prim_plan_selftest.cpp"),
                            os.path.join(csrc, "pgmprim_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "prim_plan_selftest ok" in run.stdout, run.stdout + run.stderr


def test_plan_unit_has_no_hip():
    with open(os.path.join(ROOT, "pgmpy_amd", "csrc", "pgmprim_plan.cpp")) as f:
        src = f.read()
    with open(os.path.join(ROOT, "pgmpy_amd", "csrc", "pgm_prim.h")) as f:
        src += f.read()
    assert "#include <hip" not in src and "hipLaunch" not in src and "hipMalloc" not in src


@pytest.fixture(scope="module")
def tables():
    spec = importlib.util.spec_from_file_location("make_golden_prim_plan",
                                                  os.path.join(GOLDEN, "make_golden_prim_plan.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from pgmpy_amd import _native as N

    with open(os.path.join(GOLDEN, "prim_plan.json")) as f:
        want = json.load(f)
    return gen, want, gen.table(N)


def _same_rows(name, fields, want, got):
    assert len(want) == len(got), name
    for i, (w, g) in enumerate(zip(want, got)):
        if w == g:
            continue
        if len(w) != len(fields) or len(g) != len(fields):  # one of them a rejection: [status, error text]
            assert w == g, f"{name}[{i}]: recorded {w}, now {g}"
        for f, a, b in zip(fields, w, g):
            assert a == b, f"{name}[{i}].{f}: recorded {a}, now {b} (recorded row {dict(zip(fields, w))})"


def test_binary_plans_are_the_recorded_ones(tables):
    gen, want, got = tables
    assert want["seed"] == got["seed"] and want["binary"]["fields"] == got["binary"]["fields"]
    assert want["binary"]["inputs_sha256"] == got["binary"]["inputs_sha256"], "the generated descriptors changed"
    _same_rows("binary", want["binary"]["fields"], want["binary"]["rows"], got["binary"]["rows"])


def test_nary_plans_are_the_recorded_ones(tables):
    gen, want, got = tables
    assert want["nary"]["fields"] == got["nary"]["fields"]
    assert want["nary"]["inputs_sha256"] == got["nary"]["inputs_sha256"], "the generated descriptors changed"
    _same_rows("nary", want["nary"]["fields"], want["nary"]["rows"], got["nary"]["rows"])


@pytest.mark.parametrize("mode", ["grid", "one_workgroup"])
def test_batch_blocks_are_the_recorded_ones(tables, mode):
    gen, want, got = tables
    assert want["batch"]["fields"] == got["batch"]["fields"]
    assert want["batch"][mode]["inputs_sha256"] == got["batch"][mode]["inputs_sha256"], "the generated jobs changed"
    w, g = want["batch"][mode]["rows"], got["batch"][mode]["rows"]
    assert len(w) == len(g)
    for i, (a, b) in enumerate(zip(w, g)):
        assert a == b, f"batch[{mode}][{i}]: recorded {a}, now {b}"


def test_recorded_table_reaches_every_category(tables):
    """The record is only a proof for what it holds: every kernel, both kinds of split, every lanes-per-output
    value, rejections, and both pair choices of the batch path (a pair job takes half the blocks)."""
    gen, want, _ = tables
    s = gen.summary(want)
    assert s["binary"] >= 2000 and s["binary_rejected"] >= 20 and s["nary"] >= 300 and s["nary_rejected"] >= 10
    assert all(s[f"kernel_{k}"] >= 10 for k in range(4)) and s["split"] >= 100 and s["ri_nb"] >= 20
    assert s["g_log2"] == list(range(7)) and s["nary_g_log2"] == list(range(7))
    for mode in ("grid", "one_workgroup"):
        n, rejected, blocks = s[f"batch_{mode}"]
        assert n >= 500 and rejected >= 5 and blocks > 0
        kinds = {r[0] for r in want["batch"][mode]["rows"]}
        assert kinds == set("cpgn")
    # the single-workgroup mode caps a job's lanes at one block's: fewer blocks than the grid mode in all
    assert s["batch_one_workgroup"][2] < s["batch_grid"][2]
    assert os.path.getsize(os.path.join(GOLDEN, "prim_plan.json")) < 1 << 20
