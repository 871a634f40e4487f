"""The cache policy of the specialised row kernels' memory stream (pgmpy_amd/csrc/pgmrows_plan.cpp RowsPolicy)
on the CPU: the default policy still emits the pinned source, a streaming policy changes the forms of the
evidence-code loads and of the output stores and nothing else, and every streaming source compiles for
gfx950.  tools/rows_plan_selftest.cpp is the generator stand-alone (its header gives the sanitizer line)."""
import hashlib
import json
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = (1, 2, 3, 4, 5)  # PGM_ROWS_STREAM policy words: bit 0 nontemporal code loads, word >> 1 the store form
STORE_BITS = {0: None, 1: "sc1 nt", 2: "sc0 sc1 nt"}
STORE_AUX = {0: 16, 1: 18, 2: 19}


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("rows_stream") / "rows_plan_selftest")
    csrc = os.path.join(ROOT, "pgmpy_amd", "csrc")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                            os.path.join(ROOT, "tools", "rows_plan_selftest.cpp"),
                            os.path.join(csrc, "pgmrows_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "rows_jit_source.json")) as f:
        return json.load(f)["plans"]


def source_of(selftest, case, word):
    run = subprocess.run([selftest, "--source", case, str(word)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (case, word, run.stderr)
    return run.stdout


def strip_policy(src, word):
    """src with the policy's tokens taken off: the default store macros put back, the hint off the loads."""
    body = src.index('extern "C"')
    pre, rest = src[:body], src[body:]
    bits, aux = STORE_BITS[word >> 1], STORE_AUX[word >> 1]
    if bits is not None:
        for width, ins in ((4, "global_store_dword"), (8, "global_store_dwordx2")):
            asm = ('#define PGM_WT%d(T, p, v) do { const T s_ = (v); asm volatile("%s %%0, %%1, off %s" :: '
                   '"v"((__attribute__((address_space(1))) T *)(p)), "v"(s_) : "memory"); } while (0)\n'
                   % (width, ins, bits))
            assert pre.count(asm) == 1, (word, width)
            pre = pre.replace(asm, "#define PGM_WT4(T, p, v) __hip_atomic_store((__attribute__((address_space(1))) "
                              "T *)(p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)\n" if width == 4
                              else "#define PGM_WT8(T, p, v) PGM_WT4(T, p, v)\n")
        assert pre.count("(int)((off) * 8), 0, %d); }" % aux) == 1
        pre = pre.replace("(int)((off) * 8), 0, %d); }" % aux, "(int)((off) * 8), 0, 16); }")
    if word & 1:
        rest = re.sub(r"__builtin_nontemporal_load\(&(cr\[\d+LL \* ldc\])\)", r"\1", rest)
        rest = re.sub(r"__builtin_nontemporal_load\((\(const unsigned short \*\)\(cr \+ \d+LL \* ldc\))\)", r"*\1", rest)
    assert "__builtin_nontemporal_load" not in rest and " nt" not in pre
    return pre + rest


def test_selftest_with_the_policy_cases(selftest):
    run = subprocess.run([selftest], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "rows_plan_selftest ok" in run.stdout, run.stdout + run.stderr


def test_default_policy_emits_the_golden_sources(selftest, golden):
    """Policy word 0 through the policy-taking generator is, per hand-built plan, the pinned source."""
    cases = {k[len("selftest/"):]: v for k, v in golden.items() if k.startswith("selftest/")}
    assert len(cases) == 11
    for name, g in cases.items():
        src = source_of(selftest, name, 0).encode()
        assert {"length": len(src), "sha256": hashlib.sha256(src).hexdigest()} == g, name


def test_streaming_sources_differ_only_in_load_and_store_forms(selftest, golden):
    """Every policy word on every hand-built plan: the policy's tokens stripped, the text is the default's."""
    for name in sorted(k[len("selftest/"):] for k in golden if k.startswith("selftest/")):
        default = source_of(selftest, name, 0)
        n_loads = len(re.findall(r"(?<![\w(])(?:\*\(const unsigned short \*\)\(cr \+ |cr\[)", default))
        for word in WORDS:
            src = source_of(selftest, name, word)
            assert strip_policy(src, word) == default, (name, word)
            assert src.count("__builtin_nontemporal_load(") == (n_loads if word & 1 else 0), (name, word)
            # the ring's system-scope code loads and the CPT loads are no part of the policy
            assert src.count("__HIP_MEMORY_SCOPE_SYSTEM") == default.count("__HIP_MEMORY_SCOPE_SYSTEM")
            assert src.count("V[") == default.count("V[")


def test_library_streaming_source_of_the_model_plans(monkeypatch):
    """pgm_rows_plan_stream_source on the model plans of the golden file: the shipped policy (switch unset)
    and each word of the switch strip to specialised_source(); word 0 is specialised_source() itself."""
    from tests.test_host_cpu import row_source_plans

    plans = row_source_plans()
    monkeypatch.delenv("PGM_ROWS_STREAM", raising=False)
    for name, plan in plans.items():
        default = plan.specialised_source()
        src, min_rows = plan.streaming_source()
        shipped = next((w for w in WORDS if strip_policy_ok(src, w, default)), None)
        assert (shipped is not None and 0 <= min_rows < 2 ** 63 - 1) or (src == default and min_rows == 2 ** 63 - 1), name
    plan = plans["alarm_3"]
    default = plan.specialised_source()
    for word in (0,) + WORDS:
        monkeypatch.setenv("PGM_ROWS_STREAM", str(word))
        src, min_rows = plan.streaming_source()
        if word == 0:
            assert src == default and min_rows == 2 ** 63 - 1
        else:
            assert src != default and strip_policy(src, word) == default and min_rows == 0, word
        assert plan.specialised_source() == default  # the pinned entry does not see the switch


def strip_policy_ok(src, word, default):
    try:
        return src != default and strip_policy(src, word) == default
    except AssertionError:
        return False


def test_every_streaming_source_compiles(selftest, golden, tmp_path, monkeypatch):
    """Each distinct streaming source compiles for gfx950 (device only), as hipRTC would on the GPU: the
    hand-built plans and the model plans under word 3 (both halves of the policy: nontemporal code loads
    and sc1 nt stores), the model plans under the shipped policy (switch unset), one plan under every word."""
    from tests.test_host_cpu import row_source_plans

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    sources = {}
    for name in sorted(k[len("selftest/"):] for k in golden if k.startswith("selftest/")):
        sources[name + "_3"] = source_of(selftest, name, 3)
    for word in WORDS:
        sources["two_comp_%d" % word] = source_of(selftest, "two_comp", word)
    monkeypatch.setenv("PGM_ROWS_STREAM", "3")
    plans = row_source_plans()
    for name, plan in plans.items():
        sources[name + "_3"] = plan.streaming_source()[0]
    monkeypatch.delenv("PGM_ROWS_STREAM")
    for name, plan in plans.items():
        sources[name + "_shipped"] = plan.streaming_source()[0]
    distinct = {}
    for name, src in sources.items():
        distinct.setdefault(hashlib.sha256(src.encode()).hexdigest(), name)

    def compile_one(name):
        f = tmp_path / (name + ".hip")
        f.write_text("#include <hip/hip_runtime.h>\n" + sources[name])
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "--cuda-device-only", "-c", str(f), "-o",
                            str(tmp_path / (name + ".o"))], capture_output=True, text=True, timeout=300)
        return name, r.returncode, r.stderr[-3000:]

    with ThreadPoolExecutor(max_workers=4) as pool:
        for name, rc, err in pool.map(compile_one, sorted(distinct.values())):
            assert rc == 0, name + "\n" + err
