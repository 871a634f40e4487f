"""The per-row log-probability without a device: the exported symbols, every host argument check of
pgm_fit_log_values / pgm_fit_logprob (they run before any HIP call, so they answer here), the launch
geometry pgm_fit_logprob_info reports, the long-double restatement (tests/logp_cases.py) against values
recorded from the reference (tests/golden/make_golden_metrics.py), the host-only metrics (SHD,
is_dconnected, the closed-form chi-square survival function, the F1) against recorded values, and the
errors the metrics raise before they need the device."""
import ctypes
import json
import os

import numpy as np
import pandas as pd
import pytest

from tests import logp_cases as LC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL = -1
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "metrics_cases.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "metrics_cases.npz"))


def net5(meta, edges=None):
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.models import DiscreteBayesianNetwork

    m = DiscreteBayesianNetwork([tuple(e) for e in (meta["edges"] if edges is None else edges)])
    m.add_nodes_from(meta["nodes"])
    if edges is None:
        states = meta["states"]
        for v in meta["nodes"]:
            variables = meta["cpds"][v]["variables"]
            m.add_cpds(TabularCPD(v, len(states[v]), meta["cpds"][v]["values"], evidence=variables[1:] or None,
                                  evidence_card=[len(states[u]) for u in variables[1:]] or None,
                                  state_names={u: states[u] for u in variables}))
    return m


def frame(meta, codes, columns=None):
    nodes = meta["nodes"]
    df = pd.DataFrame({v: np.asarray(meta["states"][v], dtype=object)[codes[i]] for i, v in enumerate(nodes)})
    return df[list(columns)] if columns is not None else df


# ---------------------------------------------------------------------------- the C-ABI
def test_new_symbols_are_bound_and_the_abi_version_stays():
    from pgmpy_amd import _native as N

    for name in ("pgm_fit_log_values", "pgm_fit_logprob", "pgm_fit_logprob_info"):
        assert name in N.EXPORTED and hasattr(N.load_library(), name)
    assert N.load_library().pgm_version() == 25
    assert (N.LOGP_BLOCK, N.LOGP_ROWS_PER_BLOCK) == (LC.BLOCK, LC.ROWS_PER_BLOCK)


def _plan():
    from pgmpy_amd.estimators._fit import FitPlan

    return FitPlan([([3], [2]), ([0, 3], [3, 2]), ([2, 3], [4, 2]), ([1, 0, 2], [2, 3, 4])])  # reads columns 0 .. 3


def _logprob(plan, logv=0x1000, codes=0x2000, n_cols=4, ld=64, row0=0, n_rows=64, logp=0x3000, total=0x4000,
             skipped=0x5000, handle=True):
    from pgmpy_amd import _native as N

    return N.load_library().pgm_fit_logprob(plan._h if handle else None, P(logv), P(codes), n_cols, ld, row0, n_rows,
                                            P(logp), P(total), P(skipped), None)


@pytest.mark.parametrize("kwargs,message", [
    (dict(handle=False), "null plan"),
    (dict(logv=None), "null logv"),
    (dict(codes=None), "null codes"),
    (dict(logv=0x1004), "8-byte aligned"),
    (dict(logp=0x3004), "8-byte aligned"),
    (dict(total=0x4002), "8-byte aligned"),
    (dict(skipped=0x5004), "8-byte aligned"),
    (dict(n_cols=3), "the plan reads column 3, codes has 3 columns"),
    (dict(n_rows=-1), "n_rows -1"),
    (dict(row0=-4), "row0 -4"),
    (dict(ld=-8, n_rows=0), r"outside ld -8"),
    (dict(n_rows=65), r"rows \[0, 65\) outside ld 64"),
    (dict(row0=1), r"rows \[1, 65\) outside ld 64"),
    (dict(ld=2 ** 40, n_rows=LC.ROWS_PER_BLOCK * 65536 + 1), "score the rows in several calls"),
])
def test_logprob_argument_checks_need_no_device(kwargs, message):
    """Every argument of pgm_fit_logprob is checked on the host before any HIP call: the fake addresses are
    never touched and the answer is PGM_EINVAL with a message, with or without a device."""
    import re

    from pgmpy_amd import _native as N

    plan = _plan()
    assert _logprob(plan, **kwargs) == EINVAL
    assert re.search(message, N.last_error()), N.last_error()


def test_log_values_argument_checks_need_no_device():
    from pgmpy_amd import _native as N

    L = N.load_library()
    plan = _plan()
    for args, message in (((None, P(0x1000), P(0x1000)), "null plan"), ((plan._h, None, P(0x1000)), "null values"),
                          ((plan._h, P(0x1000), None), "null logv"), ((plan._h, P(0x1004), P(0x1000)), "8-byte aligned"),
                          ((plan._h, P(0x1000), P(0x1001)), "8-byte aligned")):
        assert L.pgm_fit_log_values(*args, None) == EINVAL
        assert message in N.last_error(), N.last_error()


def test_logprob_info_geometry():
    from pgmpy_amd import _native as N

    plan = _plan()
    for codes, ld, row0, vec4 in [(0x1000, 64, 0, 1), (0x1000, 64, 4, 1), (0x1004, 8, 4, 1), (0x1000, 64, 1, 0),
                                  (0x1000, 63, 0, 0), (0x1002, 64, 0, 0), (0x1001, 63, 3, 0), (None, 64, 0, 0)]:
        i = plan.logprob_info(codes, ld, row0)
        assert (i.block, i.rows_per_block, i.vec4, i.n_families) == (256, 1024, vec4, 4), (codes, ld, row0)
    R = LC.ROWS_PER_BLOCK
    for n, parts in [(0, 0), (1, 1), (R - 1, 1), (R, 1), (R + 1, 2), (2 * R + 3, 3), (10 ** 6, 977)]:
        assert plan.logprob_info(0x1000, 2 ** 21, 0, n).n_partials == parts
    with pytest.raises(ValueError, match=r"rows \[4, 70\) outside ld 64"):
        plan.logprob_info(0x1000, 64, 4, 66)
    assert N.load_library().pgm_fit_logprob_info(plan._h, P(0x1000), 64, 0, 64, None) == EINVAL


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_logp_plan_selftest(tmp_path, flags):
    """The same checks from C++, as a stand-alone host program (tools/logp_plan_selftest.cpp), plain and under
    AddressSanitizer + UndefinedBehaviorSanitizer."""
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(GOLDEN))
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "logp_plan_selftest")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", *flags, "-I", os.path.join(root, "include"),
                            "-I", os.path.join(root, "pgmpy_amd", "csrc"), os.path.join(root, "tools", "logp_plan_selftest.cpp"),
                            os.path.join(root, "pgmpy_amd", "csrc", "pgmfit_plan.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "logp_plan_selftest ok" in run.stdout, run.stdout + run.stderr


# ---------------------------------------------------------------------------- the restatement
def test_restatement_matches_the_reference_on_net5(golden):
    """The long-double restatement against BayesianModelProbability.log_probability recorded from the
    reference (fp64 logs added node by node): twice the row bound, as both sides round."""
    meta, arrays = golden
    from tests import sample_cases as S

    _, _, fams, tables = S.model_plan(net5(meta))
    codes = arrays["net5_codes200"]
    got, exact, mag, skipped, invalid = LC.restate(fams, tables, codes)
    assert not skipped.any() and not invalid
    want = arrays["net5_logp200"]
    assert (np.abs(exact - want.astype(np.longdouble)) <= 2 * LC.row_bound(len(fams), mag)).all()
    assert abs(float(np.sum(exact)) - meta["score200"]) <= 2 * float(LC.row_bound(len(fams), mag).sum()) + 200 * 2.0 ** -53 * abs(meta["score200"])
    assert meta["score200"] == meta["loglik200"]


def test_restatement_matches_the_reference_on_alarm(golden):
    """The reference divides every column of a node with parents by its total (sampling/base.py:98); alarm's
    HREKG and HRSAT columns sum to 0.9999999 in the file, so the restatement runs on the normalised tables."""
    meta, arrays = golden
    fams, tables = LC.plan("alarm")
    assert max(abs(t.sum(axis=0) - 1).max() for t in tables) > 5e-8
    tables = LC.normalized(tables)
    codes = np.load(os.path.join(GOLDEN, "fit_alarm.npz"))["codes"]
    _, exact, mag, skipped, invalid = LC.restate(fams, tables, codes)
    assert not skipped.any() and not invalid
    want = arrays["alarm_logp"]
    assert want.shape == (1000,)
    assert (np.abs(exact - want.astype(np.longdouble)) <= 2 * LC.row_bound(len(fams), mag)).all()


def test_restatement_edge_cases():
    fams, tables = [([0], [2]), ([1, 0], [3, 2])], [np.array([[0.25], [0.75]]), np.array([[0.5, 0.0], [0.25, 1.0], [0.25, 0.0]])]
    codes = np.array([[0, 1, 1, 255, 0, 2], [2, 1, 0, 1, 255, 0]], dtype=np.uint8)
    got, _, _, skipped, invalid = LC.restate(fams, tables, codes)
    assert got[0] == np.float64(np.log(np.longdouble(0.25)) + np.log(np.longdouble(0.25)))
    assert got[1] == np.float64(np.log(np.longdouble(0.75))) and got[2] == -np.inf
    assert np.isnan(got[3:]).all() and skipped.tolist() == [False, False, False, True, True, True] and invalid
    assert LC.total_fixed_order(got[:2]) == got[0] + got[1]
    assert LC.total_fixed_order(got) == -np.inf and LC.total_fixed_order([]) == 0.0


def test_total_fixed_order_is_the_documented_tree():
    """2 * 1024 + 3 rows by hand: strided sums per work-item, the halving tree, then the three partials."""
    rng = np.random.default_rng(3)
    v = -rng.random(2 * 1024 + 3) * 40
    parts = []
    for b in range(3):
        blk = np.zeros(1024)
        chunk = v[b * 1024:(b + 1) * 1024]
        blk[:len(chunk)] = chunk
        item = [((blk[t] + blk[t + 256]) + blk[t + 512]) + blk[t + 768] for t in range(256)]
        w = 128
        while w:
            item = [item[t] + item[t + w] for t in range(w)] + item[w:]
            w //= 2
        parts.append(item[0])
    item = parts + [0.0] * 253
    w = 128
    while w:
        item = [item[t] + item[t + w] for t in range(w)] + item[w:]
        w //= 2
    assert LC.total_fixed_order(v) == item[0]


# ---------------------------------------------------------------------------- host-only metrics
def test_shd_and_dconnection_match_the_reference(golden):
    from pgmpy_amd.metrics import SHD

    meta, _ = golden
    true = net5(meta)
    for name, case in meta["dags"].items():
        dag = net5(meta, case["edges"])
        assert SHD(true, dag) == case["shd_to_true"] == SHD(dag, true)
        for u, v, z, want in case["dconnected"]:
            assert dag.is_dconnected(u, v, observed=z) == want, (name, u, v, z)
            assert dag.is_dconnected(v, u, observed=z or None) == want
    assert SHD(true, net5(meta, meta["shd_reversed"]["edges"])) == meta["shd_reversed"]["shd"] == 2
    assert meta["dags"]["pruned"]["shd_to_true"] == 2
    with pytest.raises(ValueError, match="The graphs must have the same nodes"):
        SHD(true, net5({"nodes": ["A", "B"], "edges": [["A", "B"]]}, [["A", "B"]]))


def test_chi2_sf_closed_form_against_scipy(golden):
    """exp(-x) sum_{i<k} x^i / i! against scipy.stats.chi2.sf recorded at k = 1, 7, 500 and 5,000.  The
    closed form is evaluated in long double (error far below 2^-53 relative); scipy's regularised
    incomplete gamma is the less exact side: 1e-11 relative leaves two to three decimal digits over the
    1e-13 .. 1e-14 its large-argument expansions reach."""
    from pgmpy_amd.metrics import chi2_sf_even

    meta, _ = golden
    assert {c["k"] for c in meta["chi2_sf"]} == {1, 7, 500, 5000}
    for c in meta["chi2_sf"]:
        got = chi2_sf_even(c["C"], c["k"])
        print(c["k"], c["C"], got, c["sf"], abs(got - c["sf"]) / c["sf"])
        assert 0.0 < c["sf"] <= 1.0 and abs(got - c["sf"]) <= 1e-11 * c["sf"], c
    assert chi2_sf_even(0.0, 3) == 1.0 and chi2_sf_even(2.0, 1) == float(np.exp(np.longdouble(-1.0)))
    assert np.isnan(chi2_sf_even(1.0, 0))


def test_f1_is_the_binary_f1_of_the_positive_class(golden):
    from pgmpy_amd.metrics import f1_score

    meta, _ = golden
    for case in meta["dags"].values():
        assert f1_score(y_true=case["summary"]["stat_test"], y_pred=case["summary"]["d_connected"]) == pytest.approx(case["f1"], abs=1e-15)
    assert f1_score([False, False], [False, True]) == 0.0 and f1_score([True, False], [False, False]) == 0.0
    assert f1_score([True, True, False, False], [True, False, True, False]) == 0.5


# ---------------------------------------------------------------------------- errors before the device
def _latent_model():
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.models import DiscreteBayesianNetwork

    m = DiscreteBayesianNetwork([("L", "X")], latents={"L"})
    m.add_cpds(TabularCPD("L", 2, [[0.5], [0.5]]), TabularCPD("X", 2, [[0.9, 0.2], [0.1, 0.8]], ["L"], [2]))
    return m


def test_metric_value_errors(golden):
    from pgmpy_amd import metrics as M

    meta, arrays = golden
    m = net5(meta)
    df = frame(meta, arrays["net5_codes200"])
    with pytest.raises(TypeError, match="Model expected type: DiscreteBayesianNetwork"):
        M.BayesianModelProbability(object())
    with pytest.raises(ValueError, match="without latent variables"):
        M.BayesianModelProbability(_latent_model())
    with pytest.raises(ValueError, match="data has 5 columns, ordering names 4"):
        M.BayesianModelProbability(m).log_probability(df.values, ordering=list(df.columns)[:4])
    with pytest.raises(ValueError, match="no column for the variables"):
        M.BayesianModelProbability(m).log_probability(df.drop(columns=["B"]))
    for fn in (M.log_likelihood_score, M.correlation_score):
        with pytest.raises(ValueError, match="must be a DiscreteBayesianNetwork"):
            fn(object(), df)
        with pytest.raises(ValueError, match="data must be a pandas.DataFrame instance"):
            fn(m, df.values)
        with pytest.raises(ValueError, match="Missing columns in data"):
            fn(m, df.drop(columns=["B"]))
    with pytest.raises(ValueError, match="must either be one of"):
        M.correlation_score(m, df, test="no_such_test")
    with pytest.raises(ValueError, match="score should be a classification metric"):
        M.correlation_score(m, df, score=3)
    with pytest.raises(ValueError, match="must be an instance of DiscreteBayesianNetwork"):
        M.fisher_c(object(), df, "chi_square")
    with pytest.raises(ValueError, match="can not be performed on models with latent variables"):
        M.fisher_c(_latent_model(), df, "chi_square")
    with pytest.raises(ValueError):  # check_model: a node without a CPD
        M.log_likelihood_score(net5(meta, meta["edges"]), df)
    assert "implied_cis" not in M.__all__ and not hasattr(M, "implied_cis")


def test_callable_tests_need_no_device(golden):
    """A callable test is called pair by pair with the reference's keywords; the default score is the F1."""
    from pgmpy_amd import metrics as M

    meta, arrays = golden
    m = net5(meta)
    df = frame(meta, arrays["net5_codes200"])
    case = meta["dags"]["true"]
    answers = {(u, v): s for u, v, s in zip(case["summary"]["var1"], case["summary"]["var2"], case["summary"]["stat_test"])}
    calls = []

    def test(X, Y, Z, data, boolean, significance_level):
        calls.append((X, Y, list(Z), boolean, significance_level))
        return answers[(X, Y)] if (X, Y) in answers else answers[(Y, X)]

    summary = M.correlation_score(m, df, test=test, significance_level=0.05, return_summary=True)
    assert list(summary.columns) == ["var1", "var2", "stat_test", "d_connected"] and len(calls) == 10
    assert all(c[2:] == ([], True, 0.05) for c in calls)
    by_pair = {frozenset(p): d for p, d in zip(zip(case["summary"]["var1"], case["summary"]["var2"]), case["summary"]["d_connected"])}
    assert all(by_pair[frozenset((u, v))] == d for u, v, d in zip(summary["var1"], summary["var2"], summary["d_connected"]))
    assert M.correlation_score(m, df, test=test) == pytest.approx(case["f1"], abs=1e-15)
    assert M.correlation_score(m, df, test=test, score=lambda y_true, y_pred: int(np.sum(y_true == y_pred))) == 9

    seen = []

    def ci(X, Y, Z, data, boolean):
        seen.append((X, Y, frozenset(Z)))
        return 1.0, 0.5, 1

    p, rmsea = M.fisher_c(m, df, ci, compute_rmsea=True, show_progress=False)
    pairs = {(u, v): frozenset(m.get_parents(u)) | frozenset(m.get_parents(v)) for u, v, _ in seen}
    assert len(seen) == 5 and all(z == pairs[(u, v)] for u, v, z in seen)
    C = -2 * 5 * np.log(0.5)
    assert p == pytest.approx(M.chi2_sf_even(C, 5), rel=1e-15) and rmsea == 0.0


def test_device_metrics_raise_native_unavailable_without_gpu(golden):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pgmpy_amd import metrics as M
    from pgmpy_amd._native import NativeUnavailable

    meta, arrays = golden
    m = net5(meta)
    df = frame(meta, arrays["net5_codes200"])
    bmp = M.BayesianModelProbability(m)
    for call in (lambda: bmp.log_probability(df), lambda: bmp.score(df),
                 lambda: bmp.log_probability(df.values, ordering=list(df.columns)),
                 lambda: bmp.log_probability_codes(torch.zeros((5, 8), dtype=torch.uint8)),
                 lambda: M.log_likelihood_score(m, df), lambda: M.correlation_score(m, df),
                 lambda: M.fisher_c(m, df, "chi_square", show_progress=False)):
        with pytest.raises(NativeUnavailable):
            call()
