"""ExpectationMaximization without a GPU: the ABI of pgm_fit_estep, its host argument checks, the host-only
info query, the numpy restatement (tests/em_cases.py) pinned to the reference's goldens
(tests/golden/em_cases.json + .npz), TabularCPD.get_random / get_uniform, and the constructor's and
get_parameters' checks, which run before any compute."""
import ctypes
import logging
import os
import re

import numpy as np
import pandas as pd
import pytest

from tests import em_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META, ARRAYS = C.load_golden()


# ---------------------------------------------------------------------------- ABI
def test_estep_symbols_are_bound_and_the_abi_version_stays():
    from pgmpy_amd import _native as N

    assert "pgm_fit_estep" in N.EXPORTED and "pgm_fit_estep_info" in N.EXPORTED
    lib = N.load_library()
    assert lib.pgm_fit_estep.restype is ctypes.c_int and len(lib.pgm_fit_estep.argtypes) == 12
    assert lib.pgm_fit_estep_info.restype is ctypes.c_int and len(lib.pgm_fit_estep_info.argtypes) == 4
    assert lib.pgm_version() == 25
    assert ctypes.sizeof(N.EmInfo) == 32
    with open(os.path.join(ROOT, "include", "pgmhip.h")) as f:
        header = f.read()
    for name, mine in (("LATENT", N.EM_MAX_LATENT), ("CONFIGS", N.EM_MAX_CONFIGS), ("FAMILIES", N.EM_MAX_FAMILIES)):
        assert int(re.search(rf"#define PGM_EM_MAX_{name} (\d+)", header).group(1)) == mine
    assert float(re.search(r"#define PGM_EM_FLOOR (\S+)", header).group(1)) == N.EM_FLOOR == C.FLOOR


def _i32(xs):
    return (ctypes.c_int32 * max(len(xs), 1))(*xs)


def test_fit_estep_rejects_bad_arguments_on_the_host():
    """pgm_fit_estep validates every argument before any HIP call: PGM_EINVAL, a message, no device."""
    from pgmpy_amd import _native as N
    from pgmpy_amd.estimators._fit import FitPlan

    lib = N.load_library()
    plan = FitPlan([([2], [3]), ([0, 2], [2, 3]), ([1, 2, 0], [3, 3, 2])])
    two_cards = FitPlan([([2], [3]), ([0, 2], [2, 4])])
    big = FitPlan([([j, 4 + j], [2, 9]) for j in range(4)])  # 9^4 = 6,561 configurations
    many = FitPlan([([j, 40], [2, 2]) for j in range(33)])   # 33 families with the latent
    values, tables = np.full(64, 0.5), np.full(64, 7.0)
    codes = np.zeros((2, 16), dtype=np.uint8)
    pv, pc, pt = (a.ctypes.data_as(ctypes.c_void_p) for a in (values, codes, tables))
    ok = (plan._h, _i32([2]), 1, pv, pc, 2, 16, 0, 16, pt, None, None)

    def with_(**kw):
        names = ("plan", "cols", "n", "values", "codes", "n_cols", "ld", "row0", "n_rows", "tables", "loglik", "stream")
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    for args, message in (
            (with_(plan=None), "null plan"),
            (with_(values=None), "null values"),
            (with_(codes=None), "null codes"),
            (with_(tables=None), "null tables"),
            (with_(n=0), "0 latent columns"),
            (with_(cols=_i32(list(range(2, 11))), n=9), "9 latent columns"),
            (with_(cols=_i32([2, 2]), n=2), "latent column 2 is listed twice"),
            (with_(cols=_i32([2, 5]), n=2), "latent column 5 is in no family"),
            (with_(plan=two_cards._h), "latent column 2 has cardinality 4 in family 1 and 3"),
            (with_(plan=big._h, cols=_i32([4, 5, 6, 7]), n=4, n_cols=4), "more than 4096 latent configurations"),
            (with_(plan=many._h, cols=_i32([40]), n_cols=33), "more than 32 families have a latent"),
            (with_(n_cols=1), "observed column 1, codes has 1 columns"),
            (with_(n_rows=-1), "n_rows -1"),
            (with_(row0=-1), "row0 -1"),
            (with_(row0=1), "rows [1, 17) outside ld 16"),
            (with_(ld=8), "outside ld 8")):
        assert lib.pgm_fit_estep(*args) == N.PGM_EINVAL, message
        assert message in N.last_error(), (message, N.last_error())
    assert (tables == 7.0).all()
    # the caps themselves pass: 8 latents, 4,096 configurations, 32 families (host-only query)
    info = N.EmInfo()
    at_cap = FitPlan([([j, 4 + j], [2, 8]) for j in range(4)])
    assert lib.pgm_fit_estep_info(at_cap._h, _i32([4, 5, 6, 7]), 4, ctypes.byref(info)) == N.PGM_OK
    assert info.n_configs == 4096
    at_cap = FitPlan([([j, 40], [2, 2]) for j in range(32)])
    assert lib.pgm_fit_estep_info(at_cap._h, _i32([40]), 1, ctypes.byref(info)) == N.PGM_OK
    assert info.n_latent_families == 32 and info.lds_bytes == 65536
    assert lib.pgm_fit_estep_info(at_cap._h, _i32([40]), 1, None) == N.PGM_EINVAL and "null info" in N.last_error()


def test_estep_info_reports_the_latent_side_and_the_lds_bytes():
    from pgmpy_amd.estimators._fit import FitPlan

    plan = FitPlan([([0], [2]), ([2, 0], [3, 2]), ([1, 2, 3], [2, 3, 4])])  # X0; H1 | X0; X1 | H1, H2
    info = plan.estep_info([2, 3])
    assert (info.n_latent, info.n_configs) == (2, 12)
    assert (info.n_latent_families, info.n_plain_families) == (2, 1)
    assert (info.block, info.rows_per_block) == (plan.info.block, plan.info.rows_per_block) == (256, 4096)
    # the fp64 tile, then one int32 per latent family and work-item
    assert info.lds_bytes == plan.info.tile_bins * 8 + 2 * 256 * 4
    with pytest.raises(ValueError, match="is in no family"):
        plan.estep_info([7])


# ---------------------------------------------------------------------------- the restatement and the goldens
def _restatement(case, key, dtype):
    nodes, families, latent_cols, values, codes, pseudo = C.golden_problem(META, ARRAYS, case)
    c = META[case]
    if key == "converged":
        got, _, n = C.em_ref(families, latent_cols, values, codes, 100, atol=c["atol"], pseudo=pseudo,
                             bayes=pseudo is not None, dtype=dtype)
        assert n == c["n_iter"], (case, n)
    else:
        got, _, _ = C.em_ref(families, latent_cols, values, codes, min(int(key), c["n_iter"]), pseudo=pseudo,
                             bayes=pseudo is not None, dtype=dtype)
    want = np.concatenate([np.asarray(c["results"][key][v], dtype=np.float64) for v in nodes])
    return np.asarray(got, dtype=np.float64), want


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_the_restatement_equals_the_reference(case):
    """em_ref in long double against the reference's CPDs after 1, 3 and 10 iterations and at convergence,
    within 64 d; d is what em_ref in plain fp64 differs by (measured again here: it must not exceed the
    recorded value by more than the 64)."""
    tol = C.golden_tolerance(case)
    for key in ("1", "3", "10", "converged"):
        got, want = _restatement(case, key, np.longdouble)
        assert np.max(np.abs(got - want)) <= tol, (case, key, float(np.max(np.abs(got - want))), tol)
    got, want = _restatement(case, "converged", np.float64)
    print(case, "d measured now:", float(np.max(np.abs(got - want))), "recorded:", C.GOLDEN_D[case])
    assert np.max(np.abs(got - want)) <= tol


def test_the_log_likelihood_of_the_restatement_does_not_decrease():
    for case in ("a", "c"):
        _, families, latent_cols, values, codes, _ = C.golden_problem(META, ARRAYS, case)
        _, lls, _ = C.em_ref(families, latent_cols, values, codes, 10)
        slack = float(np.sum(C.bound_loglik(len(families), 6, np.full(codes.shape[1], lls[0] / codes.shape[1]))))
        assert all(b >= a - slack for a, b in zip(lls, lls[1:])), lls


# ---------------------------------------------------------------------------- get_random / get_uniform
def test_get_random_and_get_uniform_equal_the_reference():
    from pgmpy_amd.factors.discrete import TabularCPD

    assert len(META["e"]) == 9
    for c in META["e"]:
        fn = TabularCPD.get_random if c["kind"] == "random" else TabularCPD.get_uniform
        cpd = fn(variable="A", evidence=c["evidence"], cardinality=c["cardinality"], seed=c["seed"])
        assert list(cpd.variables) == c["variables"]
        want = np.asarray(c["values"])
        assert cpd.get_values().shape == want.shape
        assert np.max(np.abs(np.asarray(cpd.get_values()) - want)) <= 1e-15, c
    with pytest.raises(ValueError, match="Cardinality for variable: B not specified"):
        TabularCPD.get_random("A", evidence=["B"], cardinality={"A": 2})
    with pytest.raises(ValueError, match="Cardinality for variable: A not specified"):
        TabularCPD.get_uniform("A", cardinality={})
    named = TabularCPD.get_uniform("A", ["B"], {"A": 2, "B": 3}, state_names={"A": ["n", "y"], "B": ["x", "y", "z"]})
    assert named.state_names == {"A": ["n", "y"], "B": ["x", "y", "z"]} and named.is_valid_cpd()


# ---------------------------------------------------------------------------- the constructor
def _frame_f():
    f = META["f"]
    return pd.DataFrame({c: [np.nan if x is None else x for x in col] for c, col in f["frame"].items()})


def test_the_constructor_keeps_the_reference_rows_and_latents(caplog):
    from pgmpy_amd.estimators import ExpectationMaximization
    from pgmpy_amd.models import DiscreteBayesianNetwork

    f = META["f"]
    model = DiscreteBayesianNetwork([tuple(e) for e in f["edges"]], latents=set(f["declared_latents"]))
    with caplog.at_level(logging.WARNING, logger="pgmpy"):
        est = ExpectationMaximization(model, _frame_f())
    assert [int(i) for i in est.data.index] == f["kept_rows"] and len(f["kept_rows"]) == 37
    assert list(est.data.columns) == f["columns"] == ["A", "B", "C"]
    # the reference keeps the declared latent only: it warns about H, then loses the update (its `latents`
    # property hands out a copy) and cannot estimate; here the all-NaN column is latent, as the warning says
    assert f["latents"] == ["G"] and f["all_nan"] == ["H"]
    assert sorted(est.model.latents) == sorted(f["latents"] + f["all_nan"])
    assert {v: [float(s) for s in est.state_names[v]] for v in est.data.columns} == f["state_names"]
    assert "Treating them as latent variables" in caplog.text and "3 rows with missing values" in caplog.text


def test_argument_errors_come_before_any_compute():
    """No device here: every one of these must be raised by the checks, not by the missing GPU."""
    from pgmpy_amd.estimators import ExpectationMaximization
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.models import DiscreteBayesianNetwork, DiscreteMarkovNetwork

    df = pd.DataFrame({"A": [0, 1, 1, 0], "B": [0, 1, 2, 1]})
    with pytest.raises(NotImplementedError, match="only implemented for DAG or DiscreteBayesianNetwork"):
        ExpectationMaximization(DiscreteMarkovNetwork([("A", "B")]), df)
    model = DiscreteBayesianNetwork([("H", "A"), ("H", "B")], latents={"H"})
    est = ExpectationMaximization(model, df)
    with pytest.raises(ValueError, match="must be either 'random' or 'uniform'. Got: zeros"):
        est.get_parameters(init_cpds="zeros")
    with pytest.raises(ValueError, match="max_iter"):
        est.get_parameters(max_iter=0)
    with pytest.raises(ValueError, match="atol"):
        est.get_parameters(atol=-1.0)
    with pytest.raises(ValueError, match="latent_card"):
        est.get_parameters(latent_card={})
    with pytest.raises(ValueError, match="latent_card"):
        est.get_parameters(latent_card={"H": 0})
    with pytest.raises(TypeError, match="unexpected keyword argument 'prior_type'"):
        est.get_parameters(prior_type="K2")
    with pytest.raises(TypeError, match="unexpected keyword argument 'prior'"):
        est.get_parameters(apply_smoothing=True, prior="K2")
    with pytest.raises(ValueError, match="'prior_type' not specified"):
        est.get_parameters(apply_smoothing=True, prior_type="bogus")
    with pytest.raises(ValueError, match="not in the model"):
        est.get_parameters(init_cpds={"Q": TabularCPD("Q", 2, [[0.5], [0.5]])})
    with pytest.raises(ValueError, match="must be the CPD of A given its parents"):
        est.get_parameters(init_cpds={"A": TabularCPD("A", 2, [[0.5], [0.5]])})
    with pytest.raises(ValueError, match="H has 3 states, the estimator has 2"):
        est.get_parameters(init_cpds={"A": TabularCPD("A", 2, np.full((2, 3), 0.5), ["H"], [3])})
    with pytest.raises(ValueError, match="more than 4096 latent configurations"):
        ExpectationMaximization(DiscreteBayesianNetwork([("H", "A"), ("G", "A"), ("G", "B")], latents={"H", "G"}),
                                df).get_parameters(latent_card={"H": 100, "G": 100})
    with pytest.raises(ValueError, match="neither latent nor present in the dataset"):
        ExpectationMaximization(DiscreteBayesianNetwork([("H", "A"), ("H", "Q")], latents={"H"}), df).get_parameters()
    with pytest.raises(ValueError, match="no latent variable"):
        ExpectationMaximization(DiscreteBayesianNetwork([("A", "B")]), df).get_parameters()
    # fit() hands any BaseEstimator subclass its keyword arguments: the same checks, the same errors
    with pytest.raises(ValueError, match="must be either 'random' or 'uniform'"):
        model.fit(df, estimator=ExpectationMaximization, init_cpds="zeros")
