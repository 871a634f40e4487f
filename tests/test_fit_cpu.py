"""Parameter learning without a GPU: the numpy restatement against the reference's goldens, the host plan
unit (tools/fit_plan_selftest.cpp over pgmpy_amd/csrc/pgmfit_plan.cpp), the argument checks of the
pgm_fit_* entry points, the estimators' constructor errors, and no compute without a device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

from tests import fit_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, ALARM = F.load_golden()
RUNS = F.golden_runs(CASES)


# ---------------------------------------------------------------------------- restatement == reference
@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_restatement_reproduces_golden(run):
    """count_ref / finish_ref over host-encoded codes give the reference's state_counts tables (exact;
    weighted sums at rtol 1e-12: the order of addition differs) and CPDs (MLE exact: count / sum is one
    rounded division; rtol 1e-12 where pseudo-counts or weights are floats)."""
    _, case, key, est, kwargs, state_names, weighted = run
    got = F.restate_run(case, est, kwargs, state_names, weighted)
    for n in case["nodes"]:
        counts, values = got[n]
        want_c = np.asarray(case[key]["counts"][n]["values"], dtype=np.float64)
        want_v = np.asarray(case[key]["cpds"][n]["values"], dtype=np.float64)
        if weighted:
            np.testing.assert_allclose(counts, want_c, rtol=1e-12, atol=0)
        else:
            assert np.array_equal(counts, want_c), n
        if est == "mle" and not weighted:
            assert np.array_equal(values, want_v, equal_nan=True), n
        else:
            np.testing.assert_allclose(values, want_v, rtol=1e-12, atol=0, equal_nan=True)


def test_restatement_reproduces_issue_values():
    """The docstring frame's C: MLE [[0,0,1,.5],[1,1,0,.5]] (one unseen parent column, filled
    uniformly), BDeu(5) [[.2778,.2778,.7222,.5], ...]."""
    a = CASES["a"]
    mle = F.restate_run(a, "mle", {}, None, False)["C"][1]
    assert np.array_equal(mle, [[0, 0, 1, .5], [1, 1, 0, .5]])
    bdeu = F.restate_run(a, "bayes", {"prior_type": "BDeu", "equivalent_sample_size": 5}, None, False)["C"][1]
    np.testing.assert_allclose(bdeu[0], [.2778, .2778, .7222, .5], atol=5e-5)
    np.testing.assert_allclose(np.asarray(a["fit_update10"]["C"]["values"])[0], [.2525, .2525, .7475, .5], atol=5e-5)


@pytest.mark.parametrize("name", ["mle", "bdeu5", "mle_first", "mle_second"])
def test_restatement_reproduces_alarm_golden(name):
    """Case (e): all 37 alarm families over the 1,000 recorded rows (and each half)."""
    from pgmpy_amd.utils import get_example_model

    m = get_example_model("alarm")
    nodes = sorted(m.nodes())
    fams = F.alarm_families(m, nodes)
    codes = ALARM["codes"]
    rows = {"mle_first": slice(0, 500), "mle_second": slice(500, 1000)}.get(name, slice(0, 1000))
    counts = F.count_ref(codes[:, rows], fams)
    assert np.array_equal(counts, ALARM[f"{name}_counts"])
    if name == "bdeu5":
        values = F.finish_ref(counts, fams, pseudo=F.pseudo_ref(fams, "bdeu", 5), bayes=True)
        np.testing.assert_allclose(values, ALARM["bdeu5_values"], rtol=1e-12, atol=0)
    else:
        assert np.array_equal(F.finish_ref(counts, fams), ALARM[f"{name}_values"])


def test_skip_rule_is_per_family():
    """A row with 255 in a column is skipped only by the families that read the column; a code that is
    not a state raises IndexError."""
    codes = np.array([[0, 1, 255, 1], [1, 255, 0, 1], [0, 0, 0, 255]], dtype=np.uint8)
    fams = [([0], [2]), ([2, 0, 1], [2, 2, 2])]
    c = F.count_ref(codes, fams)
    assert c[:2].tolist() == [1, 2] and c[2:].sum() == 1 and c[2 + 0 * 4 + 0 * 2 + 1] == 1
    codes[0, 0] = 2
    with pytest.raises(IndexError):
        F.count_ref(codes, fams)


# ---------------------------------------------------------------------------- the host plan unit
@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("fit_plan") / "fit_plan_selftest")
    csrc = os.path.join(ROOT, "pgmpy_amd", "csrc")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                            os.path.join(ROOT, "tools", "fit_plan_selftest.cpp"),
                            os.path.join(csrc, "pgmfit_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def test_fit_plan_selftest(selftest):
    run = subprocess.run([selftest], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "fit_plan_selftest ok" in run.stdout, run.stdout + run.stderr


HAND_FAMILIES = [
    ([4], [3]),                                                        # no parents
    ([2, 0, 1], [2, 3, 4]),
    (list(range(32)), [3] + [2] * 10 + [1] * 21),                       # the maximum number of parents
    ([0, 1], [254, 1]), ([1, 0], [1, 254]),                             # cardinalities 1 and 254
    ([0, 1], [17, 241]),                                                # larger than the tile
    ([3], [5]),
]


def test_host_plan_layout_equals_restatement(selftest, tmp_path):
    """Offsets, sizes and strides of hand-built families from the host unit (stand-alone program) and
    from the library's pgm_fit_plan_info equal the restatement's layout()."""
    from pgmpy_amd.estimators._fit import FitPlan

    offsets, sizes, strides = F.layout(HAND_FAMILIES)
    spec = tmp_path / "families.txt"
    spec.write_text("".join(" ".join(f"{c}:{k}" for c, k in zip(cols, cards)) + "\n" for cols, cards in HAND_FAMILIES))
    run = subprocess.run([selftest, "--print", str(spec)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == len(HAND_FAMILIES) + 1
    for f, line in enumerate(lines[:-1]):
        w = line.split()
        assert (int(w[3]), int(w[5])) == (offsets[f], sizes[f]) and [int(x) for x in w[9:]] == strides[f], line
    columns = sum(s // cards[0] for s, (_, cards) in zip(sizes, HAND_FAMILIES))
    assert lines[-1].split()[:4] == ["total", str(offsets[-1] + sizes[-1]), "columns", str(columns)]
    plan = FitPlan(HAND_FAMILIES)
    assert (plan.offsets, plan.sizes, plan.strides) == (offsets, sizes, strides)
    assert plan.total_bins == offsets[-1] + sizes[-1] and plan.info.total_columns == columns
    assert plan.info.n_cols == 32 and plan.info.tile_bins == 4096 and plan.info.n_families == len(HAND_FAMILIES)
    # [0..4] share a tile (3,607 bins), the 4,097-bin family is a group of its own, then the last
    assert plan.groups == [0, 0, 0, 0, 0, 1, 2] and plan.info.n_groups == 3
    # too many parents and a non-positive cardinality: PGM_EINVAL from the unit
    for bad in ("0:2 " * 33, "0:2 1:0", "0:-1"):
        spec.write_text(bad + "\n")
        run = subprocess.run([selftest, "--print", str(spec)], capture_output=True, text=True, timeout=120)
        assert run.stdout.startswith("error -1 fit_plan_create: family 0"), run.stdout


def _families(N, fams):
    arr = (N.FitFamily * len(fams))()
    for f, (cols, cards) in enumerate(fams):
        arr[f].n_vars = len(cols)
        for v, (c, k) in enumerate(zip(cols[:N.PGM_MAX_DIMS], cards[:N.PGM_MAX_DIMS])):
            arr[f].col[v], arr[f].card[v] = c, k
    return arr


def test_fit_entry_points_reject_bad_arguments_on_the_host():
    """pgm_fit_* validate every argument before any HIP call: PGM_EINVAL with no device present."""
    from pgmpy_amd import _native as N

    lib = N.load_library()
    h = ctypes.c_void_p()
    EINVAL = N.PGM_EINVAL
    assert lib.pgm_fit_plan_create(None, 1, ctypes.byref(h)) == EINVAL
    assert lib.pgm_fit_plan_create(_families(N, [([0], [2])]), 1, None) == EINVAL
    assert lib.pgm_fit_plan_create(_families(N, [([0], [2])]), 0, ctypes.byref(h)) == EINVAL
    assert lib.pgm_fit_plan_create(_families(N, [(list(range(33)), [2] * 33)]), 1, ctypes.byref(h)) == EINVAL
    assert "33 variables" in N.last_error()
    assert lib.pgm_fit_plan_create(_families(N, [([0, 1], [2, 0])]), 1, ctypes.byref(h)) == EINVAL and not h.value
    assert lib.pgm_fit_plan_create(_families(N, [([0], [3]), ([2, 0], [2, 3])]), 2, ctypes.byref(h)) == N.PGM_OK
    try:
        codes = np.zeros((3, 8), dtype=np.uint8)
        tables = np.zeros(9, dtype=np.int64)
        values = np.zeros(9)
        pc, pt, pv = (a.ctypes.data_as(ctypes.c_void_p) for a in (codes, tables, values))
        count, finish = lib.pgm_fit_count, lib.pgm_fit_finish
        assert count(None, pc, 3, 8, 0, 8, None, pt, None) == EINVAL     # null plan
        assert count(h, None, 3, 8, 0, 8, None, pt, None) == EINVAL      # null codes
        assert count(h, pc, 3, 7, 0, 8, None, pt, None) == EINVAL        # ld < n_rows
        assert count(h, pc, 3, 8, -1, 4, None, pt, None) == EINVAL       # negative row0
        assert count(h, pc, 3, 8, 5, 4, None, pt, None) == EINVAL        # the window leaves ld
        assert count(h, pc, 3, 8, 0, 8, None, None, None) == EINVAL      # null tables
        assert count(h, pc, 2, 8, 0, 8, None, pt, None) == EINVAL        # the plan reads column 2
        assert "codes has 2 columns" in N.last_error()
        assert count(h, pc, 3, 8, 0, 0, None, pt, None) == N.PGM_OK      # nothing to count: no launch
        assert finish(None, pt, None, N.FIT_MLE, pv, None) == EINVAL
        assert finish(h, None, None, N.FIT_MLE, pv, None) == EINVAL
        assert finish(h, pt, None, N.FIT_MLE, None, None) == EINVAL
        assert finish(h, pt, None, 8, pv, None) == EINVAL
        assert lib.pgm_fit_plan_info(None, None, None, None, None, None) == EINVAL
        assert not tables.any() and not values.any()
    finally:
        assert lib.pgm_fit_plan_destroy(h) == N.PGM_OK
    assert lib.pgm_fit_plan_destroy(None) == N.PGM_OK
    assert ctypes.sizeof(N.FitFamily) == 4 + 2 * 4 * N.PGM_MAX_DIMS and ctypes.sizeof(N.FitInfo) == 6 * 4 + 2 * 8


# ---------------------------------------------------------------------------- estimators: errors first
def _model(edges=(("A", "C"), ("B", "C")), latents=()):
    from pgmpy_amd.models import DiscreteBayesianNetwork

    return DiscreteBayesianNetwork(list(edges), latents=set(latents))


FRAME = pd.DataFrame({"A": [0, 0, 1], "B": [0, 1, 0], "C": [1, 1, 0]})


def test_estimator_errors_before_any_compute():
    """The reference's errors (MLE.py:56-84, BayesianEstimator.py:24-48, :245-250, base.py:52-57, :123),
    raised before anything touches a device."""
    from pgmpy_amd.estimators import (BaseEstimator, BayesianEstimator, MaximumLikelihoodEstimator,
                                      ParameterEstimator)

    with pytest.raises(ValueError, match="Found latent variables: {'B'}. Maximum Likelihood doesn't support latent"):
        MaximumLikelihoodEstimator(_model(latents=["B"]), FRAME)
    with pytest.raises(ValueError, match="Bayesian Parameter Estimation works only on models with all observed "
                                         "variables. Found latent variables: {'B'}"):
        BayesianEstimator(_model(latents=["B"]), FRAME)
    with pytest.raises(ValueError, match="Nodes detected in the model that are not present in the dataset: {'C'}"):
        MaximumLikelihoodEstimator(_model(), FRAME[["A", "B"]])
    with pytest.raises(ValueError, match="Data contains unexpected states for variable: A."):
        MaximumLikelihoodEstimator(_model(), FRAME, state_names={"A": [0, 2]})
    with pytest.raises(NotImplementedError, match="Maximum Likelihood Estimate is only implemented for"):
        MaximumLikelihoodEstimator(object(), FRAME)
    with pytest.raises(NotImplementedError, match="Bayesian Parameter Estimation is only implemented for"):
        BayesianEstimator(object(), FRAME)
    est = BayesianEstimator(_model(), FRAME)
    assert est.state_names == {"A": [0, 1], "B": [0, 1], "C": [0, 1]}
    assert BaseEstimator(FRAME, state_names={"A": [1, 0, 7]}).state_names == {"A": [1, 0, 7], "B": [0, 1], "C": [0, 1]}
    with pytest.raises(ValueError, match=r"The shape of pseudo_counts for the node: C must be of shape: \(2, 4\)"):
        est.estimate_cpd("C", prior_type="dirichlet", pseudo_counts=[[1, 1], [2, 2]])
    with pytest.raises(ValueError, match=r"The shape of pseudo_counts for the node: A must be of shape: \(2, 1\)"):
        est.get_parameters(prior_type="dirichlet", pseudo_counts={"A": np.ones((1, 2)), "B": np.ones((2, 1)),
                                                                  "C": np.ones((2, 4))})
    with pytest.raises(ValueError, match="'prior_type' not specified"):
        est.estimate_cpd("C", prior_type="jeffreys")
    with pytest.raises(ValueError, match="'prior_type' not specified"):
        est.get_parameters(prior_type="jeffreys")
    for call in (lambda: est.estimate_cpd("C", weighted=True), lambda: est.get_parameters(weighted=True),
                 lambda: MaximumLikelihoodEstimator(_model(), FRAME).estimate_cpd("A", weighted=True),
                 lambda: MaximumLikelihoodEstimator(_model(), FRAME).get_parameters(weighted=True),
                 lambda: ParameterEstimator(_model(), FRAME).state_counts("C", weighted=True)):
        with pytest.raises(ValueError, match="data must contain a `_weight` column if weighted=True"):
            call()
    with pytest.raises(TypeError, match="Estimator object should be a valid pgmpy estimator."):
        _model().fit(FRAME, estimator=dict)
    from pgmpy_amd.models import JunctionTree

    with pytest.raises(NotImplementedError):
        MaximumLikelihoodEstimator(JunctionTree(), FRAME).get_parameters()


def test_too_many_states_raises_the_encoders_error(monkeypatch):
    """A variable with 255 or more states raises encode_frame's ValueError (uint8 codes)."""
    from pgmpy_amd import engine as E
    from pgmpy_amd.estimators import MaximumLikelihoodEstimator

    monkeypatch.setattr(E, "device", lambda: None)  # the check is the encoders', before any device call
    df = pd.DataFrame({"A": np.arange(255), "B": 0, "C": 1})
    with pytest.raises(ValueError, match="variable A has 255 states; uint8 codes hold at most 254"):
        MaximumLikelihoodEstimator(_model(), df).estimate_cpd("A")


def test_encoders_take_a_states_mapping():
    """encode_states is encode_frame with the states given directly (one encoder, two callers)."""
    from pgmpy_amd.inference.batch import encode_frame, encode_states
    from pgmpy_amd.utils import get_example_model

    m = get_example_model("asia")
    df = pd.DataFrame({"asia": ["yes", "no", None, "no"], "smoke": ["no", "yes", "yes", None]})
    assert np.array_equal(encode_frame(m, df), encode_states(m.states, df))
    got = encode_states({"x": [0.5, 1.5], "y": ["b", "a"]}, pd.DataFrame({"x": [1.5, np.nan, 0.5], "y": ["a", "b", None]}))
    assert got.tolist() == [[1, 255, 0], [1, 0, 255]]


def test_fit_without_gpu_raises_native_unavailable():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pgmpy_amd._native import NativeUnavailable
    from pgmpy_amd.estimators import BayesianEstimator, MaximumLikelihoodEstimator

    with pytest.raises(NativeUnavailable):
        _model().fit(FRAME)
    with pytest.raises(NativeUnavailable):
        _model().fit(FRAME, estimator=BayesianEstimator, prior_type="K2")
    with pytest.raises(NativeUnavailable):
        MaximumLikelihoodEstimator(_model(), FRAME).state_counts("C")
