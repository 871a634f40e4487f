"""Gaussian structure learning without a device: the long-double restatement (tests/lgs_cases.py) against the
reference's recorded pearsonr and PC results, the closed-form log-likelihood against the summed log-density, the
job batch handle's validation and buckets, the host build of the p-value's incomplete beta function, the rounds,
the argument errors that come before the device, and the negative controls of every kernel case."""
import ctypes

import numpy as np
import pytest

from tests import lgs_cases as C

U = C.U


# ---------------------------------------------------------------------- the restatement against the reference
def _X(df):
    return np.ascontiguousarray(df.to_numpy(dtype=np.float64).T)


@pytest.mark.parametrize("name", ["chain4", "collider5", "fork6"])
def test_restatement_matches_the_reference_pearsonr(name):
    """The reference runs numpy's fp64 lstsq on the frame and scipy's fp64 pearsonr on the residuals: with kappa the
    condition number of the unit-diagonal raw conditioning block its coefficient carries about 64 u kappa (1 + max
    |mean| / sd) (as lg_cases' `host` term), and its p-value that error through dp / dcoef plus scipy's own 1e-13."""
    g, _ = C.golden()
    df = C.frame(name)
    X, cols = _X(df), list(df.columns)
    d = len(cols)
    shift = C.shift_of(X)
    sd = X.std(axis=1)
    for rec in g["pearsonr"][name]:
        job = C.pcorr_job([cols.index(z) for z in rec["Z"]], cols.index(rec["X"]), cols.index(rec["Y"]), d)
        coef, p = C.pcorr_ld(X, *job)
        kappa = C.job_condition(X, shift, job[0])
        host = 64 * U * kappa * (1 + max(abs(shift[j]) / sd[j] for j in job[0] + job[1][:2]))
        print(name, rec["X"], rec["Y"], rec["Z"], abs(coef - rec["coef"]), host, abs(p - rec["p"]))
        assert abs(coef - rec["coef"]) <= host
        assert abs(p - rec["p"]) <= C.dp_dcoef(max(abs(coef) - host, 0), X.shape[1]) * host + 1e-13 * p + 1e-300


class RestatedTester:
    """pc_skeleton's tester on the restatement."""

    def __init__(self, df):
        self.X, self.cols = _X(df), list(df.columns)
        self.calls = []

    def independent(self, triples, significance_level):
        self.calls.append(len(triples))
        d = len(self.cols)
        return [C.pcorr_ld(self.X, *C.pcorr_job([self.cols.index(z) for z in Z], self.cols.index(x), self.cols.index(y), d))[1]
                >= significance_level for x, y, Z in triples]


def check_pc(got_skeleton, got_pdag, rec):
    assert sorted(sorted(e) for e in got_skeleton.edges()) == rec["skeleton"]
    assert sorted(list(e) for e in got_pdag.directed_edges) == rec["directed"]
    assert sorted(sorted(e) for e in got_pdag.undirected_edges) == rec["undirected"]


@pytest.mark.parametrize("name", ["chain4", "collider5", "fork6"])
@pytest.mark.parametrize("variant", ["orig", "stable"])
def test_pc_loop_under_the_restatement_matches_the_reference(name, variant):
    from pgmpy_amd.estimators.PC import PC, pc_skeleton

    g, _ = C.golden()
    df = C.frame(name)
    skel, seps = pc_skeleton(list(df.columns), RestatedTester(df), variant=variant, significance_level=g["significance_level"])
    pdag = PC.orient_colliders(skel, seps).apply_meeks_rules(apply_r4=False).apply_meeks_rules(apply_r4=True)
    check_pc(skel, pdag, g["pc"][name][variant])


def test_golden_margin():
    g, _ = C.golden()
    assert g["smallest_margin"] >= g["margin_required"] == 10.0
    assert all(f["margin"] >= 10.0 for f in g["frames"].values())


def test_closed_form_llf_is_the_summed_log_density():
    """The sum over the rows rounds n terms of size |log-density| in long double: 4 n u_ld of the sum of their
    magnitudes is far below the fp64 comparison's 4 u (|llf| + n)."""
    for c in C.kernel_cases():
        if c["kind"] == "ll":
            score, rss, closed = C.score_ld(c["X"], c["K"], c["T"], "ll")
            assert abs(score - closed) <= 4 * U * (abs(closed) + c["X"].shape[1]), c["name"]


# ---------------------------------------------------------------------- the C side without a device
def test_symbols_and_abi():
    from pgmpy_amd import _native as N

    lib = N.load_library()
    for name in ("pgm_lgs_jobs_create", "pgm_lgs_jobs_destroy", "pgm_lgs_jobs_info", "pgm_lgs_pcorr", "pgm_lgs_score",
                 "pgm_lgs_ibeta_half"):
        assert name in N.EXPORTED and getattr(lib, name).argtypes is not None
    assert lib.pgm_version() == 25
    assert (N.LGS_MAX_COND, N.LGS_LANE_MAX, N.LGS_MAX_TARGETS) == (64, 7, 3)
    assert ctypes.sizeof(N.LgsInfo) == 40


def test_plan_refusals():
    from pgmpy_amd.models import _lg

    d = 70
    ok = _lg.SchurJobs(d, [(list(range(64)), [64, 65, d])])
    assert ok.info.max_cond == 64 and ok.info.n_wave_jobs == 1 and ok.info.wave_lds_bytes == 37520
    for jobs, words in (([([0, 1, 0], [2])], "twice"),
                        ([([0, 1], [2, 2, d])], "twice"),
                        ([([0, 1], [1, 2])], "also a conditioning column"),
                        ([(list(range(65)), [65, 66, d])], "at most 64"),
                        ([([0], [])], "0 targets"),
                        ([([0], [1, 2, 3, 4])], "4 targets"),
                        ([([d + 1], [0])], f"column {d + 1}"),
                        ([([-1], [0])], "column -1")):
        with pytest.raises(ValueError, match=words):
            _lg.SchurJobs(d, jobs)


def test_call_shape_checks_need_no_device():
    """The shape of a batch's jobs against the call is checked before any HIP call: with no device the library is
    driven through ctypes with null device pointers and must answer PGM_EINVAL, not touch them."""
    from pgmpy_amd import _native as N
    from pgmpy_amd.models import _lg

    L = N.load_library()
    one = ctypes.c_void_p(8)  # never dereferenced: the checks refuse first
    d = 5
    for jobs, intercept, words in (([([0], [1, 2])], 0, "needs 3"), ([([0], [1, 2, d])], 1, "needs 2"),
                                   ([([0], [1, 2, 3])], 0, "ones column"), ([([0], [1, 2])], 1, "ones column")):
        h = _lg.SchurJobs(d, jobs)
        assert L.pgm_lgs_pcorr(h._h, one, one, d, intercept, one, one, one, None) == N.PGM_EINVAL
        assert words in N.last_error()
    h = _lg.SchurJobs(d, [([0], [1])])
    assert L.pgm_lgs_score(h._h, one, one, d, N.LGS_BIC, one, one, one, None) == N.PGM_EINVAL and "ones column" in N.last_error()
    h = _lg.SchurJobs(d, [([d, 0], [1])])
    assert L.pgm_lgs_score(h._h, one, one, d, 7, one, one, one, None) == N.PGM_EINVAL and "kind" in N.last_error()
    assert L.pgm_lgs_score(h._h, one, one, d + 1, N.LGS_LL, one, one, one, None) == N.PGM_EINVAL
    empty = _lg.SchurJobs(d, [])
    assert L.pgm_lgs_score(empty._h, None, None, d, N.LGS_LL, None, None, None, None) == N.PGM_OK
    assert L.pgm_lgs_pcorr(empty._h, None, None, d, 0, None, None, None, None) == N.PGM_OK


def test_buckets():
    from pgmpy_amd.models import _lg

    d = 20
    jobs = [(list(range(k)), [17, 18, d]) for k in (3, 0, 8, 3, 7, 0, 9, 8)] + [([d, 1], [0])]
    h = _lg.SchurJobs(d, jobs)
    buckets, order = h.buckets()
    assert buckets == [(0, 3, 0, 2), (2, 1, 2, 1), (3, 3, 3, 2), (7, 3, 5, 1), (8, 3, 6, 2), (9, 3, 8, 1)]
    assert order == [1, 5, 8, 0, 3, 4, 2, 7, 6]  # each bucket in the batch's own order
    assert (h.info.n_lane_jobs, h.info.n_wave_jobs) == (6, 3)


A_GRID = (0.5, 1.0, 50.0, 5e5)


@pytest.mark.parametrize("a", A_GRID)
def test_host_incomplete_beta_against_mpmath(a):
    """y = r^2 near 0 (p near 1), in between, and near 1 (p tiny); a = 5e5 needs ~ sqrt(a) steps of the fraction
    around y ~ 1 / a."""
    from pgmpy_amd import _native as N

    L = N.load_library()
    ys = [1e-300, 1e-18, 1e-9, 0.1 / a, 0.5 / a, 1.0 / a, 3.0 / a, 30.0 / a, 0.25, 0.5, 0.9, 1 - 1e-9, 1 - 2.0 ** -52]
    worst = 0.0
    for y in ys:
        if not 0.0 < y < 1.0:
            continue
        out = ctypes.c_double()
        assert L.pgm_lgs_ibeta_half(a, y, ctypes.byref(out)) == N.PGM_OK
        ref = C.ibeta_half(a, y)
        if ref < 1e-300:
            assert out.value < 1e-299
            continue
        tol = C.ibeta_rel(a, y) * ref + (2 * U if ref > 0.1 else 0.0)
        worst = max(worst, abs(out.value - ref) / tol)
        assert abs(out.value - ref) <= tol, (a, y, out.value, ref, abs(out.value - ref) / ref, C.ibeta_rel(a, y))
    print("a", a, "worst error / bound", worst)
    for y, want in ((0.0, 1.0), (1.0, 0.0)):
        out = ctypes.c_double()
        L.pgm_lgs_ibeta_half(a, y, ctypes.byref(out))
        assert out.value == want
    for bad in ((a, -0.1), (a, 1.5), (a, float("nan")), (0.0, 0.5), (-1.0, 0.5)):
        out = ctypes.c_double()
        L.pgm_lgs_ibeta_half(bad[0], bad[1], ctypes.byref(out))
        assert np.isnan(out.value)


# ---------------------------------------------------------------------- Python: rounds, errors before the device
def _df(n=20, cols="abcde"):
    import pandas as pd

    rng = np.random.default_rng(0)
    return pd.DataFrame(rng.standard_normal((n, len(cols))), columns=list(cols))


def test_rounds_split_a_batch_and_keep_its_order(monkeypatch):
    import torch

    from pgmpy_amd.estimators import GaussCITester, _gauss
    from pgmpy_amd.inference import batch
    from pgmpy_amd.models import _lg

    made = []

    class FakeJobs:
        def __init__(self, d, jobs):
            self.jobs = jobs
            made.append(jobs)

        def pcorr(self, G, shift, intercept=False):
            v = torch.tensor([float(sum(K) * 100 + T[0] * 10 + T[1]) for K, T in self.jobs], dtype=torch.float64)
            return v, -v, None

    monkeypatch.setattr(_lg, "SchurJobs", FakeJobs)
    monkeypatch.setattr(batch, "download", lambda t: t.numpy())
    monkeypatch.setattr(_gauss.GaussData, "gram", lambda self: (None, None))
    monkeypatch.setattr(_gauss, "ROUND_COLUMNS", 9)  # two tests with one conditioning column, or one with more
    t = GaussCITester(_df())
    triples = [("a", "b", []), ("a", "c", ["b"]), ("b", "c", ["a"]), ("d", "e", ["a", "b", "c"]), ("a", "e", [])]
    coef, p = t.tests(triples)
    assert [len(j) for j in made] == [2, 1, 2]
    assert list(coef) == [1.0, 102.0, 12.0, 334.0, 4.0] and list(p) == [-c for c in coef]


def test_argument_errors_come_before_the_device():
    """No device on this side: reaching it would raise NativeUnavailable instead."""
    from pgmpy_amd.estimators import AICGauss, BICGauss, GaussCITester, LogLikelihoodGauss, StructureScore
    from pgmpy_amd.estimators.CITests import pearsonr

    df = _df()
    t = GaussCITester(df)
    with pytest.raises(ValueError, match="can't be in Z"):
        t.tests([("a", "b", ["a"])])
    with pytest.raises(ValueError, match="iterable"):
        t.tests([("a", "b", 3)])
    with pytest.raises(KeyError):
        t.tests([("a", "zz", [])])
    with pytest.raises(ValueError, match="twice"):
        t.tests([("a", "a", [])])
    with pytest.raises(ValueError, match="iterable"):
        pearsonr("a", "b", 3, df)
    with pytest.raises(ValueError, match="DataFrame"):
        pearsonr("a", "b", [], df.to_numpy())
    assert t.tests([])[0].shape == (0,) and t.independent([]).shape == (0,)
    wide = _df(4, [f"v{i}" for i in range(70)])
    with pytest.raises(ValueError, match="PGM_LGS_MAX_COND = 64"):
        GaussCITester(wide).tests([("v0", "v1", [f"v{i}" for i in range(2, 67)])])
    with pytest.raises(ValueError, match="at most 63"):
        GaussCITester(wide).tests([("v0", "v1", [f"v{i}" for i in range(2, 66)])], intercept=True)
    for cls in (LogLikelihoodGauss, BICGauss, AICGauss):
        s = cls(wide)
        assert isinstance(s, StructureScore) and not hasattr(s, "state_names")
        with pytest.raises(ValueError, match="PGM_LGS_MAX_COND = 64"):
            s.local_scores([("v0", [f"v{i}" for i in range(1, 65)])])
        with pytest.raises(KeyError):
            s.local_score("v0", ["nope"])
        with pytest.raises(ValueError, match="twice"):
            s.local_score("v0", ["v1", "v1"])
        assert s.local_scores([]) == [] and s.structure_prior(None) == 0 and s.structure_prior_ratio("+") == 0


def test_instances_pass_get_scoring_method_and_names_stay_closed():
    from pgmpy_amd.estimators import BICGauss, get_scoring_method
    from pgmpy_amd.estimators.CITests import get_callable_ci_test, pearsonr

    df = _df()
    s = BICGauss(df)
    assert get_scoring_method(s, df) == (s, s)
    assert get_callable_ci_test(pearsonr) is pearsonr
    with pytest.raises(ValueError, match="not built"):
        get_callable_ci_test("pearsonr")
    with pytest.raises(ValueError, match="not built"):
        get_scoring_method("bic-g", df)


def test_pc_hands_a_level_to_the_gauss_tester_in_one_call():
    """PC with ci_test=pearsonr or tester=GaussCITester builds the batching tester, not one call per test."""
    from pgmpy_amd.estimators import PC, GaussCITester
    from pgmpy_amd.estimators.CITests import chi_square, pearsonr
    from pgmpy_amd.estimators.PC import _GaussTester

    df = _df()
    pc = PC(df)
    t = pc._tester(pearsonr, {})
    assert isinstance(t, _GaussTester) and isinstance(t.tester, GaussCITester) and not t.intercept
    assert pc._tester(pearsonr, {"intercept": True}).tester is t.tester  # one tester, one Gram, per PC
    mine = GaussCITester(df)
    pc2 = PC(df, tester=mine)
    assert pc2._tester(None, {}).tester is mine and pc2.variables == list(df.columns)
    assert PC(None, tester=mine).variables == list(df.columns)
    with pytest.raises(ValueError, match="pearsonr"):
        pc2._tester(chi_square, {})


# ---------------------------------------------------------------------- the negative controls
@pytest.mark.parametrize("case", [c for c in C.kernel_cases() if [z for z in c["K"] if z != c["d"]]], ids=lambda c: c["name"])
def test_negative_control(case):
    """The restatement with one conditioning column left out lies outside the bound of the true job (a case without
    a conditioning column has none to leave out)."""
    ratio = C.negative_control(case["X"], case["shift"], case["K"], case["T"], case["kappa"], case["kind"])
    assert ratio > 1.0, ratio
