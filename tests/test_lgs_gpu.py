"""Gaussian structure learning on the device: k_lgs_lane / k_lgs_wave against the long-double restatement under the
bounds of tests/lgs_cases.py at every conditioning-set size where the code takes another path, their bit-identity,
degenerate inputs, and the Python layers (pearsonr, GaussCITester, PC, the Gaussian scores, HillClimbSearch) against
the reference's goldens and the restatement, down to the resident chain simulate -> learn -> fit -> score."""
import numpy as np
import pytest

from tests import lg_cases as LC
from tests import lgs_cases as C

pytestmark = pytest.mark.gpu

U = C.U


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


_MOMENTS = {}


def _moments(X, key=None):
    """(G, shift) device tensors of all the columns of the host matrix X[d, n], at the shift the bounds assume (the
    long-double column means, rounded); cached per key."""
    from pgmpy_amd.models._lg import GramPlan

    if key is not None and key in _MOMENTS:
        return _MOMENTS[key]
    shift = np.nan_to_num(C.shift_of(np.nan_to_num(X)))
    sd = _dev(shift if len(shift) else np.zeros(1))
    out = (GramPlan(range(X.shape[0])).gram(_dev(X), sd), sd)
    if key is not None:
        _MOMENTS[key] = out
    return out


def _run(d, jobs, G, shift, kind=None, intercept=None):
    """(out0, out1, rank) host arrays of one batch."""
    from pgmpy_amd.models._lg import SchurJobs

    batch = SchurJobs(d, jobs)
    if kind is None:
        if intercept is None:
            intercept = len(jobs[0][1]) == 2
        a, b, r = batch.pcorr(G, shift, intercept=intercept)
    else:
        a, b, r = batch.score(G, shift, kind)
    return a.cpu().numpy(), b.cpu().numpy(), r.cpu().numpy()


def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32).tolist() for a in arrays]


def _case_moments(c):
    return _moments(c["X"], ("case", c["d"], c["seed"], c["shifted"]))


# ---------------------------------------------------------------------- every size against the restatement
@pytest.mark.parametrize("case", C.kernel_cases(), ids=lambda c: c["name"])
def test_kernel_case(gpu, case):
    want0, want1, tol0, tol1 = C.case_reference(case)
    G, shift = _case_moments(case)
    got0, got1, rank = _run(case["d"], [(case["K"], case["T"])], G, shift, case["kind"])
    print(case["name"], "errors", abs(got0[0] - want0), abs(got1[0] - want1), "bounds", tol0, tol1)
    assert rank[0] == len(case["K"])
    assert abs(got0[0] - want0) <= tol0 and abs(got1[0] - want1) <= tol1


def test_cap_plus_one_is_refused_without_a_launch(gpu):
    from pgmpy_amd.models._lg import SchurJobs

    with pytest.raises(ValueError, match="at most 64"):
        SchurJobs(67, [(list(range(65)), [65, 66, 67])])


def test_score_kinds_and_rank(gpu):
    """The three kinds of one family differ by their penalties alone; rank counts the ones column, df does not."""
    from math import log

    c = next(c for c in C.kernel_cases() if c["name"] == "score-d37-p6")
    G, shift = _case_moments(c)
    job = [(c["K"], c["T"])]
    ll, rss, rank = _run(c["d"], job, G, shift, "ll")
    bic, rss_b, _ = _run(c["d"], job, G, shift, "bic")
    aic, rss_a, _ = _run(c["d"], job, G, shift, "aic")
    n, df = C.N_ROWS, 6
    assert rank[0] == 7 and _bits(rss) == _bits(rss_b) == _bits(rss_a)
    assert abs((ll[0] - bic[0]) - 0.5 * (df + 2) * log(n)) <= 4 * U * abs(ll[0])
    assert abs((ll[0] - aic[0]) - (df + 2)) <= 4 * U * abs(ll[0])


# ---------------------------------------------------------------------- batches and bit-identity
def _pair_jobs(d, k, count, intercept=False):
    """`count` distinct jobs of one size over d columns."""
    jobs = []
    for i in range(count):
        x, y = i % d, (i // d + 1 + i) % d
        if x == y:
            y = (y + 1) % d
        Z = [z for z in range(d) if z not in (x, y)]
        Z = Z[i % 3:][:k] if len(Z[i % 3:]) >= k else Z[:k]
        jobs.append(C.pcorr_job(Z, x, y, d, intercept))
    return jobs


@pytest.mark.parametrize("k", [2, 8])
def test_batches_of_one_size(gpu, k):
    """1, 63, 64, 65 and 257 jobs (a lane-path workgroup is 64 jobs): a job's bits do not depend on the batch, and the
    first and last jobs agree with the restatement."""
    d = 37
    X = C.case_data(d, 23)
    G, shift = _moments(X, ("case", d, 23, ()))
    jobs = _pair_jobs(d, k, 257)
    full = _run(d, jobs, G, shift)
    assert (full[2] == k).all() and np.isfinite(full[0]).all()
    for count in (1, 63, 64, 65):
        part = _run(d, jobs[:count], G, shift)
        assert _bits(*part) == _bits(*(a[:count] for a in full)), count
    tail = _run(d, jobs[::-1], G, shift)  # every job at another position
    assert _bits(*(a[::-1] for a in tail)) == _bits(*full)
    assert _bits(*_run(d, jobs, G, shift)) == _bits(*full)  # a second run
    for i in (0, 256):
        kappa = C.job_condition(X, C.shift_of(X), jobs[i][0])
        want = C.pcorr_ld(X, *jobs[i])
        tol = C.pcorr_bound(X, C.shift_of(X), *jobs[i], kappa)
        assert abs(full[0][i] - want[0]) <= tol[0] and abs(full[1][i] - want[1]) <= tol[1]


@pytest.mark.parametrize("kind", [None, "bic"])
def test_mixed_batch_bits(gpu, kind):
    """Every size in one batch (one launch per size): each job's outputs carry the bits of the job run alone."""
    d = 37
    G, shift = _moments(C.case_data(d, 23), ("case", d, 23, ()))
    sizes = [0, 1, 2, 7, 8, 9, 30, 7, 8, 0, 34]
    if kind is None:
        jobs = [C.pcorr_job(range(2, 2 + k), 0, 1, d) for k in sizes]
    else:
        jobs = [C.score_job(range(1, 1 + k), 0, d) for k in sizes]
    mixed = _run(d, jobs, G, shift, kind)
    for i, job in enumerate(jobs):
        alone = _run(d, [job], G, shift, kind)
        assert _bits(*alone) == _bits(*(a[i:i + 1] for a in mixed)), sizes[i]
    assert _bits(*mixed) == _bits(*_run(d, jobs, G, shift, kind))


def test_empty_batch(gpu):
    G, shift = _moments(C.case_data(17, 22), ("case", 17, 22, ()))
    for kind in (None, "ll"):
        out = _run(17, [], G, shift, kind, intercept=False)
        assert [len(a) for a in out] == [0, 0, 0]


# ---------------------------------------------------------------------- degenerate inputs
def _check_pcorr(X, job, restated_job, got, i=0):
    """The device's job `job` against the restatement of `restated_job` (the same job without its dropped column)."""
    shift = C.shift_of(X)
    kappa = C.job_condition(X, shift, restated_job[0])
    want = C.pcorr_ld(X, *restated_job)
    tol = C.pcorr_bound(X, shift, *restated_job, kappa)
    assert abs(got[0][i] - want[0]) <= tol[0] and abs(got[1][i] - want[1]) <= tol[1], (got[0][i], want, tol)


@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("intercept", [False, True])
def test_twin_columns_drop_one_pivot(gpu, k, intercept):
    d = 17
    X = C.case_data(d, 22).copy()
    X[5] = X[2]  # columns 2 and 5 are twins
    Z = [1, 2, 3, 5, 6, 7, 8, 9, 10][:k] if k == 9 else [2, 3, 5]
    job = C.pcorr_job(Z, 0, 16, d, intercept)
    without = C.pcorr_job([z for z in Z if z != 5], 0, 16, d, intercept)
    G, shift = _moments(X)
    got = _run(d, [job], G, shift)
    assert got[2][0] == len(job[0]) - 1
    _check_pcorr(X, job, without, got)


@pytest.mark.parametrize("value", [3.0, 0.1])
def test_constant_column_in_k(gpu, value):
    """With an intercept a constant column adds nothing and is dropped (3.0: its shifted column is exactly zero, dropped
    before scaling; 0.1: the shift rounds, its pivot after the ones column is rounding noise, dropped at RCOND).
    Without an intercept it IS the intercept: kept, and the result is that of the job with the ones column in its place."""
    d = 17
    X = C.case_data(d, 22).copy()
    X[4] = value
    G, shift = _moments(X)
    with_icpt = C.pcorr_job([3, 4, 5], 0, 16, d, True)
    got = _run(d, [with_icpt], G, shift)
    assert got[2][0] == 3
    _check_pcorr(X, with_icpt, C.pcorr_job([3, 5], 0, 16, d, True), got)
    no_icpt = C.pcorr_job([3, 4, 5], 0, 16, d, False)
    got = _run(d, [no_icpt], G, shift)
    assert got[2][0] == 3
    _check_pcorr(X, no_icpt, no_icpt, got)


@pytest.mark.parametrize("value", [3.0, 0.1])
def test_constant_x_is_nan_for_that_job_only(gpu, value):
    d = 17
    X = C.case_data(d, 22).copy()
    X[4] = value
    G, shift = _moments(X)
    jobs = [C.pcorr_job([1, 2], 0, 16, d), C.pcorr_job([1, 2], 4, 16, d), C.pcorr_job([1, 2], 16, 4, d, False),
            C.pcorr_job([], 4, 3, d), C.pcorr_job([1, 2], 3, 16, d)]
    got = _run(d, jobs, G, shift)
    assert np.isnan(got[0][1:4]).all() and np.isnan(got[1][1:4]).all()
    for i in (0, 4):
        assert _bits(*_run(d, [jobs[i]], G, shift)) == _bits(*(a[i:i + 1] for a in got))
        _check_pcorr(X, jobs[i], jobs[i], got, i)
    icpt = [C.pcorr_job([1, 2], 4, 16, d, True), C.pcorr_job([1, 2], 0, 16, d, True)]
    got = _run(d, icpt, G, shift)
    assert np.isnan(got[0][0]) and np.isnan(got[1][0]) and np.isfinite(got[0][1])


def test_two_and_three_rows(gpu):
    X = C.case_data(17, 22)
    for n, finite in ((2, False), (3, True)):
        Xn = np.ascontiguousarray(X[:3, :n])
        G, shift = _moments(Xn)
        for job in (C.pcorr_job([], 0, 1, 3), C.pcorr_job([], 0, 1, 3, True)):
            got = _run(3, [job], G, shift)
            if not finite:
                assert np.isnan(got[0][0]) and np.isnan(got[1][0])
            else:
                _check_pcorr(Xn, job, job, got)


def test_nan_cell_touches_its_jobs_only(gpu):
    d = 17
    X = C.case_data(d, 22)
    bad = X.copy()
    bad[6, 100] = np.nan
    G, shift = _moments(X, ("case", d, 22, ()))
    Gb, shift_b = _moments(bad)
    jobs = [C.pcorr_job([1, 2], 0, 16, d), C.pcorr_job([1, 6], 0, 16, d), C.pcorr_job([1, 2], 6, 16, d),
            C.pcorr_job(range(1, 10), 0, 16, d), C.pcorr_job([7, 8, 9, 10, 11, 12, 13, 14, 15], 0, 16, d), C.pcorr_job([], 3, 4, d)]
    clean, dirty = _run(d, jobs, G, shift), _run(d, jobs, Gb, shift_b)
    touched = [1, 2, 3]
    assert np.isnan(dirty[0][touched]).all() and np.isnan(dirty[1][touched]).all()
    rest = [0, 4, 5]
    assert _bits(*(a[rest] for a in dirty)) == _bits(*(a[rest] for a in clean))
    fams = [C.score_job([1, 2], 0, d), C.score_job([6], 0, d), C.score_job([1], 6, d), C.score_job(range(1, 12), 0, d)]
    clean, dirty = _run(d, fams, G, shift, "bic"), _run(d, fams, Gb, shift_b, "bic")
    assert np.isnan(dirty[0][1:]).all() and np.isnan(dirty[1][1:]).all()
    assert _bits(*(a[:1] for a in dirty)) == _bits(*(a[:1] for a in clean))


def test_exact_fit_scores_plus_infinity(gpu):
    """rss <= 0: a target that is an exact dyadic combination of its parents."""
    d = 4
    rng = np.random.default_rng(5)
    X = np.round(rng.standard_normal((d, 64)) * 8) / 8
    X[3] = 2 * X[0] - 0.5 * X[1]
    G, shift = _moments(X)
    score, rss, _ = _run(d, [C.score_job([0, 1], 3, d), C.score_job([0], 3, d)], G, shift, "bic")
    assert (score[0] == np.inf or rss[0] > 0) and np.isfinite(score[1])
    assert rss[0] <= 64 * 64 * U * float((X[3] ** 2).sum())


# ---------------------------------------------------------------------- the Python layers
GOLD, _ = C.golden()
FRAMES = sorted(GOLD["frames"])


def _host_slack(X, shift, job):
    """The reference's own fp64 error (test_lgs_cpu.test_restatement_matches_the_reference_pearsonr)."""
    sd = X.std(axis=1)
    kappa = C.job_condition(X, shift, job[0])
    return 64 * U * kappa * (1 + max(abs(shift[j]) / sd[j] for j in job[0] + job[1][:2])), kappa


@pytest.mark.parametrize("name", FRAMES)
def test_pearsonr_and_tester_match_the_reference(gpu, name):
    import torch

    from pgmpy_amd.estimators import GaussCITester
    from pgmpy_amd.estimators.CITests import pearsonr

    df = C.frame(name)
    X, cols = np.ascontiguousarray(df.to_numpy(dtype=np.float64).T), list(df.columns)
    d, n = X.shape
    recs = GOLD["pearsonr"][name]
    tester = GaussCITester(df)
    coef, p = tester.tests([(r["X"], r["Y"], r["Z"]) for r in recs])
    resident = GaussCITester.from_values(torch.from_numpy(X).cuda(), cols)
    coef_r, p_r = resident.tests([(r["X"], r["Y"], r["Z"]) for r in recs])
    assert _bits(coef, p) == _bits(coef_r, p_r)  # the frame route uploads the same matrix
    shift = tester.gram()[1].cpu().numpy()
    for i, r in enumerate(recs):
        job = C.pcorr_job([cols.index(z) for z in r["Z"]], cols.index(r["X"]), cols.index(r["Y"]), d)
        host, kappa = _host_slack(X, shift, job)
        tol = C.pcorr_bound(X, shift, *job, kappa)
        assert abs(coef[i] - r["coef"]) <= tol[0] + host
        assert abs(p[i] - r["p"]) <= tol[1] + C.dp_dcoef(max(abs(r["coef"]) - host - tol[0], 0), n) * host + 1e-13 * r["p"]
    one = pearsonr(recs[2]["X"], recs[2]["Y"], recs[2]["Z"], df, boolean=False)
    assert _bits(np.array(one)) == _bits(np.array([coef[2], p[2]]))
    assert pearsonr(recs[2]["X"], recs[2]["Y"], recs[2]["Z"], df, significance_level=0.01) is bool(p[2] >= 0.01)
    ci, pi = tester.tests([(r["X"], r["Y"], r["Z"]) for r in recs[:2]], intercept=True)  # Z empty: the same test
    assert np.allclose(ci, coef[:2], rtol=0, atol=1e-12) and np.allclose(pi, p[:2], rtol=1e-9, atol=0)


def _pc_record(skeleton, pdag):
    return {"skeleton": sorted(sorted(e) for e in skeleton.edges()), "directed": sorted(list(e) for e in pdag.directed_edges),
            "undirected": sorted(sorted(e) for e in pdag.undirected_edges)}


@pytest.mark.parametrize("name", FRAMES)
@pytest.mark.parametrize("variant", ["orig", "stable"])
def test_pc_matches_the_reference(gpu, name, variant, monkeypatch):
    from pgmpy_amd.estimators import PC, GaussCITester
    from pgmpy_amd.estimators.CITests import pearsonr
    from pgmpy_amd.models import _lg

    df = C.frame(name)
    want = {k: GOLD["pc"][name][variant][k] for k in ("skeleton", "directed", "undirected")}
    launches = []
    real = _lg.SchurJobs.pcorr
    monkeypatch.setattr(_lg.SchurJobs, "pcorr",
                        lambda self, *a, **k: (launches.append((int(self.info.n_buckets), self.buckets()[0][0][0])), real(self, *a, **k))[1])
    for route in ("function", "tester"):
        del launches[:]
        pc = PC(df) if route == "function" else PC(df, tester=GaussCITester(df))
        ci_test = pearsonr if route == "function" else None
        skeleton, _ = pc.estimate(variant=variant, ci_test=ci_test, return_type="skeleton", significance_level=0.01)
        n_skeleton = len(launches)
        pdag = pc.estimate(variant=variant, ci_test=ci_test, return_type="pdag", significance_level=0.01)
        assert _pc_record(skeleton, pdag) == want, route
        assert all(b == 1 for b, _ in launches)  # a call is one launch: one conditioning-set size
        if variant == "stable":  # one call, so one launch, per level
            levels = [k for _, k in launches[:n_skeleton]]
            assert levels == sorted(set(levels)) and len(levels) >= 2


class RestatedScorer:
    """hill_climb's scorer on the restatement."""

    def __init__(self, df):
        self.X = np.ascontiguousarray(df.to_numpy(dtype=np.float64).T)
        self.cols = list(df.columns)

    def job(self, v, parents):
        return C.score_job([self.cols.index(u) for u in parents], self.cols.index(v), len(self.cols))

    def local_scores(self, families):
        return [C.score_ld(self.X, *self.job(v, ps), "bic")[0] for v, ps in families]

    def structure_prior_ratio(self, operation):
        return 0

    def structure_prior(self, model):
        return 0


@pytest.mark.parametrize("name", FRAMES)
def test_hill_climb_with_bicgauss_matches_the_restatement(gpu, name):
    from pgmpy_amd.estimators import BICGauss, HillClimbSearch
    from pgmpy_amd.estimators.HillClimbSearch import hill_climb

    df = C.frame(name)
    scorer = BICGauss(df)
    model = HillClimbSearch(df).estimate(scoring_method=scorer)
    host = RestatedScorer(df)
    want, _, _ = hill_climb(list(df.columns), host)
    assert sorted(model.edges()) == sorted(want.edges())
    fams = [(v, sorted(model.predecessors(v))) for v in df.columns]
    shift = scorer.gram()[1].cpu().numpy()
    total_tol = sum(C.score_bound(host.X, shift, *host.job(v, ps), C.job_condition(host.X, shift, host.job(v, ps)[0]))[0]
                    for v, ps in fams)
    total = sum(host.local_scores(fams))
    assert abs(scorer.score(model) - total) <= total_tol + 8 * U * abs(total)
    assert scorer.local_score(*fams[-1]) == scorer.local_scores(fams)[-1]


# zero intercepts: the reference's pearsonr regresses WITHOUT one, so it is a partial correlation for centred data only
CHAIN = {"cpds": [("a", [0.0], 1.0, []), ("b", [0.0], 1.0, []), ("c", [0.0, 1.0, -1.0], 1.0, ["a", "b"]),
                  ("d", [0.0, 0.75], 1.0, ["c"]), ("e", [0.0, 1.0], 1.0, ["d"])],
         "edges": [("a", "c"), ("b", "c"), ("c", "d"), ("d", "e")], "seed": 2026, "rows": 4096}


def markov_class(edges):
    """(skeleton, v-structures): two DAGs are Markov equivalent when both agree."""
    from itertools import combinations

    import networkx as nx

    g = nx.DiGraph(list(edges))
    skeleton = {frozenset(e) for e in g.edges()}
    return skeleton, {(frozenset((a, b)), c) for c in g.nodes() for a, b in combinations(sorted(g.predecessors(c)), 2)
                      if frozenset((a, b)) not in skeleton}


def test_resident_chain(gpu):
    """simulate_values -> PC / hill_climb -> fit_values -> log_likelihood_values on one resident matrix of 4,096 rows
    (a -> c <- b, c -> d -> e; rehearsed on the CPU with lg_cases.sample_ld's restatement of the sampler: the restated
    PC and hill climb recover the class at this seed and its two successors)."""
    from pgmpy_amd.estimators import PC, BICGauss, GaussCITester, LogLikelihoodGauss
    from pgmpy_amd.estimators.HillClimbSearch import hill_climb
    from pgmpy_amd.factors.continuous import LinearGaussianCPD
    from pgmpy_amd.models import LinearGaussianBayesianNetwork

    truth = LinearGaussianBayesianNetwork(CHAIN["edges"])
    for v, beta, std, ev in CHAIN["cpds"]:
        truth.add_cpds(LinearGaussianCPD(v, beta, std, ev))
    nodes = list(truth.nodes())
    X = truth.simulate_values(CHAIN["rows"], seed=CHAIN["seed"])
    pdag = PC(None, tester=GaussCITester.from_values(X, nodes)).estimate(variant="stable", significance_level=0.01)
    assert markov_class(pdag.to_dag().edges()) == markov_class(CHAIN["edges"])
    dag, _, _ = hill_climb(nodes, BICGauss.from_values(X, nodes))
    assert markov_class(dag.edges()) == markov_class(CHAIN["edges"])
    learned = LinearGaussianBayesianNetwork(list(dag.edges())).fit_values(X, nodes, std_estimator="mle")
    _, total = learned.log_likelihood_values(X, nodes)
    # The fitted model's log-likelihood IS the sum of its families' concentrated log-likelihoods.  A family's term
    # n log sigma moves by n dsigma / sigma, and dsigma / sigma is at most the fit's eps kappa = 2 p (n + 2) u kappa
    # (lg_cases.coef_rtol) with p <= 2 parents and kappa <= 16 here: 64 (n + 2) u per family; the row sums of both
    # sides add n roundings of terms of the total's size (lg_cases, logpdf): 16 n u |ll| covers them.
    want = LogLikelihoodGauss.from_values(X, nodes).score(learned)
    n = CHAIN["rows"]
    assert np.isfinite(total) and abs(total - want) <= 64 * (n + 2) * U * n * len(nodes) + 16 * n * U * abs(want)
