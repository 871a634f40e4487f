"""CI tests and PC on the device: the CI kernels against the long-double restatement on the case table and
their bit-identity alone and in a batch, CITester against the reference's goldens, the rounds, PC against
the golden skeletons and PDAGs, and the chain simulate -> PC -> fit -> predict.

The references are tests/ci_cases.py's restatement (which tests/test_ci_cpu.py pins to the goldens) and the
goldens themselves (tests/golden/ci_cases.json + .npz).  Bounds: ci_cases.bound / p_bound."""
import functools

import networkx as nx
import numpy as np
import pytest

from tests import ci_cases as C
from tests import fit_cases as F

pytestmark = pytest.mark.gpu

KCASES = {c["name"]: c for c in C.kernel_cases()}
MIXED, ORIGIN = C.mixed_batch(list(KCASES.values()))
GOLDEN = C.load_golden()
ALPHA = GOLDEN["s"]["alpha"]
# (lambda, Yates): the six named lambdas with the correction, Pearson and G without
COMBOS = [(lam, True) for lam in C.LAMBDAS.values()] + [(1.0, False), (0.0, False)]


def _dev(a):
    from pgmpy_amd import engine as E

    return E.to_device_raw(np.ascontiguousarray(a))


def _host(t):
    from pgmpy_amd.inference.batch import download

    return download(t)


def _plan(families):
    from pgmpy_amd import _native as N
    from pgmpy_amd.estimators._fit import FitPlan

    assert N.CI_CHUNK == C.CHUNK  # the cases' geometry
    return FitPlan(families)


@functools.lru_cache(maxsize=None)
def _tables(name):
    c = MIXED if name == "mixed" else KCASES[name]
    return C.tables_of(c["codes"], c["families"])


@functools.lru_cache(maxsize=None)
def _reference(name, lam, yates):
    """[(stat, dof, p, magnitude, cells)] per family of a kernel case, computed once."""
    c = MIXED if name == "mixed" else KCASES[name]
    return [C.ci_ref(t, lam, yates, len(cols) > 2) for t, (cols, _) in zip(_tables(name), c["families"])]


def _citest(plan, counts, lam, yates):
    stat, dof, p = plan.citest(counts, lam, yates=yates)
    return _host(stat), _host(dof), _host(p)


def _assert_equal_the_restatement(name, got, lam, yates):
    stat, dof, p = got
    for f, (s, d, pv, mag, cells) in enumerate(_reference(name, lam, yates)):
        key = (name, f, lam, yates)
        assert int(dof[f]) == d, key
        b = C.bound(cells, mag)
        assert C.same(stat[f], s, b), (key, float(stat[f]), float(s), b)
        assert C.same(p[f], pv, C.p_bound(s, d, pv, b)), (key, float(p[f]), float(pv))


# ---------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("name", list(KCASES))
def test_kernel_equals_the_restatement(gpu, name):
    """Every family's (stat, dof, p) is the long-double restatement's within ci_cases.bound; dof is exact; a
    second run gives the same bits."""
    c = KCASES[name]
    plan = _plan(c["families"])
    counts = plan.count(_dev(c["codes"]))
    assert np.array_equal(_host(counts), F.count_ref(c["codes"], c["families"]))
    for lam, yates in COMBOS:
        got = _citest(plan, counts, lam, yates)
        _assert_equal_the_restatement(name, got, lam, yates)
        again = _citest(plan, counts, lam, yates)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_mixed_batch_equals_the_restatement_and_each_test_alone(gpu):
    """One plan that mixes all the cases: the restatement's values, and for every test the same bits as the
    test alone in a plan of its own (the chunks and the order of additions are the test's own)."""
    codes = _dev(MIXED["codes"])
    plan = _plan(MIXED["families"])
    counts = plan.count(codes)
    for lam, yates in ((1.0, True), (0.0, True), (-0.5, True), (1.0, False)):
        _assert_equal_the_restatement("mixed", _citest(plan, counts, lam, yates), lam, yates)
    for lam in (1.0, 2.0 / 3.0):
        stat, dof, p = _citest(plan, counts, lam, True)
        for f, fam in enumerate(MIXED["families"]):
            alone = _plan([fam])
            s1, d1, p1 = _citest(alone, alone.count(codes), lam, True)
            assert (s1.tobytes(), d1.tobytes(), p1.tobytes()) == (stat[f:f + 1].tobytes(), dof[f:f + 1].tobytes(),
                                                                  p[f:f + 1].tobytes()), (f, ORIGIN[f], lam)


def test_a_weighted_table_is_refused(gpu):
    import torch

    plan = _plan([([0, 1], [3, 2])])
    with pytest.raises(ValueError, match="weighted tables have no CI test"):
        plan.citest(torch.zeros(6, dtype=torch.float64, device="cuda"), 1.0)
    with pytest.raises(ValueError, match="int64"):
        plan.citest(torch.zeros(5, dtype=torch.int64, device="cuda"), 1.0)


# ---------------------------------------------------------------------------- CITester == the reference
def _check_goldens(df, tests):
    from pgmpy_amd.estimators import CITester

    tester = CITester(df)
    host = C.HostTester(df)
    triples = [(t["X"], t["Y"], t["Z"]) for t in tests]
    for name, lam in C.LAMBDAS.items():
        stat, p, dof = tester.tests(triples, name)
        assert stat.dtype == np.float64 and p.dtype == np.float64 and dof.dtype == np.int64
        for i, (t, (s, d, pv, mag, cells)) in enumerate(zip(tests, host.tests(triples, lam))):
            chi, p_ref, dof_ref = t["results"][name]
            key = (t["X"], t["Y"], t["Z"], name)
            assert int(dof[i]) == dof_ref, key
            b = C.bound(cells, mag)
            assert C.same(stat[i], chi, b), (key, stat[i], chi, b)
            assert C.same(p[i], p_ref, C.p_bound(s, d, pv, b) + (1e-15 if t["Z"] else 0.0)), (key, p[i], p_ref)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(tester.independent(triples, ALPHA, name), p >= ALPHA)


def test_citester_equals_the_goldens_of_s(gpu):
    _check_goldens(C.frame_of(GOLDEN["s"]), GOLDEN["s"]["tests"])


@pytest.mark.parametrize("key", sorted(GOLDEN["edge"]))
def test_citester_equals_the_goldens_of_the_edge_frames(gpu, key):
    _check_goldens(C.frame_of(GOLDEN["edge"][key]), GOLDEN["edge"][key]["tests"])


def test_module_functions_are_the_one_test_case(gpu):
    from pgmpy_amd.estimators import CITests as T

    df = C.frame_of(GOLDEN["s"])
    t = next(t for t in GOLDEN["s"]["tests"] if len(t["Z"]) == 2)
    one = T.CITester(df).tests([(t["X"], t["Y"], t["Z"])], 1.0)
    chi, p, dof = T.chi_square(t["X"], t["Y"], t["Z"], df, boolean=False)
    assert (chi, p, dof) == (float(one[0][0]), float(one[1][0]), int(one[2][0])) and isinstance(dof, int)
    assert T.chi_square(t["X"], t["Y"], t["Z"], df, boolean=True, significance_level=ALPHA) == (p >= ALPHA)
    for fn, name in ((T.g_sq, "log-likelihood"), (T.log_likelihood, "log-likelihood"),
                     (T.modified_log_likelihood, "mod-log-likelihood"), (T.power_divergence, "cressie-read")):
        got = fn(t["X"], t["Y"], t["Z"], df, boolean=False)
        want = T.CITester(df).tests([(t["X"], t["Y"], t["Z"])], name)
        assert got == (float(want[0][0]), float(want[1][0]), int(want[2][0]))
    assert np.array_equal(T.power_divergence(t["X"], t["Y"], t["Z"], df, boolean=False, lambda_=-2.0),
                          T.power_divergence(t["X"], t["Y"], t["Z"], df, boolean=False, lambda_="neyman"), equal_nan=True)


def test_split_rounds_give_the_same_bits(gpu, monkeypatch):
    from pgmpy_amd.estimators import CITester
    from pgmpy_amd.estimators import _rounds as module

    df = C.frame_of(GOLDEN["s"])
    triples = [(t["X"], t["Y"], t["Z"]) for t in GOLDEN["s"]["tests"]]
    whole = CITester(df).tests(triples, 0.0)
    monkeypatch.setattr(module, "SCORE_BIN_BUDGET", 40)  # a few tests per round; a test of 54 bins runs alone
    assert len(module.rounds([6, 18, 54, 6, 6, 54], 40)) == 4
    split = CITester(df).tests(triples, 0.0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, split))


# ---------------------------------------------------------------------------- PC
def _pdag_record(pdag):
    return (sorted(pdag.nodes()), sorted(list(e) for e in pdag.directed_edges),
            sorted(sorted(e) for e in pdag.undirected_edges))


@pytest.mark.parametrize("name", ["chi_square", "g_sq"])
def test_pc_estimate_returns_the_golden_pdag_of_s(gpu, name):
    from pgmpy_amd.estimators import PC

    df = C.frame_of(GOLDEN["s"])
    want = GOLDEN["s"]["pc"][name]
    for variant in ("parallel", "stable", "orig"):
        pdag = PC(df).estimate(variant=variant, ci_test=name, significance_level=ALPHA, show_progress=False)
        assert _pdag_record(pdag) == (want["pdag"]["nodes"], want["pdag"]["directed"], want["pdag"]["undirected"]), variant
    skeleton, sepsets = PC(df).build_skeleton(ci_test=name, significance_level=ALPHA)
    assert sorted(sorted(e) for e in skeleton.edges()) == want["edges"]
    assert sorted([sorted(k), sorted(v)] for k, v in sepsets.items()) == want["separating_sets"]


def test_pc_skeleton_of_the_alarm_rows(gpu):
    """The reference's chi_square skeletons over the 1,000 alarm rows; the separating sets are compared by
    size (which of several equally small sets is met first depends on the walking order).  The reference's
    "stable" removes an edge as soon as it is separated, exactly as its "orig" does, so its skeleton (33
    edges) is the one "orig" gives here; its "parallel" tests a level against frozen neighbour sets and
    its skeleton (30 edges) is the one "stable" and "parallel" give here."""
    from pgmpy_amd.estimators import PC

    df, states = C.alarm_frame()
    est = PC(df, state_names=states)
    for variant, want in (("orig", GOLDEN["alarm"]), ("stable", GOLDEN["alarm"]["parallel"]),
                          ("parallel", GOLDEN["alarm"]["parallel"])):
        skeleton, sepsets = est.estimate(variant=variant, ci_test="chi_square", return_type="skeleton",
                                         significance_level=ALPHA)
        assert sorted(sorted(e) for e in skeleton.edges()) == want["edges"], variant
        assert sorted([sorted(k), len(v)] for k, v in sepsets.items()) == want["separating_set_sizes"], variant
    assert len(GOLDEN["alarm"]["edges"]) == 33 and len(GOLDEN["alarm"]["parallel"]["edges"]) == 30


def test_simulate_pc_fit_predict(gpu):
    """2,000 simulated alarm rows -> PC (dag) -> fit -> predict_probability on 10 rows, no graph given:
    shapes, acyclicity and finiteness only."""
    from pgmpy_amd.estimators import PC
    from pgmpy_amd.utils import get_example_model

    alarm = get_example_model("alarm")
    df = alarm.simulate(n_samples=2000, seed=3, show_progress=False)
    model = PC(df).estimate(return_type="dag", ci_test="chi_square", max_cond_vars=3, show_progress=False)
    assert set(model.nodes()) == set(alarm.nodes()) and nx.is_directed_acyclic_graph(model)
    assert 20 <= model.number_of_edges()
    model.fit(df)
    assert len(model.get_cpds()) == 37
    hidden = ["HR", "CATECHOL", "BP"]
    prob = model.predict_probability(df.iloc[:10].drop(columns=hidden))
    assert len(prob) == 10 and np.isfinite(prob.to_numpy(dtype=np.float64)).all()
    assert prob.shape[1] == sum(int(model.get_cpds(v).variable_card) for v in hidden)
