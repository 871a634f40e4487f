"""ExpectationMaximization on the device: the E-step kernel (pgm_fit_estep) against the long-double
restatement of tests/em_cases.py on the case table, the estimator against the reference's goldens
(tests/golden/em_cases.json + .npz, which tests/test_em_cpu.py pins the restatement to), its log-likelihood
trace, and the chains fit -> query and simulate -> fit.  Bounds: em_cases.bound / bound_loglik; golden
tolerances: em_cases.golden_tolerance (recorded there, not chosen here)."""
import functools

import numpy as np
import pandas as pd
import pytest

from tests import em_cases as C

pytestmark = pytest.mark.gpu

META, ARRAYS = C.load_golden()
KERNEL_CASES = sorted(C.kernel_cases())


def _dev(a):
    from pgmpy_amd import engine as E

    return E.to_device_raw(np.ascontiguousarray(a))


def _host(t):
    from pgmpy_amd.inference.batch import download

    return download(t)


def _plan(families):
    from pgmpy_amd.estimators._fit import FitPlan

    return FitPlan(families)


def _shape(families, latent_cols):
    """(families with a latent, L) of a case: what the bounds take."""
    card = {c: k for cols, cards in families for c, k in zip(cols, cards)}
    n_lat_fam = sum(any(c in latent_cols for c in cols) for cols, _ in families)
    return n_lat_fam, int(np.prod([card[c] for c in latent_cols]))


@functools.lru_cache(maxsize=None)
def _reference(name, row0=0, pad=0):
    """(inputs, estep_ref of the window) of a kernel case, computed once and left unchanged."""
    families, latent_cols, values, codes = C.case_inputs(name, row0=row0, pad=pad)
    n = C.kernel_cases()[name][2]
    return (families, latent_cols, values, codes), C.estep_ref(families, latent_cols, values, codes[:, row0:row0 + n])


def _assert_equal_the_restatement(families, latent_cols, got_tables, got_loglik, ref, n_rows, key):
    tables, loglik, counted, _ = ref
    n_lat_fam, L = _shape(families, latent_cols)
    want = np.asarray(tables, dtype=np.float64)
    b = C.bound(n_rows, n_lat_fam, L, want)
    worst = np.max(np.abs(got_tables - want) - b)
    print(key, "tables: max error", float(np.max(np.abs(got_tables - want))), "max bound", float(np.max(b)))
    assert worst <= 0, (key, float(worst))
    # the latent-free families hold exact integers
    offsets, sizes, _ = C.layout(families)
    for f, (cols, _) in enumerate(families):
        if not any(c in latent_cols for c in cols):
            assert np.array_equal(got_tables[offsets[f]:offsets[f] + sizes[f]], want[offsets[f]:offsets[f] + sizes[f]]), (key, f)
    if got_loglik is not None:
        want_ll = np.asarray(loglik, dtype=np.float64)
        bl = C.bound_loglik(len(families), L, want_ll)
        print(key, "loglik: max error", float(np.max(np.abs(got_loglik - want_ll))), "min bound", float(np.min(bl)))
        assert np.all(np.abs(got_loglik - want_ll) <= bl), key
        assert np.all(got_loglik[~counted] == 0.0), key


# ---------------------------------------------------------------------------- the kernel cases
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_estep_equals_the_restatement(gpu, name):
    (families, latent_cols, values, codes), ref = _reference(name)
    n = codes.shape[1]
    plan = _plan(families)
    tables, loglik = plan.estep(latent_cols, _dev(values), _dev(codes), want_loglik=True)
    got = _host(tables)
    _assert_equal_the_restatement(families, latent_cols, got, _host(loglik), ref, n, name)
    # every latent family's table sums to the number of counted rows
    n_lat_fam, L = _shape(families, latent_cols)
    offsets, sizes, _ = C.layout(families)
    for f, (cols, _) in enumerate(families):
        total = float(got[offsets[f]:offsets[f] + sizes[f]].sum())
        assert abs(total - n) <= C.bound(n, n_lat_fam, L, n) + n * 2.0 ** -52 * n, (name, f, total)


def test_a_window_inside_a_longer_buffer(gpu):
    """row0 = 5 and ld > row0 + n_rows: the rows before and after the window are not read or written."""
    (families, latent_cols, values, codes), ref = _reference("shared_child", 5, 3)
    n = C.kernel_cases()["shared_child"][2]
    assert codes.shape[1] == 5 + n + 3
    edges = codes.copy()
    edges[:, :5], edges[:, 5 + n:] = 200, 200  # not states: an IndexError if the kernel looked at them
    tables, loglik = _plan(families).estep(latent_cols, _dev(values), _dev(edges), n_rows=n, row0=5, want_loglik=True)
    ll = _host(loglik)
    assert ll.shape == (5 + n + 3,) and np.all(ll[:5] == 0.0) and np.all(ll[5 + n:] == 0.0)
    _assert_equal_the_restatement(families, latent_cols, _host(tables), ll[5:5 + n], ref, n, "window")


def test_two_windows_add_up_to_one_call(gpu):
    (families, latent_cols, values, codes), ref = _reference("mixed")
    n = codes.shape[1]
    plan, dv, dc = _plan(families), _dev(values), _dev(codes)
    whole = _host(plan.estep(latent_cols, dv, dc))
    tables = plan.estep(latent_cols, dv, dc, n_rows=300, row0=0)
    tables = plan.estep(latent_cols, dv, dc, n_rows=n - 300, row0=300, tables=tables)
    _assert_equal_the_restatement(families, latent_cols, _host(tables), None, ref, n, "two windows")
    _assert_equal_the_restatement(families, latent_cols, whole, None, ref, n, "one call")


def test_a_latent_free_family_equals_fit_count(gpu):
    (families, latent_cols, values, codes), _ = _reference("mixed")
    offsets, sizes, _ = C.layout(families)
    got = _host(_plan(families).estep(latent_cols, _dev(values), _dev(codes)))
    plain = [f for f, (cols, _) in enumerate(families) if not any(c in latent_cols for c in cols)]
    assert len(plain) == 2
    counts = _host(_plan([families[f] for f in plain]).count(_dev(codes)))
    mine = np.concatenate([got[offsets[f]:offsets[f] + sizes[f]] for f in plain])
    assert counts.dtype == np.int64 and np.array_equal(mine, counts.astype(np.float64))


def test_entries_of_exactly_zero_meet_the_floor(gpu):
    """Zero for some l: those configurations weigh floor / value.  Zero for every l of a row, L a power of
    two, a uniform prior: the posterior is exactly uniform."""
    families, latent_cols = [([1], [4]), ([0, 1], [3, 4])], [1]  # H:4; X | H
    values = np.concatenate([np.full(4, 0.25), np.array([0.0, 0.0, 0.6, 0.3,    # X = 0: zero for H = 0, 1
                                                         0.0, 0.0, 0.0, 0.0,    # X = 1: zero for every H
                                                         1.0, 1.0, 0.4, 0.7])])
    codes = np.array([[0] * 40 + [1] * 64 + [2] * 24], dtype=np.uint8)
    ref = C.estep_ref(families, latent_cols, values, codes)
    tables, loglik = _plan(families).estep(latent_cols, _dev(values), _dev(codes), want_loglik=True)
    got, ll = _host(tables), _host(loglik)
    _assert_equal_the_restatement(families, latent_cols, got, ll, ref, 128, "zeros")
    # the 64 rows with X = 1 add exactly 1/4 to each state of H and to each entry of their row of X | H
    assert np.array_equal(got[4 + 4:4 + 8], np.full(4, 16.0))
    assert np.all(ll[40:104] == ll[40]) and abs(ll[40] - np.log(1e-10)) <= C.bound_loglik(2, 4, np.log(1e-10))
    # a floored configuration is not dropped: H = 0 given X = 0 weighs 1e-10 / (2e-10 + 0.9) per row
    assert got[4 + 0] > 0 and abs(got[4 + 0] - 40 * 1e-10 / (2e-10 + 0.9)) <= 1e-20


def test_rows_with_a_missing_code_are_not_counted(gpu):
    (families, latent_cols, values, codes), _ = _reference("mixed")
    codes = codes.copy()
    rng = np.random.default_rng(21)
    for col in range(codes.shape[0]):
        codes[col, rng.choice(codes.shape[1], 9, replace=False)] = C.MISSING
    ref = C.estep_ref(families, latent_cols, values, codes)
    counted = ref[2]
    assert 0 < int((~counted).sum()) <= 36 and not ref[3]
    tables, loglik = _plan(families).estep(latent_cols, _dev(values), _dev(codes), want_loglik=True)
    got, ll = _host(tables), _host(loglik)
    _assert_equal_the_restatement(families, latent_cols, got, ll, ref, codes.shape[1], "missing")
    assert np.all(ll[~counted] == 0.0) and np.all(ll[counted] < 0.0)
    offsets, sizes, _ = C.layout(families)
    n_lat_fam, L = _shape(families, latent_cols)
    n = int(counted.sum())
    for f in range(len(families)):  # a row missing in one family's column is missing from every table
        total = float(got[offsets[f]:offsets[f] + sizes[f]].sum())
        assert abs(total - n) <= C.bound(n, n_lat_fam, L, n) + n * 2.0 ** -52 * n, (f, total, n)


def test_a_code_that_is_no_state_raises_and_the_other_rows_are_counted(gpu):
    import torch

    (families, latent_cols, values, codes), _ = _reference("mixed")
    codes = codes.copy()
    codes[1, 17], codes[3, 640] = 3, 200  # column 1 and column 3 have 3 states
    ref = C.estep_ref(families, latent_cols, values, codes)
    assert ref[3] and int((~ref[2]).sum()) == 2
    plan = _plan(families)
    tables = torch.zeros(plan.total_bins, dtype=torch.float64, device=gpu)
    with pytest.raises(IndexError, match="fit_estep: a state code is >= its variable's cardinality"):
        plan.estep(latent_cols, _dev(values), _dev(codes), tables=tables)
    _assert_equal_the_restatement(families, latent_cols, _host(tables), None, ref, codes.shape[1], "bad code")


def test_estep_checks_its_tensors(gpu):
    import torch

    (families, latent_cols, values, codes), _ = _reference("one_child")
    plan, dv, dc = _plan(families), _dev(values), _dev(codes)
    with pytest.raises(ValueError, match="codes must be"):
        plan.estep(latent_cols, dv, dc.to(torch.int32))
    with pytest.raises(ValueError, match="values must be"):
        plan.estep(latent_cols, dv[:-1], dc)
    with pytest.raises(ValueError, match="tables must be"):
        plan.estep(latent_cols, dv, dc, tables=torch.zeros(plan.total_bins, dtype=torch.int64, device=gpu))
    with pytest.raises(ValueError, match="outside ld"):
        plan.estep(latent_cols, dv, dc, n_rows=codes.shape[1], row0=1)
    with pytest.raises(ValueError, match="is in no family"):
        plan.estep([9], dv, dc)


# ---------------------------------------------------------------------------- the estimator against the goldens
def _golden_model(case):
    from pgmpy_amd.models import DiscreteBayesianNetwork

    c = META[case]
    model = DiscreteBayesianNetwork([tuple(e) for e in c["edges"]], latents=set(c["latents"]))
    codes = ARRAYS[f"{c['frame']}_codes"]
    return c, model, pd.DataFrame({v: codes[i].astype(np.int64) for i, v in enumerate(c["observed"])})


def _golden_kwargs(case):
    """The arguments the reference was called with; explicit init_cpds are rebuilt from the recorded values."""
    from pgmpy_amd.factors.discrete import TabularCPD

    c = META[case]
    kwargs = dict(c["kwargs"], latent_card={v: c["cardinality"][v] for v in c["latents"]}, atol=c["atol"])
    if "init_cpds" not in kwargs:
        nodes, families, _, values, _, _ = C.golden_problem(META, ARRAYS, case)
        offsets, sizes, _ = C.layout(families)
        init = {}
        for f, node in enumerate(nodes):
            parents, card = c["parents"][node], c["cardinality"]
            init[node] = TabularCPD(node, card[node], values[offsets[f]:offsets[f] + sizes[f]].reshape(card[node], -1),
                                    evidence=parents or None, evidence_card=[card[p] for p in parents] or None,
                                    state_names={v: list(range(card[v])) for v in [node] + parents})
        kwargs["init_cpds"] = init
    return kwargs


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_get_parameters_equals_the_reference(gpu, case):
    from pgmpy_amd.estimators import ExpectationMaximization

    c, model, df = _golden_model(case)
    tol = C.golden_tolerance(case)
    for key in ("1", "3", "10", "converged"):
        est = ExpectationMaximization(model, df)
        cpds = est.get_parameters(max_iter=100 if key == "converged" else int(key), **_golden_kwargs(case))
        assert est.n_iter_ == (c["n_iter"] if key == "converged" else min(int(key), c["n_iter"])), (case, key, est.n_iter_)
        assert len(est.log_likelihoods_) == est.n_iter_
        assert sorted(cpd.variable for cpd in cpds) == sorted(c["nodes"])
        worst = 0.0
        for cpd in cpds:
            assert list(cpd.variables[1:]) == c["parents"][cpd.variable]
            want = np.asarray(c["results"][key][cpd.variable]).reshape(cpd.variable_card, -1)
            worst = max(worst, float(np.max(np.abs(np.asarray(cpd.get_values()) - want))))
        print(case, key, "max difference", worst, "tolerance", tol)
        assert worst <= tol, (case, key, worst, tol)


def _restated_log_likelihoods(case, k):
    """(k log-likelihoods of the restatement in long double, the bound summed over the rows).  The CPDs
    estimated once are not in the restatement's plan: their term is added from the recorded values."""
    c = META[case]
    nodes, families, latent_cols, values, codes, _ = C.golden_problem(META, ARRAYS, case)
    _, lls, _ = C.em_ref(families, latent_cols, values, codes, k)
    const, n_fixed = np.longdouble(0), 0
    for node in c["nodes"]:
        if node not in nodes:
            assert not c["parents"][node]
            p = np.asarray(c["results"]["1"][node], dtype=np.longdouble)
            const, n_fixed = const + np.log(p[codes[c["observed"].index(node)]]).sum(), n_fixed + 1
    n, (_, L) = codes.shape[1], _shape(families, latent_cols)
    per_row = np.full(n, float(lls[0] + const) / n)
    return [float(x + const) for x in lls], float(np.sum(C.bound_loglik(len(families) + n_fixed, L, per_row)))


@pytest.mark.parametrize("case", ["a", "c"])
def test_the_log_likelihood_trace(gpu, case):
    """The trace equals the restatement's within the bound summed over the rows, over the first three
    iterations: from the second on the two start from parameters that differ by the order of the additions
    (some 1e-16), which the likelihood of n rows magnifies by about n per unit of probability, so only
    the first iterations stay inside a bound that covers one evaluation.  It does not decrease over ten
    iterations, up to that bound (MLE, positive initial values: the floor is inactive)."""
    from pgmpy_amd.estimators import ExpectationMaximization

    _, model, df = _golden_model(case)
    est = ExpectationMaximization(model, df)
    est.get_parameters(max_iter=10, **_golden_kwargs(case))
    got = est.log_likelihoods_
    want, slack = _restated_log_likelihoods(case, 3)
    print(case, "log-likelihoods", got, "restated", want, "bound", slack)
    assert len(got) == min(10, META[case]["n_iter"])
    for g, w in zip(got, want):
        assert abs(g - w) <= slack, (case, g, w, slack)
    assert all(b >= a - slack for a, b in zip(got, got[1:])), got


# ---------------------------------------------------------------------------- integration
def test_fit_then_query_the_latent(gpu):
    from pgmpy_amd.estimators import ExpectationMaximization
    from pgmpy_amd.inference import VariableElimination

    c, model, df = _golden_model("c")
    assert model.fit(df, estimator=ExpectationMaximization, latent_card={"Z": 3}, seed=1, max_iter=20) is model
    assert model.check_model()
    nodes = c["nodes"]
    families = [([nodes.index(v) for v in [n] + c["parents"][n]], [c["cardinality"][v] for v in [n] + c["parents"][n]])
                for n in nodes]
    values = np.concatenate([np.asarray(model.get_cpds(n).get_values()).ravel() for n in nodes])
    assert all(list(model.get_cpds(n).variables[1:]) == c["parents"][n] for n in nodes)
    ve = VariableElimination(model)
    for r in (0, 7, 311):
        row = {v: int(df[v].iloc[r]) for v in c["observed"]}
        codes = np.zeros((len(nodes), 1), dtype=np.uint8)
        for v, s in row.items():
            codes[nodes.index(v), 0] = s
        tables, _, _, _ = C.estep_ref(families, [nodes.index("Z")], values, codes)
        posterior = np.asarray(tables[:3], dtype=np.float64)  # the latent's own family: w_l
        got = np.asarray(ve.query(["Z"], evidence=row, show_progress=False).values)
        assert np.max(np.abs(got - posterior)) <= 1e-12, (r, got, posterior)


def test_simulate_then_fit_with_the_latents_hidden(gpu):
    from pgmpy_amd.estimators import ExpectationMaximization
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.models import DiscreteBayesianNetwork

    edges = [("H", "A"), ("H", "B"), ("A", "C"), ("G", "C")]
    truth = DiscreteBayesianNetwork(edges, latents={"H", "G"})
    card = {"H": 3, "G": 2, "A": 2, "B": 3, "C": 2}
    for node in truth.nodes():
        parents = truth.get_parents(node)
        truth.add_cpds(TabularCPD.get_random(node, parents, {v: card[v] for v in [node] + parents}, seed=len(node) + card[node]))
    df = truth.simulate(n_samples=400, include_latents=False, seed=3, show_progress=False)
    assert sorted(df.columns) == ["A", "B", "C"]
    model = DiscreteBayesianNetwork(edges, latents={"H", "G"})
    model.fit(df, estimator=ExpectationMaximization, latent_card={"H": 3, "G": 2}, max_iter=3, seed=0)
    assert model.check_model()
    assert model.get_cpds("H").variable_card == 3 and model.get_cpds("C").get_values().shape == (2, 4)
