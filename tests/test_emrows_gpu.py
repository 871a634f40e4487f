"""The rows E-step on the device (pgm_fit_estep_rows) against the brute-force long-double restatement of
tests/emrows_cases.py, then the estimator and the scorer built on it.  Bounds: emrows_cases.atol / atol_loglik."""
import numpy as np
import pandas as pd
import pytest

from tests import emrows_cases as C

pytestmark = pytest.mark.gpu
F64 = np.float64


def _run(c, codes=None, n_rows=None):
    """(plan, tables, loglik, status, n_skipped) of a case on the device, downloaded."""
    from pgmpy_amd import engine as E
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.inference.batch import download

    plan, codes = FitPlan(c["families"]), np.ascontiguousarray(c["codes"] if codes is None else codes)
    out = plan.estep_rows(c["latent"], E.to_device_raw(c["values"]), E.to_device_raw(codes), n_rows=n_rows or c["n_rows"],
                          row0=c["row0"], want_loglik=True, want_status=True, no_floor=c["no_floor"])
    return plan, download(out["tables"]), download(out["loglik"]), download(out["status"]), out["n_skipped"]


@pytest.mark.parametrize("name", C.NAMES)
def test_estep_rows_equals_the_brute_force(gpu, name):
    c = C.case(name)
    tables, loglik, status, adds, logsum = C.expected(name)
    plan, got, got_ll, got_status, got_skipped = _run(c)
    assert bool(plan.estep_rows_info(c["latent"]).tile) == c["tile"]
    lo, hi = c["row0"], c["row0"] + c["n_rows"]
    assert np.array_equal(got_status[lo:hi], status) and got_skipped == (status == 2).sum() == len(c["skip"]) + (name == "unobserved33")
    assert np.all(np.isnan(got_ll[:lo])) and np.all(np.isnan(got_ll[hi:]))  # outside the window: not written
    want = tables.astype(F64)
    assert np.all(np.abs(got - want) <= C.atol(c, want, adds)), (name, float(np.abs(got - want).max()))
    want_ll, got_ll, fin = loglik.astype(F64), got_ll[lo:hi], np.isfinite(loglik.astype(F64))
    assert np.array_equal(got_ll[~fin], want_ll[~fin], equal_nan=True)  # NaN skipped, -inf impossible
    bound_ll = C.atol_loglik(c, logsum)
    assert np.all(np.abs(got_ll - want_ll)[fin] <= bound_ll[fin]), (name, float(np.abs(got_ll - want_ll)[fin].max()))
    if name == "complete":  # nothing added; the log-probability of complete rows
        from pgmpy_amd import engine as E
        from pgmpy_amd.inference.batch import download
        logp, _, _ = plan.logprob(plan.log_values(E.to_device_raw(c["values"])), E.to_device_raw(c["codes"]))
        assert not got.any() and not status.any() and np.all(np.abs(got_ll - download(logp)) <= bound_ll)
    if name == "zero_no_floor":  # same rows as zero_floor: the floor changes the result, and only its absence is impossible
        floored = C.expected("zero_floor")
        assert (status == 3).any() and not (floored[2] == 3).any() and not np.array_equal(tables, floored[0])


def test_a_row_is_bit_identical_wherever_it_sits(gpu):
    c = C.case("latent_missing")
    _, _, ll, st, _ = _run(c)
    order = np.random.default_rng(3).permutation(c["n_rows"])
    _, _, ll2, st2, _ = _run(c, codes=c["codes"][:, order])
    assert np.array_equal(ll2, ll[order], equal_nan=True) and np.array_equal(st2, st[order])
    for r in (0, 17, 199):  # alone
        _, _, ll1, st1, _ = _run(c, codes=c["codes"][:, r:r + 1], n_rows=1)
        assert ll1[0] == ll[r] and st1[0] == st[r]


def _frame(codes, names):
    df = pd.DataFrame({v: codes[i].astype(F64) for i, v in enumerate(names)})
    return df.where(df != C.MISSING)


def _cpds(families, values, names):
    """{node: TabularCPD} of flat values; the states of a data column are floats, as a frame with NaN has them."""
    from pgmpy_amd.factors.discrete import TabularCPD

    out, (offsets, sizes, _) = {}, C.layout(families)
    for (cols, cards), o, s in zip(families, offsets, sizes):
        scope = [names[c] for c in cols]
        out[scope[0]] = TabularCPD(scope[0], cards[0], np.asarray(values[o:o + s], dtype=F64).reshape(cards[0], -1),
                                   evidence=scope[1:] or None, evidence_card=cards[1:] or None,
                                   state_names={v: [float(x) if v != "H" else x for x in range(k)] for v, k in zip(scope, cards)})
    return out


def _worst(cpds, families, want, names):
    mine = _cpds(families, want, names)
    return max(float(np.max(np.abs(cpd.get_values() - mine[cpd.variable].get_values()))) for cpd in cpds if cpd.variable in mine)


def test_em_marginalises_the_missing_cells(gpu):
    from pgmpy_amd.estimators import ExpectationMaximization
    from pgmpy_amd.models import DiscreteBayesianNetwork

    edges = [("H", "A"), ("H", "B"), ("A", "C"), ("B", "D")]
    codes, values = C.em_problem()
    want, want_ll = C.em_ref(C.EM_FAMILIES, [4], codes, values, 3)
    df = _frame(codes, "ABCD")
    kw = dict(latent_card={"H": 2}, max_iter=3, atol=0, init_cpds=_cpds(C.EM_FAMILIES, values, "ABCDH"))
    est = ExpectationMaximization(DiscreteBayesianNetwork(edges, latents={"H"}), df, incomplete="marginalize")
    worst = _worst(est.get_parameters(**kw), C.EM_FAMILIES, want, "ABCDH")
    assert est.n_iter_ == 3 and est.n_skipped_ == 0 and worst <= 64 * C.EM_FP64_VS_LONGDOUBLE, worst
    lls = est.log_likelihoods_
    assert all(abs(g - float(w)) <= 1e-9 * abs(float(w)) for g, w in zip(lls, want_ll))
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(lls, lls[1:])), lls
    # "drop" (here through fit) is today's path, the rows with a missing cell dropped.  pgm_fit_estep adds with fp64 atomics
    # in no fixed order, so two runs agree to the order of the additions only: <= 300 weights per entry, three iterations
    a = DiscreteBayesianNetwork(edges, latents={"H"}).fit(df, estimator=ExpectationMaximization, incomplete="drop", **kw)
    b = ExpectationMaximization(DiscreteBayesianNetwork(edges, latents={"H"}), df.dropna())
    for x, y in zip(sorted(a.get_cpds(), key=lambda cpd: cpd.variable), sorted(b.get_parameters(**kw), key=lambda cpd: cpd.variable)):
        assert x.variable == y.variable and np.max(np.abs(x.get_values() - y.get_values())) <= 3 * (300 + 64) * 2.0 ** -52


def test_log_probability_marginalises_the_missing_cells(gpu):
    """Rows without NaN equal the complete-row path within atol_loglik, not bit for bit: that path adds the families one
    after the other, this one per lane and then by a butterfly."""
    from pgmpy_amd.metrics import BayesianModelProbability
    from pgmpy_amd.models import DiscreteBayesianNetwork

    c = C.case("vstructure")
    _, loglik, status, _, logsum = C.brute_force(c["families"], [], c["values"], c["codes"], no_floor=True)
    model = DiscreteBayesianNetwork([("A", "C"), ("B", "C")])
    model.add_cpds(*_cpds(c["families"], c["values"], "ABC").values())
    df, scorer = _frame(c["codes"], "ABC"), BayesianModelProbability(model)
    got, bound = scorer.log_probability(df, incomplete="marginalize"), C.atol_loglik(c, logsum)
    assert (status == 1).any() and np.all(np.abs(got - loglik.astype(F64)) <= bound)
    assert np.all(np.abs(got[status == 0] - scorer.log_probability(df[status == 0])) <= bound[status == 0])
    with pytest.raises(ValueError):
        scorer.log_probability(df)
