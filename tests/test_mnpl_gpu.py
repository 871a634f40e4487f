"""The pseudo-likelihood kernels (csrc/pgmmnpl.hip k_mn_pl, k_mn_pl_gather) and the estimator on them against the
row-by-row longdouble reference of tests/mnpl_cases.py, within the bound derived there (mnpl_cases.atol)."""
from functools import lru_cache

import numpy as np
import pytest

from tests import mnpl_cases as C

pytestmark = pytest.mark.gpu
CASES = C.cases(163840 - 256)  # pgm_mnpl_info_t.lds_max; test_mnpl_cpu.py checks the figure against the library


@lru_cache(maxsize=None)
def reference(name):
    case = CASES[name]
    return C.reference(case["card"], case["scopes"], case["codes"], case["theta"])


def launch(case, l2=0.0):
    """(value, node_values, grad) on the host from one count launch and one evaluation."""
    from pgmpy_amd import engine as E
    from pgmpy_amd.estimators._mnpl import MnplPlan
    from pgmpy_amd.inference.batch import download

    codes = E.to_device_raw(case["codes"])  # first: the upload brings torch's HIP runtime in before the library loads
    plan = MnplPlan([(list(s), [case["card"][v] for v in s]) for s in case["scopes"]], case["card"])
    counts = plan.fit_plan().count(codes)
    value, grad, node_values = plan.eval(counts, E.to_device(case["theta"]), l2, want_node_values=True)
    return float(download(value)[0]), download(node_values), download(grad)


@pytest.mark.parametrize("name", list(CASES))
def test_value_and_gradient_against_the_reference(name):
    case = CASES[name]
    want_value, want_nodes, want_grad, dev = reference(name)
    assert np.isfinite(np.float64(want_value)) and np.isfinite(want_grad.astype(np.float64)).all()
    value, node_values, grad = launch(case)
    n_rows = case["codes"].shape[1]
    tol = C.atol(case["card"], case["scopes"], n_rows, dev)
    tol_value = C.atol(case["card"], case["scopes"], n_rows, dev, whole=True)
    err = (abs(value - want_value), np.abs(node_values - want_nodes).max(), np.abs(grad - want_grad).max())
    print(f"{name}: errors value {float(err[0]):.3e} (bound {tol_value:.3e}), node {float(err[1]):.3e}, "
          f"grad {float(err[2]):.3e} (bound {tol:.3e})")
    assert err[0] <= tol_value and err[1] <= tol and err[2] <= tol


def test_ridge_term():
    case, l2 = CASES["triangle"], 0.375
    value, _, grad = launch(case, l2)
    plain_value, _, plain_grad = launch(case)
    theta = case["theta"]
    assert np.abs(grad - (plain_grad - l2 * theta)).max() <= 2.0 ** -52 * (np.abs(plain_grad).max() + l2 * 2)  # one rounding
    assert abs(value - (plain_value - 0.5 * l2 * np.dot(theta, theta))) <= 8 * 2.0 ** -53 * abs(plain_value) * len(theta)


def test_bits_do_not_depend_on_the_rest_of_the_plan_or_on_the_launch():
    same_bits = lambda a, b: a.shape == b.shape and a.tobytes() == b.tobytes()
    chain = CASES["chain"]
    alone, both = launch(chain), launch(C.joined(chain, CASES["grid"]))
    n, k = len(chain["theta"]), len(chain["card"])
    assert same_bits(alone[2], both[2][:n]) and same_bits(alone[1], both[1][:k])
    again = launch(C.joined(chain, CASES["grid"]))
    assert all(same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(both, again))


def model_of(card, scopes):
    from pgmpy_amd.models import DiscreteMarkovNetwork

    names = [f"x{v}" for v in range(len(card))]
    model = DiscreteMarkovNetwork()
    model.add_nodes_from(names)
    for s in scopes:
        model.add_edges_from((names[a], names[b]) for a in s for b in s if a < b)
    return model, names


@pytest.mark.parametrize("card,scopes,seed", [(*C.CHAIN, 11), (*C.TRIANGLE, 12)])
def test_fit_recovers_a_distribution_of_the_family(card, scopes, seed):
    from pgmpy_amd import engine as E
    from pgmpy_amd.estimators import PseudoLikelihoodEstimator
    from pgmpy_amd.inference import LoopyBeliefPropagation
    from pgmpy_amd.sampling import GibbsSampling

    codes, log_phi = C.family_data(card, scopes, seed)
    n_rows, t = codes.shape[1], 1e-8
    model, names = model_of(card, scopes)
    est = PseudoLikelihoodEstimator.from_codes(model, E.to_device_raw(codes), card=dict(zip(names, card)),
                                               scopes=[[names[v] for v in s] for s in scopes])
    factors = est.estimate(tol=t)
    assert est.converged
    theta = np.log(np.concatenate([np.asarray(f.values, dtype=np.float64).ravel() for f in factors]))
    value, _, grad, dev = C.reference(card, scopes, codes, theta)
    best = C.reference(card, scopes, codes, log_phi)[0]
    print(f"fit: {est.n_iter} iterations, {est.n_eval} evaluations, max|g|/n {float(np.abs(grad).max()) / n_rows:.3e}, "
          f"PL - PL(log phi) {float(value - best):.3e}")
    assert np.abs(grad).max() / n_rows <= t + C.atol(card, scopes, n_rows, dev) / n_rows
    assert value >= best - C.atol(card, scopes, n_rows, dev, whole=True)
    # the loop on resident data: sample from the fit, fit the sample, and hand the result on as it stands
    model.add_factors(*factors)
    drawn, nodes = GibbsSampling(model).sample_codes(512, 20, seed=3)
    model.fit_codes(drawn, nodes, l2=1e-3, tol=1e-6)
    assert [tuple(f.variables) for f in model.factors] == [tuple(names[v] for v in s) for s in scopes]
    marginals = LoopyBeliefPropagation(model).query([names[0]])
    assert abs(float(np.asarray(marginals[names[0]].values).sum()) - 1.0) < 1e-9
    assert GibbsSampling(model).sample_codes(64, 2, seed=4)[0].shape == (len(card), 64)
