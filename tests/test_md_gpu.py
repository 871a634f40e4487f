"""MirrorDescentEstimator on the device (csrc/pgmmd.hip k_md) against the longdouble restatement of tests/md_cases.py,
whose calibration is brute force on the joint: mu / n and theta / max(1, |theta|) within md_cases.tolerance (8 x the
case's float64-against-longdouble figure), the loss to the same relative size, alpha and both trial counts exactly."""
import numpy as np
import pytest

from pgmpy_amd import _native as N
from tests import md_cases as C

pytestmark = pytest.mark.gpu
same_bits = lambda a, b: a.shape == b.shape and a.tobytes() == b.tobytes()


def launch(name, tier=N.MD_TIER_AUTO, rows=slice(None)):
    """One launch of the case's rows; host arrays (theta, mu, values, trials)."""
    from pgmpy_amd import engine as E
    from pgmpy_amd.estimators._md import MdPlan
    from pgmpy_amd.inference.batch import download

    case = C.CASES[name]
    targets = E.to_device(case["targets"][rows])  # before the plan: torch is imported before the library is loaded
    plan = MdPlan(case["card"], case["cliques"], case["edges"], case["marginals"])
    plan.set_tier(tier)
    theta = np.concatenate([t.ravel() for t in case["theta"]])[None, :]
    out = plan.run(targets, E.to_device(case["totals"][rows]), E.to_device(theta), case["metric"], case["iterations"], case["stepsize"])
    return [download(x) for x in out]


def check(name, got, row, b=0):
    (ref, _, _), (tol, scale), n = C.reference(name, row), C.tolerance(name, row), C.CASES[name]["totals"][row]
    theta, mu, values, trials = (x[b] for x in got)
    gaps = [float(np.abs(mu - ref["mu"]).max()) / n, float(np.abs(theta - ref["theta"]).max()) / scale,
            abs(values[0] - float(ref["loss"])) / (n * n * len(C.CASES[name]["targets"][row]))]
    print(name, row, "tolerance", tol, "mu / n, theta, loss / (n^2 n_y):", gaps, "trials", list(trials), "alpha", values[1])
    assert list(trials) == [ref["trials"], ref["rejected"]] and values[1] == ref["alpha"] and max(gaps) <= tol


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_against_the_longdouble_reference(gpu, name):
    got = launch(name)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()  # "hot": log space stays finite
    for row in range(len(C.CASES[name]["totals"])):
        check(name, got, row, row)


@pytest.mark.parametrize("name", C.GLOBAL_TIER)
def test_global_tier_forced(gpu, name):
    check(name, launch(name, tier=N.MD_TIER_GLOBAL), 0)


def test_batch_rows_equal_their_own_runs(gpu):
    got = launch("batch")
    for b in range(3):
        alone = launch("batch", rows=slice(b, b + 1))
        assert all(same_bits(x[b:b + 1], y) for x, y in zip(got, alone)), b


def star_estimator():
    import pandas as pd
    from pgmpy_amd.estimators import MirrorDescentEstimator
    from pgmpy_amd.factors.discrete import DiscreteFactor
    from pgmpy_amd.models import JunctionTree

    model = JunctionTree()
    model.add_edges_from([(("a", "b"), ("b", "c")), (("b", "c"), ("c", "d")), (("b", "c"), ("c", "e"))])
    model.add_factors(*[DiscreteFactor(node, [2, 2], np.ones((2, 2))) for node in model.nodes()])
    return MirrorDescentEstimator(model, pd.DataFrame(C.STAR_ROWS, columns=list("abcde")))


def test_estimate_on_the_star_and_warm_start(gpu):
    """The public path on the reference's star (its cliques as marginals, 8 iterations of the line search), then
    2 + 3 iterations of a fixed step on one estimator against 5 in one call."""
    est = star_estimator()
    tree = est.estimate(marginals=list(est.belief_propagation.junction_tree.nodes()), iterations=8)
    (ref, _, _), (tol, _) = C.reference("star_cliques"), C.tolerance("star_cliques")
    for i, clique in enumerate([("a", "b"), ("b", "c"), ("c", "d"), ("c", "e")]):
        f = tree.clique_beliefs[clique]
        got = np.transpose(np.asarray(f.values), [f.variables.index(v) for v in clique]).ravel()
        assert np.abs(got - ref["mu"][4 * i:4 * i + 4]).max() / 5 <= tol
    one, two = star_estimator(), star_estimator()
    whole = one.estimate([("c",), ("b", "c"), ("e",)], iterations=5, stepsize=0.1)
    two.estimate([("c",), ("b", "c"), ("e",)], iterations=2, stepsize=0.1)
    rest = two.estimate([("c",), ("b", "c"), ("e",)], iterations=3, stepsize=0.1)
    for c in whole.nodes():  # bit for bit: an accepted trial's theta is recomputed into omega by the same expression
        assert same_bits(np.asarray(whole.clique_beliefs[c].values), np.asarray(rest.clique_beliefs[c].values))
        assert same_bits(np.asarray(one.theta[c].values), np.asarray(two.theta[c].values))


@pytest.mark.parametrize("marginals, printed", [([("a", "b")], [1, 1, 1, 2]), ([("a",)], [1, 1, 1.5, 1.5])])
def test_docstring_examples_of_the_reference(gpu, marginals, printed):
    import pandas as pd
    from pgmpy_amd.estimators import MirrorDescentEstimator
    from pgmpy_amd.factors.discrete import DiscreteFactor
    from pgmpy_amd.models import FactorGraph

    data = pd.DataFrame(data={"a": [0, 0, 1, 1, 1], "b": [0, 1, 0, 1, 1]})
    model, phi = FactorGraph(), DiscreteFactor(["a", "b"], [2, 2], np.zeros(4))
    model.add_nodes_from(["a", "b"])
    model.add_factors(phi)
    model.add_edges_from([("a", phi), ("b", phi)])
    f = MirrorDescentEstimator(model=model, data=data).estimate(marginals=marginals).factors[0]
    values = np.transpose(np.asarray(f.values), [f.variables.index(v) for v in ("a", "b")]).ravel()
    assert np.round(values, 4).tolist() == printed  # as the reference prints them
    with pytest.raises(ValueError, match="No data was found"):
        MirrorDescentEstimator(model=model, data=None).estimate(marginals=marginals)
