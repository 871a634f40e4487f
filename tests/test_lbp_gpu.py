"""LoopyBeliefPropagation on the device (csrc/pgmlbp.hip k_lbp) against brute force on trees and the longdouble
restatement of tests/lbp_cases.py on graphs with loops, within 8 x the case's figure (lbp_cases.figure)."""
import numpy as np
import pytest

from tests import lbp_cases as C

pytestmark = pytest.mark.gpu
LOOPY = ["grid_2x3", "grid_6x6", "pair_70", "chain_120"]
same_bits = lambda a, b: a.shape == b.shape and a.tobytes() == b.tobytes()


def launch(case, unaries, n_iter, tol=0.0, damping=0.0, state=None):
    """One launch (unaries None: the case's own); host arrays (marginals, values, iterations, factor beliefs, state)."""
    from pgmpy_amd import engine as E
    from pgmpy_amd.inference._lbp import LbpPlan
    from pgmpy_amd.inference.batch import download

    theta = np.concatenate([t.ravel() for _, t in case[2]])
    unaries = np.concatenate(case[1])[None, :] if unaries is None else unaries
    out = LbpPlan(case[0], [vs for vs, _ in case[2]], theta).run(
        E.to_device(unaries), E.to_device(theta), n_iter, tol, damping, want_beliefs=True, want_state=True,
        state=None if state is None else E.to_device(state))
    return [download(x) for x in out]


def model_of(case, state_names=False):
    """(LoopyBeliefPropagation of the case as a DiscreteMarkovNetwork with its node terms as unary factors, names)."""
    from pgmpy_amd.factors.discrete import DiscreteFactor
    from pgmpy_amd.inference import LoopyBeliefPropagation
    from pgmpy_amd.models import DiscreteMarkovNetwork

    card, unary, factors = case
    names = [f"x{v}" for v in range(len(card))]
    model = DiscreteMarkovNetwork()
    model.add_nodes_from(names)
    for vs, table in factors + [((v,), unary[v]) for v in range(len(card))]:
        model.add_edges_from((names[a], names[b]) for a in vs for b in vs if a < b)
        states = {names[v]: [f"s{i}" for i in range(card[v])] for v in vs} if state_names else {}
        model.add_factors(DiscreteFactor([names[v] for v in vs], [card[v] for v in vs], table, state_names=states))
    return LoopyBeliefPropagation(model), names


# the figures: chain 5.3e-16, star 1.4e-15, triple 2.5e-16 (log Z between 3 and 8); grid_2x3 8.2e-16 (log Z 8.6),
# grid_6x6 2.1e-14 (log Z 50.8), pair_70 6.3e-16 (log Z 8.8), chain_120 7.4e-16 (log Z 14.8)
@pytest.mark.parametrize("name, damping", [(n, 0.0) for n in sorted(C.TREES)] + [(n, d) for n in LOOPY for d in (0.0, 0.5)])
def test_against_brute_force_or_longdouble(gpu, name, damping):
    """Trees after diameter + 1 iterations against brute force; loopy cases after 8, messages and residual too."""
    case, n_iter = C.CASES[name], C.TREES[name] + 1 if name in C.TREES else 8
    ref, fig = C.figure(name, n_iter, damping)
    m, values, iters, fb, state = launch(case, None, n_iter, 0.0, damping)
    want = C.brute_force(case) if name in C.TREES else (ref["marginals"], ref["factor_beliefs"], ref["logz"])
    pairs = [(m[0], want[0]), (fb[0], want[1]), (values[0, 0], want[2])]
    pairs += [] if name in C.TREES else [(state[0], ref["state"]), (values[0, 1], ref["residual"])]
    gaps = [float(np.abs(x - y).max()) for x, y in pairs]
    print(name, damping, "figure", fig, "marginals, factor beliefs, log Z, messages, residual:", gaps)
    assert iters[0] == n_iter and max(gaps) <= 8 * fig


def test_batch_rows_stop_alone_and_equal_their_own_runs(gpu):
    from pgmpy_amd import engine as E
    from pgmpy_amd.inference.batch import download

    (un, refs), case = C.batch(), C.CASES["grid_2x3"]
    lbp, _ = model_of((case[0], [np.ones(k) for k in case[0]], case[2]))
    run = lambda rows: lbp.query_batch(E.to_device(rows), 40, C.BATCH_TOL, return_state=True, return_factor_beliefs=True)
    got = run(un)
    assert list(download(got.n_iter)) == [r["n_iter"] for r in refs] == [7, 8, 2, 8, 8]
    for b in range(len(un)):
        alone = run(un[b:b + 1])
        for key in ("marginals", "values", "factor_beliefs", "state"):
            assert same_bits(download(getattr(got, key))[b:b + 1], download(getattr(alone, key))), (b, key)


def test_resume_equals_one_run(gpu):
    case = C.CASES["grid_2x3"]
    whole, half = launch(case, None, 20), launch(case, None, 10)
    rest = launch(case, None, 10, state=half[4])
    assert all(same_bits(whole[i], rest[i]) for i in (0, 1, 3, 4)) and rest[2][0] == 10


def test_contradiction_ends_its_row_alone(gpu):
    case = C.CONTRADICTION
    un = np.array([[1.0, 1.0, 1.0, 1.0], [1.0, 0.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]])  # row 1 forces x0 = 0, the table forbids it
    got, alone = launch(case, un, 5), launch(case, un[:1], 5)
    assert list(got[2]) == [5, -1, 5] and all(np.isnan(got[i][1]).all() for i in (0, 1, 3))
    assert all(same_bits(got[i][b:b + 1], alone[i]) for i in (0, 1, 3, 4) for b in (0, 2))
    with pytest.raises(ValueError, match="contradicts"):
        model_of(case)[0].query(["x1"], evidence={"x0": 0})


def test_query_with_evidence_and_state_names(gpu):
    (card, unary, factors), (lbp, names) = C.CASES["star"], model_of(C.CASES["star"], state_names=True)
    got = lbp.query(["x0", "x2", "x5"], evidence={"x3": "s1"})
    seen = [u * np.eye(k)[1] if v == 3 else u for v, (k, u) in enumerate(zip(card, unary))]
    marg, fbel, logz = C.brute_force((card, seen, factors))
    tol, off = 8 * C.figure("star", C.TREES["star"] + 1)[1], np.cumsum([0] + card)
    for v in (0, 2, 5):
        f = got[names[v]]
        assert f.variables == [names[v]] and f.state_names[names[v]] == [f"s{i}" for i in range(card[v])]
        assert np.abs(np.asarray(f.values) - marg[off[v]:off[v + 1]]).max() <= tol
    belief = lbp.factor_beliefs()[("x2", "x0")]  # the second factor: cells 6 .. 17 of the factor beliefs
    assert np.abs(np.asarray(belief.values).ravel() - fbel[6:18]).max() <= tol
    assert abs(lbp.log_partition() - logz) <= tol and 0 < lbp.n_iter_used < 100
