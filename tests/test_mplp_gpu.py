"""Mplp on the device (csrc/pgmmplp.hip k_mplp) against the numpy restatement of tests/mplp_cases.py."""
import numpy as np
import pytest

from tests import mplp_cases as M

pytestmark = pytest.mark.gpu
THR = 0.0002


def mplp_of(case):
    from pgmpy_amd.factors.discrete import DiscreteFactor
    from pgmpy_amd.inference import Mplp
    from pgmpy_amd.models import DiscreteMarkovNetwork

    card, unary, clusters, n_trip = case
    names = [f"x{v}" for v in range(len(card))]
    model = DiscreteMarkovNetwork()
    model.add_nodes_from(names)
    factors = [DiscreteFactor([names[v]], [card[v]], unary[v]) for v in range(len(card))]
    for vs, theta in clusters[:len(clusters) - n_trip]:
        model.add_edge(names[vs[0]], names[vs[1]])
        factors.append(DiscreteFactor([names[v] for v in vs], [card[v] for v in vs], theta))
    model.add_factors(*factors)
    return Mplp(model), [tuple(names[v] for v in vs) for vs, _ in clusters[len(clusters) - n_trip:]]


def launch(mplp, unaries, n_iter, thr, triplets=None, state=None):
    """One launch; host arrays (codes, values [B, 4], iterations, state)."""
    from pgmpy_amd import engine as E
    from pgmpy_amd.inference.batch import download

    r = mplp.map_query_batch(E.to_device(unaries), n_iter, thr, thr, triplets=triplets,
                             state=None if state is None else E.to_device(state), return_state=True)
    return download(r.codes), download(r.values), download(r.n_iter), download(r.state)


def own_unaries(case):
    return np.concatenate(case[1])[None, :]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64),
                                                 np.asarray(b, dtype=np.float64).view(np.int64))


def values_of(ref):
    return np.array([ref[k] for k in ("best", "dual_lp", "dual_gap", "int_gap")], dtype=np.float64)


@pytest.mark.parametrize("name", ["grid", "chord"])
def test_exact_cases_bit_for_bit(gpu, name):
    """Dyadic terms, k = 1 or 2, 20 iterations: codes, values, gaps and the whole state equal the float64
    restatement bit for bit.  The halvings round after some ten iterations (a bit per update along a chain), so
    this holds because the operations and their order are the same, the two sums' lattice included."""
    case = M.EXACT[name]
    ref = M.run(case, 20)
    codes, values, iters, state = launch(mplp_of(case)[0], own_unaries(case), 20, 0.0)
    assert iters[0] == 20 and np.array_equal(codes[0], ref["codes"])
    assert same_bits(values[0], values_of(ref)) and same_bits(state[0], ref["state"])


@pytest.mark.parametrize("name", ["doc", "grid"])
def test_against_longdouble(gpu, name):
    case = M.NEAR[name]
    ref, fig = M.figure(case, 40)
    assert min(t[2] for t in ref["trace"]) > 1e-6  # no decode is near a tie
    tol = 8 * fig  # the measured figure: 7.6e-13 (doc, values near 4400), 2.9e-15 (grid, values near 6.6)
    codes, values, iters, _ = launch(mplp_of(case)[0], own_unaries(case), 40, THR)
    print(name, "figure", fig, "primal", values[0, 0] - float(ref["best"]), "dual", values[0, 1] - float(ref["dual_lp"]))
    assert np.array_equal(codes[0], ref["codes"]) and iters[0] == ref["n_iter"]
    assert abs(values[0, 0] - float(ref["best"])) <= tol and abs(values[0, 1] - float(ref["dual_lp"])) <= tol


@pytest.mark.parametrize("name", ["triangle", "signs_2x3"])
def test_weak_duality_and_tightening(gpu, name):
    case = M.triangle() if name == "triangle" else M.signs_2x3()
    top, tol = M.brute_force(case), 8 * M.figure(case, 100)[1]
    mplp, _ = mplp_of(case)
    _, values, _, _ = launch(mplp, own_unaries(case), 100, THR)
    assert values[0, 0] <= top + tol and top <= values[0, 1] + tol
    if name == "triangle":
        assert values[0, 3] > THR  # the pairwise relaxation is loose
        tight = M.triangle(1)
        _, values, _, _ = launch(mplp, own_unaries(case), 100, THR, triplets=mplp_of(tight)[1])
        assert values[0, 0] <= top + tol and top <= values[0, 1] + tol
        found = mplp.map_query(tighten_triplet=True)
        x = [found[f"x{v}"] for v in range(3)]
        value = sum(case[1][v][x[v]] for v in range(3)) + sum(t[tuple(x[v] for v in vs)] for vs, t in case[2])
        assert abs(value - top) <= tol and mplp.get_integrality_gap() < THR and len(mplp._triplets) == 1


def test_batch_rows_equal_their_own_runs(gpu):
    case = M.EXACT["grid"]
    mplp, unaries = mplp_of(case)[0], M.batch_unaries(case)
    batch = launch(mplp, unaries, 40, THR)
    for b in range(len(unaries)):
        alone = launch(mplp, unaries[b:b + 1], 40, THR)
        assert all(same_bits(x[b:b + 1], y) for x, y in zip(batch, alone)), b
    ref = M.run(M.with_unary(case, unaries[50]), 40, THR, THR)
    assert ref["n_iter"] == 17 == batch[2][50] and batch[2][49] == 40 == batch[2][51]
    assert same_bits(batch[1][50], values_of(ref)) and same_bits(batch[3][50], ref["state"])


def test_resume_equals_one_run(gpu):
    case = M.EXACT["grid"]
    mplp, un = mplp_of(case)[0], own_unaries(case)
    whole, half = launch(mplp, un, 20, 0.0), launch(mplp, un, 10, 0.0)
    rest = launch(mplp, un, 10, 0.0, state=half[3])
    assert all(same_bits(whole[i], rest[i]) for i in (0, 1, 3)) and rest[2][0] == 10
