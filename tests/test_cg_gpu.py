"""The conditional-Gaussian scores on the device against the long-double restatement of tests/cg_cases.py:
k_cg_moments at every operand-layout boundary, k_cg_score in every case of the density, bit-identity, and the
Python layer up to one HillClimbSearch over mixed data.

Bounds: a moment is a sum of n products of shifted values, so the Gram tests' derived bound (n + 2) u sum|a b|
(tests/lg_cases.py gram_bound) holds for it and is used instead of the parity band; a score is held to
|got - want| <= 1e-9 max(1, |want|).  Largest errors observed on an MI355X are in DESIGN.md."""
import numpy as np
import pytest

from tests import cg_cases as C
from tests import lg_cases as LC

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _shift(X, w):
    return np.array([float(np.nansum(x[w].astype(C.LD)) / max(1, np.sum(~np.isnan(x[w])))) for x in X])


def _moments(codes, cards, X, var_disc, n, row0=0, slice_rows=64):
    """(got [Q, mp, mp], want, bound, plan info) of one family over all the given columns."""
    from pgmpy_amd.estimators._cg import CgPlan

    w = slice(row0, row0 + n)
    shift = _shift(X, w)
    plan = CgPlan([(range(len(cards)), cards, range(len(X)), var_disc)])
    plan.set_slice(slice_rows)
    dX = _dev(X) if len(X) else None
    flat = plan.moments(_dev(codes) if len(cards) else None, dX, _dev(shift) if len(X) else None, n, row0)
    got = plan.family_moments(flat, 0).cpu().numpy()
    want, A = C.moments(codes[:, w], cards, X[:, w], shift)
    info = plan.moments_info(n, dX.data_ptr() if len(X) else 0, X.shape[1], row0)
    return got, want, LC.gram_bound(A, n), info


def _assert_moments(got, want, bound):
    err = np.abs(got - want).astype(np.float64)
    print("largest moment error / bound:", float((err / np.maximum(bound, 1e-300)).max()))
    assert (got[:, 0, 0] == want[:, 0, 0].astype(np.float64)).all()  # the counts are exact
    assert (err <= bound).all()


@pytest.mark.parametrize("n", [1, 15, 16, 17, 193])
@pytest.mark.parametrize("q_kind", ["one", "tile", "tile+1", "block+1"])
@pytest.mark.parametrize("m", [0, 1, 3, 4, 7])
def test_moments_every_layout(gpu, m, q_kind, n):
    """Every mp boundary x one configuration, a full tile, the second tile, the second 16-tile block x row counts
    around one step and, with the forced slice of 64, four slices, the last with one row."""
    mp = C.mp_of(m)
    Q = {"one": 1, "tile": 16 // mp, "tile+1": 16 // mp + 1, "block+1": 256 // mp + 1}[q_kind]
    cards = C.cards_for(Q) or ([1] if m == 0 else [])
    codes, X = C.data(1000 * m + 10 * Q + n, n, cards, m)
    got, want, bound, info = _moments(codes, cards, X, m == 0, n)
    assert info[1] == -(-n // 64) and got.shape == (int(np.prod(cards, dtype=int)), mp, mp)
    _assert_moments(got, want, bound)


@pytest.mark.parametrize("row0, ld", [(1, 60), (0, 51)])
def test_moments_unaligned(gpu, row0, ld):
    """An odd first row and an odd leading dimension take the 8-byte loads; cells outside the window are not read."""
    cards = [3, 2]
    codes, X = C.data(7, 50, cards, 3, ld=ld, row0=row0)
    got, want, bound, info = _moments(codes, cards, X, False, 50, row0=row0)
    assert not info[3]
    _assert_moments(got, want, bound)


def test_moments_one_group_is_the_gram(gpu):
    """Q = 1, m = 7: the same moments as GramPlan's of the same columns, both within the Gram bound of the truth."""
    from pgmpy_amd.models._lg import GramPlan

    n = 193
    codes, X = C.data(3, n, [], 7)
    got, want, bound, _ = _moments(codes, [], X, False, n)
    G = GramPlan(range(7)).gram(_dev(X), _dev(_shift(X, slice(0, n)))).cpu().numpy()  # the ones column last
    order = [7] + list(range(7))
    _assert_moments(got, want, bound)
    assert (np.abs(G[np.ix_(order, order)] - got[0]) <= 2 * bound[0]).all()


def _score(codes, cards, X, var_disc, more=()):
    """(ll, n_complete, n_observed, n_dropped) of the family on the device, and the restatement's."""
    from pgmpy_amd.estimators._cg import CgPlan

    n = codes.shape[1] if len(cards) else X.shape[1]
    plan = CgPlan([(range(len(cards)), cards, range(len(X)), var_disc)] + list(more))
    flat = plan.moments(_dev(codes) if len(cards) else None, _dev(X) if len(X) else None,
                        _dev(_shift(X, slice(0, n))) if len(X) else None, n)
    got = [t.cpu().numpy()[0] for t in plan.score(flat)]
    want = C.score(codes, cards, X, var_disc)
    print("score error:", abs(got[0] - float(want[0])), "of", float(want[0]))
    return got, want


def _assert_score(got, want):
    assert abs(got[0] - float(want[0])) <= C.tol(want[0])
    assert tuple(int(x) for x in got[1:]) == tuple(want[1:])


@pytest.mark.parametrize("var_disc", [False, True])
@pytest.mark.parametrize("cards, m", [([], 3), ([3, 4], 0), ([3, 4], 3)], ids=["D empty", "C empty", "both"])
def test_scores(gpu, cards, m, var_disc):
    """A continuous and a discrete variable with no discrete parents, no continuous parents, and both."""
    cards, m = ([5] + cards, m) if var_disc else (cards, m + 1)
    codes, X = C.data(11 + m, 400, cards, m)
    _assert_score(*_score(codes, cards, X, var_disc))


@pytest.mark.parametrize("var_disc", [False, True])
def test_scores_small_groups(gpu, var_disc):
    """Groups of 0, 1, 2, 3, 4 and 40 rows under k = 3 columns (and k = 2 for a continuous variable's
    denominator): both sides of the fallback and n_g = k, where the last column is dropped."""
    sizes = [0, 1, 2, 3, 4, 40]
    codes, X = C.data(5, sum(sizes), [6], 3)
    codes[0] = np.repeat(np.arange(6), sizes)
    cards = [6, 1] if var_disc else [6]
    codes = np.vstack([codes, np.zeros_like(codes)])[:len(cards)]
    got, want = _score(codes, cards, X, var_disc)
    _assert_score(got, want)
    assert want[2] == (1 if var_disc else 5) and want[3] >= 1


def test_scores_constant_parent_dropped(gpu):
    """A continuous parent constant inside one group: its column is dropped there and the score stays finite."""
    codes, X = C.data(9, 300, [3], 3)
    X[0, codes[0] == 1] = 2.5
    got, want = _score(codes, [3], X, False)
    assert np.isfinite(got[0]) and got[3] == 1
    _assert_score(got, want)


def test_scores_skip_incomplete_rows(gpu):
    codes, X = C.data(13, 200, [2, 3], 2)
    codes[1, ::7] = C.MISSING
    X[0, 3::11] = np.nan
    got, want = _score(codes, [2, 3], X, True)
    assert got[1] == want[1] == int(C.complete(codes, X).sum()) < 200
    _assert_score(got, want)


def test_bad_code_raises(gpu):
    codes, X = C.data(2, 40, [3], 1)
    codes[0, 17] = 3
    with pytest.raises(IndexError):
        _score(codes, [3], X, False)


def test_bit_identity(gpu):
    """A family's ll alone, first of 65 and last of 65 families, and on a second call: the same bits."""
    codes, X = C.data(21, 500, [3, 4, 2], 4)
    others = [([d], [k], [j], False) for d, k in enumerate([3, 4, 2]) for j in range(4)] * 6
    fam = ([0, 1, 2], [3, 4, 2], [0, 1, 2, 3], False)
    runs = [_score(codes, [3, 4, 2], X, False)[0][0], _score(codes, [3, 4, 2], X, False, others[:64])[0][0]]
    from pgmpy_amd.estimators._cg import CgPlan

    plan = CgPlan(others[:64] + [fam])
    for _ in range(2):
        flat = plan.moments(_dev(codes), _dev(X), _dev(_shift(X, slice(0, 500))), 500)
        runs.append(plan.score(flat)[0].cpu().numpy()[64])
    assert len({np.float64(r).tobytes() for r in runs}) == 1


def test_python_layer(gpu):
    """BIC / AIC are ll minus the host penalty; from_columns gives the frame form's bits; structure_score and
    get_scoring_method take an instance; HillClimbSearch over 2,000 rows returns the true skeleton."""
    from math import log

    import networkx as nx

    from pgmpy_amd.estimators import AICCondGauss, BICCondGauss, HillClimbSearch, LogLikelihoodCondGauss, get_scoring_method
    from pgmpy_amd.metrics import structure_score

    df, edges = C.mixed_network(2000)
    fams = [("X", ["A"]), ("Z", ["X", "B"]), ("Y", ["B", "X"]), ("A", [])]
    ll, bic, aic = (cls(df).local_scores(fams) for cls in (LogLikelihoodCondGauss, BICCondGauss, AICCondGauss))
    for f, k in enumerate([2 * 2, 3 * 1 * 3, 3 * 3, 1]):
        assert bic[f] == ll[f] - 0.5 * k * log(2000) and aic[f] == ll[f] - k
    codes = np.array([df[v].cat.codes.to_numpy() for v in "ABZ"], dtype=np.uint8)
    want = C.score(codes[[2, 1]], [2, 3], df[["X"]].to_numpy().T, True)
    assert abs(ll[1] - float(want[0])) <= C.tol(want[0])
    scorer = BICCondGauss(df)
    codes_d, X_d, _, _ = scorer.resident()
    resident = BICCondGauss.from_columns(codes_d, scorer.code_variables, scorer.cardinalities, X_d, scorer.value_variables)
    assert resident.local_scores(fams) == bic
    assert get_scoring_method(scorer, df)[0] is scorer
    true = nx.DiGraph(edges)
    true.add_nodes_from(df.columns)
    assert structure_score(true, df, scorer) == sum(scorer.local_scores([(v, list(true.predecessors(v))) for v in true.nodes()]))
    model = HillClimbSearch(df).estimate(scoring_method=scorer)
    assert {frozenset(e) for e in model.edges()} == {frozenset(e) for e in edges}
