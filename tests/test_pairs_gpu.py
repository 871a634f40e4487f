"""Pairwise counts and tree learners on the device: k_pair_count against exact np.bincount tables (integer
equality), k_pair_mi / k_pair_emi against the long-double restatement under the bounds of
tests/pair_cases.py, and the public API (TreeSearch, NaiveBayes, pairwise_counts) against the goldens of the
reference."""
import functools

import numpy as np
import pandas as pd
import pytest

from tests import pair_cases as PC

pytestmark = pytest.mark.gpu

G = PC.golden()
FRAMES = PC.frames()
GUARD = 0x5A5A5A5A5A5A5A5A


def _dev(a):
    from pgmpy_amd import engine as E

    return E.to_device_raw(np.ascontiguousarray(a))


def _host(t):
    from pgmpy_amd.inference.batch import download

    return download(t.contiguous())


def _plan(cols, cards):
    from pgmpy_amd.estimators._pairs import PairPlan

    return PairPlan(cols, cards)


def _assert_blocks(plan, counts, codes, cols, cards, stratum=None, n_strata=1):
    got = PC.blocks_of(_host(counts), cards, plan.Sp)
    want = PC.tables(codes, cols, cards, stratum, n_strata)
    assert got.keys() == want.keys()
    for key in want:
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])


def _count_and_check(codes, cols, cards, stratum=None, n_strata=1):
    plan = _plan(cols, cards)
    counts = plan.count(_dev(codes), stratum=stratum, n_strata=n_strata)
    _assert_blocks(plan, counts, codes, cols, cards, stratum, n_strata)
    return plan, counts


# ---------------------------------------------------------------------- k_pair_count
@pytest.mark.parametrize("n_rows", [1, 15, 16, 17, 63, 64, 65, 1000])
def test_count_asymmetric_tables_every_row_count(gpu, n_rows):
    """Cards (2, 3, 4) with dependent columns: every block is an asymmetric table, so a wrong row / column
    map of the MFMA operands or of its result would show."""
    cards = [2, 3, 4]
    codes = PC.dependent_codes(n_rows, cards, seed=n_rows)
    if n_rows == 1000:
        t = PC.table(codes, [0, 1, 2], cards, 1, 2)
        assert not np.array_equal(t[:3, :3], t[:3, :3].T)
    _count_and_check(codes, [0, 1, 2], cards)


@pytest.mark.parametrize("cards", [[8, 8], [8, 8, 1], [15, 3, 15], [1, 5, 1, 9], [254, 2], [2, 254, 3], [60, 7, 60, 5, 70]],
                         ids=lambda c: "-".join(map(str, c)))
def test_count_layouts_across_tile_edges(gpu, cards):
    """S = 16, 17, 33; a variable straddling a tile boundary; card-1 variables; a 254-state variable beside a
    binary one; more than one super-tile."""
    codes = PC.dependent_codes(777, cards, seed=len(cards))
    cols = list(range(len(cards)))[::-1]  # the variables in another order than the columns
    _count_and_check(codes, cols, cards[::-1])


def test_count_missing_cells(gpu):
    cards = [2, 3, 4, 3]
    cols = [0, 1, 2, 3]
    base = PC.dependent_codes(500, cards, seed=5)
    for c in cols:  # each column in turn
        codes = base.copy()
        codes[c, ::3] = PC.MISSING
        _count_and_check(codes, cols, cards)
    codes = PC.dependent_codes(500, cards, seed=6, missing=0.2)
    _count_and_check(codes, cols, cards)
    codes[2, :] = PC.MISSING  # one column all missing
    _count_and_check(codes, cols, cards)
    codes[:, :] = PC.MISSING  # all rows missing
    plan, counts = _count_and_check(codes, cols, cards)
    assert int(_host(counts).sum()) == 0


@pytest.mark.parametrize("col,row", [(0, 0), (1, 499), (2, 250), (3, 17)])
def test_bad_code_is_an_index_error_and_counted_nowhere(gpu, col, row):
    import torch

    cards = [2, 3, 4, 70]
    cols = [0, 1, 2, 3]
    codes = PC.dependent_codes(500, cards, seed=9)
    codes[col, row] = cards[col]  # neither a state nor 255
    plan = _plan(cols, cards)
    n = plan.Sp * plan.Sp
    buf = torch.full((n + 32,), GUARD, dtype=torch.int64, device="cuda")
    counts = buf[16:16 + n]
    counts.zero_()
    with pytest.raises(IndexError, match="pair_count: a state code is >= its variable's cardinality"):
        plan.count(_dev(codes), counts=counts)
    as_missing = codes.copy()
    as_missing[col, row] = PC.MISSING
    _assert_blocks(plan, counts, as_missing, cols, cards)
    host = _host(buf)
    assert (host[:16] == GUARD).all() and (host[16 + n:] == GUARD).all()  # nothing written outside counts
    counts.zero_()
    plan.count(_dev(as_missing), counts=counts)  # the flag is reset by the next call
    _assert_blocks(plan, counts, as_missing, cols, cards)


def test_count_unaligned_window_equals_the_aligned_path(gpu):
    """row0 = 3 and ld = 1,003: no 16-byte load is aligned, the guarded byte path runs."""
    import torch

    cards = [2, 3, 4, 20]
    cols = [0, 1, 2, 3]
    codes = PC.dependent_codes(1000, cards, seed=11, missing=0.05)
    plan = _plan(cols, cards)
    aligned = plan.count(_dev(codes))
    wide = np.full((4, 1003), 7, dtype=np.uint8)  # 7 is no state of columns 0..2: reading outside the window would flag
    wide[:, 3:] = codes
    d_wide = _dev(wide)
    assert plan.count_info(1000, codes_ptr=d_wide.data_ptr(), ld=1003, row0=3)[2] is False
    narrow = plan.count(d_wide, row0=3, n_rows=1000)
    assert torch.equal(aligned, narrow)
    _assert_blocks(plan, narrow, codes, cols, cards)
    # an aligned base with a window that ends inside a 16-row group, and one that starts at row 16
    part = plan.count(_dev(codes), row0=16, n_rows=333)
    _assert_blocks(plan, part, codes[:, 16:349], cols, cards)


def test_count_stratified(gpu):
    cards = [2, 3, 4, 3]
    codes = PC.dependent_codes(1000, cards, seed=13, missing=0.03)
    codes[3, ::7] = PC.MISSING  # a card-3 class with some 255s
    _count_and_check(codes, [0, 1, 2], cards[:3], stratum=3, n_strata=3)  # the class beside the variables
    _count_and_check(codes, [0, 1, 2, 3], cards, stratum=3, n_strata=3)  # the class among the variables
    _count_and_check(codes, [0, 1, 2], cards[:3], stratum=3, n_strata=1)  # one stratum: class state 0 only
    _count_and_check(codes, [0, 1, 2], cards[:3], stratum=3, n_strata=2)


def test_count_row_windows_add_up_and_slices_do_not_matter(gpu):
    import torch

    cards = [2, 3, 4, 5]
    cols = [0, 1, 2, 3]
    codes = PC.dependent_codes(5000, cards, seed=17, missing=0.02)
    d = _dev(codes)
    plan = _plan(cols, cards)
    whole = plan.count(d)
    parts = plan.count(d, row0=0, n_rows=1237)
    plan.count(d, row0=1237, n_rows=5000 - 1237, counts=parts)
    assert torch.equal(whole, parts)
    for rows in (256, 1000, 4096):  # a forced slice length: another launch, the same integers
        plan.set_slice(rows)
        assert plan.count_info(5000)[0] == -(-rows // 256) * 256
        assert torch.equal(whole, plan.count(d))
    _assert_blocks(plan, whole, codes, cols, cards)


@functools.lru_cache(maxsize=None)
def _alarm_sample(n):
    from pgmpy_amd.sampling import BayesianModelSampling
    from pgmpy_amd.utils import get_example_model

    model = get_example_model("alarm")
    d_codes, nodes = BayesianModelSampling(model).forward_sample_codes(n, seed=2)
    cards = [len(model.states[v]) for v in nodes]
    return model, d_codes, nodes, cards


def test_count_alarm_70000_rows_sampled_on_the_device(gpu):
    model, d_codes, nodes, cards = _alarm_sample(70_000)
    cols = list(range(len(nodes)))
    plan = _plan(cols, cards)
    assert plan.n_pairs == 666 and plan.count_info(70_000)[1] > 1  # several row slices
    counts = plan.count(d_codes)
    _assert_blocks(plan, counts, _host(d_codes), cols, cards)


# ---------------------------------------------------------------------- k_pair_mi / k_pair_emi
def _assert_stats(plan, counts, codes, cols, cards, stratum=None, n_strata=1):
    mi, hu, hv, n = (_host(t) for t in plan.mi(counts))
    emi = _host(plan.emi(counts))
    for (c, u, v), t in PC.tables(codes, cols, cards, stratum, n_strata).items():
        st = PC.pair_stats(t, want_emi=True)
        p = plan.pair_index(u, v)
        assert n[c, p] == st["N"]
        for key, got in (("mi", mi), ("hu", hu), ("hv", hv)):
            print(key, (c, u, v), got[c, p], float(st[key][0]), PC.bound(st[key]))
            assert abs(got[c, p] - float(st[key][0])) <= PC.bound(st[key]), (key, c, u, v)
        print("emi", (c, u, v), emi[c, p], float(st["emi"][0]), PC.emi_bound(st["emi"]))
        assert abs(emi[c, p] - float(st["emi"][0])) <= PC.emi_bound(st["emi"]), ("emi", c, u, v)
    return mi, hu, hv, n, emi


def test_statistics_against_the_restatement(gpu):
    cards = [2, 3, 4, 3]
    codes = PC.dependent_codes(1000, cards, seed=19, missing=0.03)
    plan, counts = _count_and_check(codes, [0, 1, 2, 3], cards)
    _assert_stats(plan, counts, codes, [0, 1, 2, 3], cards)
    plan, counts = _count_and_check(codes, [0, 1, 2, 3], cards, stratum=3, n_strata=3)
    _assert_stats(plan, counts, codes, [0, 1, 2, 3], cards, stratum=3, n_strata=3)
    cards = [254, 2, 60]
    codes = PC.dependent_codes(4000, cards, seed=21)
    plan, counts = _count_and_check(codes, [0, 1, 2], cards)
    _assert_stats(plan, counts, codes, [0, 1, 2], cards)


def test_statistics_of_empty_and_one_hot_blocks(gpu):
    cards = [3, 4, 2]
    codes = np.zeros((3, 300), dtype=np.uint8)
    codes[0, :] = 2  # (0, 1): every row in the cell (2, 3): a one-hot block
    codes[1, :] = 3
    codes[2, :] = PC.MISSING  # (0, 2), (1, 2): no complete row, N = 0
    plan, counts = _count_and_check(codes, [0, 1, 2], cards)
    mi, hu, hv, n, emi = _assert_stats(plan, counts, codes, [0, 1, 2], cards)
    assert n[0].tolist() == [300, 0, 0]
    assert mi[0].tolist() == [0.0, 0.0, 0.0] and hu[0].tolist() == [0.0] * 3 and hv[0].tolist() == [0.0] * 3
    assert emi[0, 1] == 0.0 and emi[0, 2] == 0.0


def test_a_pair_alone_has_the_bits_it_has_among_666(gpu):
    model, d_codes, nodes, cards = _alarm_sample(70_000)
    plan = _plan(list(range(37)), cards)
    counts = plan.count(d_codes)
    full = [_host(t) for t in (*plan.mi(counts), plan.emi(counts))]
    for u, v in ((0, 1), (5, 30), (35, 36)):
        alone = _plan([u, v], [cards[u], cards[v]])
        c2 = alone.count(d_codes)
        got = [_host(t) for t in (*alone.mi(c2), alone.emi(c2))]
        p = plan.pair_index(u, v)
        for a, b in zip(got, full):
            assert a[0, 0].tobytes() == b[0, p].tobytes(), (u, v)


# ---------------------------------------------------------------------- the public API
@functools.lru_cache(maxsize=None)
def _restated(name, kind, conditional):
    case = G["cases"][name]
    codes, cards = PC.encode(FRAMES[name])
    k = case["columns"].index(case["class_node"]) if conditional else None
    args = (kind, codes, list(range(len(cards))), cards, k, cards[k] if conditional else 1)
    return PC.weight_matrix(*args), PC.weight_matrix(*args, device=False)


def _assert_weights(got, name, kind, conditional, ref):
    """The device's matrix against the restatement under the device bound (+ the rounding of the restated
    value to fp64), and against the reference's own numbers under the sum of both bounds."""
    (W, B, left), (_, Bh, left_h) = _restated(name, kind, conditional)
    if name in ("net5", "alarm"):
        PC.check_left_out(left, W.shape[0])
    ok = ~np.isnan(W)
    print(name, kind, "max |device - restatement|", float(np.abs(got - W)[ok].max(initial=0)), "max bound",
          float(B[ok].max(initial=0)))
    assert (np.abs(got - W)[ok] <= B[ok] + PC.U * np.abs(W[ok])).all()
    ok &= ~np.isnan(Bh)
    assert (np.abs(got - np.array(ref))[ok] <= B[ok] + 2 * Bh[ok]).all()
    assert np.array_equal(got, got.T) and (np.diag(got) == 0).all()


@pytest.mark.parametrize("name", sorted(G["cases"]))
@pytest.mark.parametrize("kind", PC.KINDS)
def test_device_weights_match_the_goldens(gpu, name, kind):
    from pgmpy_amd.estimators import TreeSearch

    case = G["cases"][name]
    _assert_weights(TreeSearch._get_weights(FRAMES[name], kind), name, kind, False, case["weights"][kind])
    if kind == "mutual_info" and "conditional_weights" in case:
        got = TreeSearch._get_conditional_weights(FRAMES[name], case["class_node"], kind)
        _assert_weights(got, name, kind, True, case["conditional_weights"])


@pytest.mark.parametrize("name,kind", [(n, k) for n, c in sorted(G["cases"].items()) for k in sorted(c["estimates"])])
def test_device_edge_sets_match_the_goldens(gpu, name, kind):
    from pgmpy_amd.estimators import TreeSearch
    from pgmpy_amd.models import DiscreteBayesianNetwork

    case = G["cases"][name]
    df = FRAMES[name]
    est = case["estimates"][kind]
    given = TreeSearch(df, root_node=case["root"]).estimate("chow-liu", edge_weights_fn=kind, show_progress=False)
    assert isinstance(given, DiscreteBayesianNetwork) and not given.get_cpds()
    assert sorted(map(list, given.edges())) == est["chow-liu"]["edges"]
    assert sorted(given.nodes()) == sorted(case["columns"])
    search = TreeSearch(df)
    auto = search.estimate("chow-liu", edge_weights_fn=kind)
    assert search.root_node == est["chow-liu-auto"]["root"]
    assert sorted(map(list, auto.edges())) == est["chow-liu-auto"]["edges"]
    tan = TreeSearch(df, root_node=case["root"], n_jobs=2).estimate("tan", class_node=case["class_node"],
                                                                    edge_weights_fn=kind)
    assert sorted(map(list, tan.edges())) == est["tan"]["edges"]


def test_pairwise_counts_equal_state_counts(gpu):
    from pgmpy_amd.estimators import BaseEstimator

    df = FRAMES["net5"].iloc[:300].astype(object)
    df.iloc[::9, 1] = np.nan
    df.iloc[::11, 4] = np.nan
    est = BaseEstimator(df)
    pairs = est.pairwise_counts()
    assert list(pairs) == [(u, v) for i, u in enumerate(df.columns) for v in df.columns[i + 1:]]
    for (u, v), t in pairs.items():
        want = est.state_counts(u, [v])
        assert np.array_equal(t.to_numpy(), want.to_numpy()) and list(t.index) == list(want.index)
        assert list(t.columns) == [c[0] if isinstance(c, tuple) else c for c in want.columns]
    given = est.pairwise_counts(["v0", "v1", "v2"], given="v4")
    for (u, v), t in given.items():
        want = est.state_counts(u, [v, "v4"])
        assert np.array_equal(t.to_numpy(), want.to_numpy()) and list(t.columns) == list(want.columns)
    with pytest.raises(KeyError):
        est.pairwise_counts(["v0", "zz"])


def test_naive_bayes_fit_predict_equals_the_same_network(gpu):
    from pgmpy_amd.models import DiscreteBayesianNetwork, NaiveBayes

    df = FRAMES["net5"]
    nb = NaiveBayes()
    nb.fit(df.iloc[:800], "v4")
    assert sorted(nb.edges()) == [("v4", f"v{j}") for j in range(4)] and nb.dependent == "v4"
    plain = DiscreteBayesianNetwork([("v4", f"v{j}") for j in range(4)])
    plain.fit(df.iloc[:800])
    for node in df.columns:
        assert np.array_equal(np.asarray(nb.get_cpds(node).get_values()), np.asarray(plain.get_cpds(node).get_values()))
    rows = df.iloc[800:].drop(columns=["v4"])
    assert nb.predict(rows).equals(plain.predict(rows))
    again = NaiveBayes(feature_vars=["v0", "v1"], dependent_var="v4")
    again.fit(df.iloc[:800])  # the dependent variable known from the constructor; the other columns join
    assert again.features == {"v0", "v1", "v2", "v3"}


def test_simulate_tan_fit_predict_probability(gpu):
    from pgmpy_amd.estimators import TreeSearch
    from pgmpy_amd.utils import get_example_model

    alarm = get_example_model("alarm")
    df = alarm.simulate(n_samples=3000, seed=4, show_progress=False)
    model = TreeSearch(df, root_node="HR").estimate("tan", class_node="CATECHOL", show_progress=False)
    assert set(model.nodes()) == set(alarm.nodes()) and model.number_of_edges() == 36 + 35
    assert all(model.has_edge("CATECHOL", v) for v in alarm.nodes() if v != "CATECHOL")
    model.fit(df)
    prob = model.predict_probability(df.drop(columns=["CATECHOL", "HR"]).head(64))
    for v in ("CATECHOL", "HR"):
        cols = [c for c in prob.columns if c.startswith(v + "_")]
        np.testing.assert_allclose(prob[cols].to_numpy(dtype=float).sum(axis=1), 1.0, rtol=0, atol=1e-9)
