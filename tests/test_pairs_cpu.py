"""Pairwise counts and tree learners without a GPU: the long-double restatement against the goldens of the
reference's TreeSearch, the tree logic under the numpy scorer, argument errors, the NaiveBayes structure
rules, and the validation of the pair plan through ctypes (no device call)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

from tests import pair_cases as PC

G = PC.golden()
FRAMES = PC.frames()


@pytest.fixture(scope="module")
def restated():
    """{(frame, kind, conditional): (W, B, left)} under the host bound, computed once."""
    out = {}
    for name, case in G["cases"].items():
        codes, cards = PC.encode(FRAMES[name])
        cols = list(range(len(cards)))
        for kind in PC.KINDS:
            out[(name, kind, False)] = PC.weight_matrix(kind, codes, cols, cards, device=False)
        if "conditional_weights" in case:
            k = case["columns"].index(case["class_node"])
            out[(name, "mutual_info", True)] = PC.weight_matrix("mutual_info", codes, cols, cards, k, cards[k], device=False)
    return out


@pytest.mark.parametrize("name", sorted(G["cases"]))
@pytest.mark.parametrize("kind", PC.KINDS)
def test_restatement_matches_reference_weights(restated, name, kind):
    W, B, left = restated[(name, kind, False)]
    ref = np.array(G["cases"][name]["weights"][kind])
    assert list(FRAMES[name].columns) == G["cases"][name]["columns"]
    PC.check_left_out(left, W.shape[0]) if name in ("net5", "alarm") else None
    ok = ~np.isnan(W)
    assert ok.sum() >= W.size - 2 * len(left)
    assert (np.abs(W - ref)[ok] <= 2 * B[ok]).all(), float(np.nanmax(np.abs(W - ref) - 2 * B))


@pytest.mark.parametrize("name", [n for n, c in sorted(G["cases"].items()) if "conditional_weights" in c])
def test_restatement_matches_reference_conditional_weights(restated, name):
    W, B, left = restated[(name, "mutual_info", True)]
    ref = np.array(G["cases"][name]["conditional_weights"])
    assert not left
    assert (np.abs(W - ref) <= 2 * B).all(), float(np.max(np.abs(W - ref) - 2 * B))


EDGE_CASES = [(n, k, w) for n, c in sorted(G["cases"].items()) for k, e in sorted(c["estimates"].items()) for w in sorted(e)]


@pytest.mark.parametrize("name,kind,what", EDGE_CASES)
def test_tree_logic_reproduces_reference_edges(name, kind, what):
    from pgmpy_amd.estimators.TreeSearch import tree_search

    case = G["cases"][name]
    g = case["estimates"][kind][what]
    assert g["margin"] >= G["min_margin"]
    scorer = PC.HostScorer(FRAMES[name])
    root = None if what == "chow-liu-auto" else case["root"]
    model, picked = tree_search(scorer, case["columns"], root, "tan" if what == "tan" else "chow-liu",
                                case["class_node"] if what == "tan" else None, kind)
    assert sorted(map(list, model.edges())) == g["edges"]
    if what == "chow-liu-auto":
        assert picked == g["root"]
    assert sorted(model.nodes()) == sorted(case["columns"])  # every column is a node (DESIGN.md deviation 11)
    assert set(g["nodes"]) <= set(case["columns"])


def test_constant_column_stays_an_isolated_node():
    from pgmpy_amd.estimators.TreeSearch import tree_search

    case = G["cases"]["const"]
    g = case["estimates"]["mutual_info"]["chow-liu"]
    assert "k" not in g["nodes"]  # the reference builds its graph from the non-zero weights only
    model, _ = tree_search(PC.HostScorer(FRAMES["const"]), case["columns"], case["root"])
    assert "k" in model.nodes() and model.degree("k") == 0


def test_tree_search_argument_errors():
    from pgmpy_amd.estimators import TreeSearch
    from pgmpy_amd.estimators.TreeSearch import tree_search

    df = FRAMES["net5"]
    scorer = PC.HostScorer(df)
    cols = list(df.columns)
    with pytest.raises(ValueError, match="Root node: zz not found in data columns."):
        TreeSearch(df, root_node="zz")
    with pytest.raises(ValueError, match="Invalid estimator_type. Expected either chow-liu or tan. Got: x"):
        tree_search(scorer, cols, "v0", "x")
    with pytest.raises(ValueError, match="class_node argument must be specified for estimator_type='tan'"):
        tree_search(scorer, cols, "v0", "tan")
    with pytest.raises(ValueError, match="Class node: zz not found in data columns"):
        tree_search(scorer, cols, "v0", "tan", "zz")
    with pytest.raises(ValueError, match="Root node: v0 and class node: v0 are identical"):
        tree_search(scorer, cols, "v0", "tan", "v0")
    with pytest.raises(ValueError, match="edge_weights_fn should either be"):
        tree_search(scorer, cols, "v0", "chow-liu", None, "entropy")
    with pytest.raises(ValueError, match="edge_weights_fn should either be"):
        TreeSearch._get_weights(df, "entropy")
    est = TreeSearch(df, root_node="v1", n_jobs=3)
    assert est.root_node == "v1" and est.n_jobs == 3


def test_callable_weights_run_on_the_host():
    """A callable goes pair by pair over the frame's columns, no device: the slow path."""
    from sklearn.metrics import mutual_info_score

    from pgmpy_amd.estimators import TreeSearch

    df = FRAMES["net5"]
    case = G["cases"]["net5"]
    calls = []

    def fn(x, y):
        calls.append((x.name, y.name))
        return mutual_info_score(x, y)

    w = TreeSearch._get_weights(df, fn)
    assert len(calls) == 10 and calls[0] == ("v0", "v1")
    np.testing.assert_allclose(w, np.array(case["weights"]["mutual_info"]), rtol=0, atol=1e-12)
    cw = TreeSearch._get_conditional_weights(df, "v4", fn)
    np.testing.assert_allclose(cw, np.array(case["conditional_weights"]), rtol=0, atol=1e-12)
    model = TreeSearch(df, root_node="v0").estimate("chow-liu", edge_weights_fn=fn)
    assert sorted(map(list, model.edges())) == case["estimates"]["mutual_info"]["chow-liu"]["edges"]
    tan = TreeSearch(df, root_node="v0").estimate("tan", class_node="v4", edge_weights_fn=fn)
    assert sorted(map(list, tan.edges())) == case["estimates"]["mutual_info"]["tan"]["edges"]


def test_pair_weights_special_cases():
    """scikit-learn's special cases on hand-made statistics (pgmpy_amd.estimators._pairs.pair_weights)."""
    from pgmpy_amd.estimators._pairs import pair_weights, stratified_weight

    mi = np.array([0.2, 1e-17, 0.3, 0.0, 0.1])
    hu = np.array([0.6, 0.0, 0.0, 0.5, 0.4])
    hv = np.array([0.7, 0.0, 0.4, 0.6, 0.4])
    n = np.array([10, 10, 10, 10, 0])
    emi = np.array([0.05, 0.0, 0.0, 0.01, 0.0])
    np.testing.assert_array_equal(pair_weights("mutual_info", mi, hu, hv, n), [0.2, 0.0, 0.0, 0.0, 0.0])
    np.testing.assert_allclose(pair_weights("normalized_mutual_info", mi, hu, hv, n), [0.2 / 0.65, 1.0, 0.0, 0.0, 0.0])
    np.testing.assert_allclose(pair_weights("adjusted_mutual_info", mi, hu, hv, n, emi),
                               [0.15 / 0.6, 1.0, 0.0, -0.01 / 0.54, 0.0])
    w = np.array([[0.5, 0.1], [0.25, 0.3]])
    nn = np.array([[30, 0], [10, 0]])
    np.testing.assert_allclose(stratified_weight(w, nn), [0.75 * 0.5 + 0.25 * 0.25, 0.0])


# ---------------------------------------------------------------------- NaiveBayes
def test_naive_bayes_structure_rules():
    from pgmpy_amd.models import DiscreteBayesianNetwork, NaiveBayes

    m = NaiveBayes(feature_vars=["b", "c"], dependent_var="a")
    assert isinstance(m, DiscreteBayesianNetwork)
    assert sorted(m.edges()) == [("a", "b"), ("a", "c")] and m.dependent == "a" and m.features == {"b", "c"}
    with pytest.raises(ValueError, match="Model can only have edges outgoing from: a"):
        m.add_edge("b", "c")
    with pytest.raises(ValueError, match="Model can only have edges outgoing from: a"):
        m.add_edges_from([("a", "d"), ("d", "e")])
    assert ("a", "d") in m.edges() and m.features == {"b", "c", "d"}
    e = NaiveBayes()
    e.add_nodes_from(["x", "y"])
    e.add_edge("x", "y")
    assert e.dependent == "x" and e.features == {"y"}
    assert m.active_trail_nodes("a") == {"a", "b", "c", "d"}
    assert m.active_trail_nodes("a", ["b", "c"]) == {"a", "d"}
    assert m.active_trail_nodes("b", ["a"]) == {"b"}
    ind = m.local_independencies("b")
    (a,) = ind.get_assertions()
    assert a.event1 == {"b"} and a.event2 == {"c", "d"} and a.event3 == {"a"}
    assert m.local_independencies("a").get_assertions() == []
    assert m._get_ancestors_of([]) == set() and m._get_ancestors_of(["b"]) == {"a", "b"}


def test_naive_bayes_fit_errors():
    from pgmpy_amd.models import NaiveBayes

    df = pd.DataFrame({"A": [0, 1], "B": [1, 0]})
    with pytest.raises(ValueError, match="parent node must be specified for the model"):
        NaiveBayes().fit(df)
    with pytest.raises(ValueError, match="Dependent variable: Z is not present in the data"):
        NaiveBayes().fit(df, "Z")


# ---------------------------------------------------------------------- the host plan unit, stand-alone
def test_pair_plan_selftest(tmp_path):
    """tools/pair_plan_selftest.cpp drives pgmpair_plan.cpp alone (state table, tile list, slice choice)."""
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "pgmpy_amd", "csrc")
    exe = str(tmp_path / "pair_plan_selftest")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-I", os.path.join(root, "include"), "-I", csrc,
                            os.path.join(root, "tools", "pair_plan_selftest.cpp"),
                            os.path.join(csrc, "pgmpair_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "pair_plan_selftest ok" in run.stdout, run.stdout + run.stderr


# ---------------------------------------------------------------------- the plan, through ctypes
def test_pair_plan_layout_and_lists():
    from pgmpy_amd.estimators._pairs import PairPlan

    p = PairPlan([4, 0, 2], [2, 3, 4])
    assert (p.S, p.Sp, p.offsets, p.n_pairs) == (9, 16, [0, 2, 5, 9], 3)
    assert p.tile_pairs() == [(0, 0)] and p.groups() == [(0, 0, 2)]
    assert int(p.info.n_cols) == 5 and int(p.info.table_size) == 256 and int(p.info.n_state_entries) == 64
    assert [p.pair_index(0, 1), p.pair_index(0, 2), p.pair_index(1, 2)] == [0, 1, 2]
    # a 254-state variable beside a binary one: only the tiles of the binary column's state pair up
    q = PairPlan([0, 1], [254, 2])
    assert (q.S, q.Sp) == (256, 256) and q.tile_pairs() == [(t, 15) for t in range(16)]
    assert q.groups() == [(0, 3, 3), (1, 3, 1), (2, 3, 1), (3, 3, 0)]
    # every super-tile that is in a group checks its codes exactly once
    for plan in (p, q, PairPlan(list(range(37)), [3] * 37), PairPlan(list(range(40)), [7] * 40)):
        seen = []
        for I, J, check in plan.groups():
            seen += [I] * (check & 1) + [J] * (check >> 1 & 1)
        assert sorted(seen) == sorted({t for I, J, _ in plan.groups() for t in (I, J)})
    # a single variable has no pair: nothing to launch
    one = PairPlan([3], [5])
    assert one.n_pairs == 0 and one.groups() == [] and one.tile_pairs() == []
    # S = 16, 17, 33; a variable straddling a tile boundary; a card-1 variable
    for cards, sp in (([8, 8], 16), ([8, 8, 1], 32), ([15, 3, 15], 48), ([1, 1], 16)):
        r = PairPlan(list(range(len(cards))), cards)
        assert r.S == sum(cards) and r.Sp == sp
    straddle = PairPlan([0, 1, 2], [15, 3, 15])
    assert straddle.tile_pairs() == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2)]  # tile 2 holds one variable only


def test_pair_plan_validation():
    from pgmpy_amd.estimators._pairs import PairPlan

    with pytest.raises(ValueError, match=r"variable 1 cardinality 0 \(1 .. 254\)"):
        PairPlan([0, 1], [2, 0])
    with pytest.raises(ValueError, match=r"variable 0 cardinality 255 \(1 .. 254\)"):
        PairPlan([0, 1], [255, 2])
    with pytest.raises(ValueError, match="column 3 is listed twice"):
        PairPlan([3, 1, 3], [2, 2, 2])
    with pytest.raises(ValueError, match="variable 1 column -2"):
        PairPlan([0, -2], [2, 2])
    with pytest.raises(ValueError, match="0 variables"):
        PairPlan([], [])
    with pytest.raises(ValueError, match="2 columns, 1 cardinalities"):
        PairPlan([0, 1], [2])


def test_pair_count_argument_checks_before_any_device_call():
    from pgmpy_amd import _native as N
    from pgmpy_amd.estimators._pairs import PairPlan

    L = N.load_library()
    p = PairPlan([0, 1, 2], [2, 3, 4])
    P = ctypes.c_void_p

    def count(codes=64, n_cols=3, ld=100, row0=0, n_rows=100, strat=-1, n_strata=1, counts=64):
        return L.pgm_pair_count(p._h, P(codes), n_cols, ld, row0, n_rows, strat, n_strata, P(counts), None)

    for kwargs, text in ((dict(strat=3), "stratum column 3, codes has 3 columns"),
                         (dict(strat=-2), "stratum column -2"),
                         (dict(n_strata=2), "2 strata"),
                         (dict(strat=1, n_strata=0), "0 strata"),
                         (dict(strat=1, n_strata=255), "255 strata"),
                         (dict(n_cols=2), "the plan reads column 2, codes has 2 columns"),
                         (dict(row0=1), r"rows \[1, 101\) outside ld 100"),
                         (dict(n_rows=-1), "n_rows -1"),
                         (dict(codes=None), "null codes / counts"),
                         (dict(counts=None), "null codes / counts")):
        assert count(**kwargs) == N.PGM_EINVAL
        with pytest.raises(ValueError, match=text):
            N.check(N.PGM_EINVAL, "pair_count")
    assert count(n_rows=0) == N.PGM_OK  # nothing to count: no device call
    assert L.pgm_pair_mi(p._h, None, 1, None, None, None, None, None) == N.PGM_EINVAL
    assert L.pgm_pair_emi(p._h, P(64), 0, P(64), None) == N.PGM_EINVAL
    assert L.pgm_pair_plan_destroy(None) == N.PGM_OK


def test_pair_slice_choice_and_budget():
    from pgmpy_amd.estimators._pairs import PairPlan

    p = PairPlan(list(range(37)), [3] * 37)
    for n_rows in (1, 255, 256, 257, 70_000, 1_000_000, 3_000_000_000):
        rows, slices, vec = p.count_info(n_rows)
        assert rows % 256 == 0 and 256 <= rows <= 1 << 30 and (slices - 1) * rows < n_rows <= slices * rows
        assert slices <= 65535
    assert p.count_info(70_000)[1] > 1  # several row slices
    p.set_slice(1000)
    assert p.count_info(70_000)[:2] == (1024, 69)
    p.set_slice(0)
    assert p.count_info(70_000)[0] == 256
    with pytest.raises(ValueError, match="pair_plan_set_slice"):
        p.set_slice(-1)
    assert p.count_info(64, codes_ptr=4096, ld=1024, row0=16)[2] is True
    assert p.count_info(64, codes_ptr=4096, ld=1003, row0=0)[2] is False
    assert p.count_info(64, codes_ptr=4096, ld=1024, row0=3)[2] is False
    # the budget on n_strata * Sp^2 * 8 bytes names the size
    small = PairPlan(list(range(37)), [3] * 37, budget=1 << 16)
    assert small.count_bytes(3) == 3 * 112 * 112 * 8
    with pytest.raises(ValueError, match=r"3 strata x 112 x 112 int64 take 301056 bytes, above the budget of 65536"):
        small._check_budget(3)
