"""CI tests and PC without a GPU: the ABI of pgm_fit_citest, the numpy restatement against the reference's
goldens, Q(a, x) and the host argument checks in a sanitized stand-alone program (tools/ci_selftest.cpp),
the PC loop, collider orientation and Meek's rules under a host tester, PDAG against the reference's
fixtures, and the API's errors."""
import ctypes
import os
import re
import shutil
import subprocess

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import ci_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = C.load_golden()
ALPHA = GOLDEN["s"]["alpha"]


# ---------------------------------------------------------------------------- ABI
def test_citest_symbol_is_bound_and_the_abi_version_stays():
    from pgmpy_amd import _native as N

    assert "pgm_fit_citest" in N.EXPORTED
    lib = N.load_library()
    assert lib.pgm_fit_citest.restype is ctypes.c_int and len(lib.pgm_fit_citest.argtypes) == 8
    assert lib.pgm_fit_citest.argtypes[2] is ctypes.c_double
    assert lib.pgm_version() == 25
    with open(os.path.join(ROOT, "include", "pgmhip.h")) as f:
        header = f.read()
    assert int(re.search(r"#define PGM_CI_CHUNK (\d+)", header).group(1)) == N.CI_CHUNK == C.CHUNK
    assert int(re.search(r"#define PGM_CI_YATES (\d+)", header).group(1)) == N.CI_YATES == C.YATES
    with open(os.path.join(ROOT, "pgmpy_amd", "csrc", "pgm_fit.h")) as f:
        assert int(re.search(r"kCiSmall = (\d+)", f.read()).group(1)) == C.SMALL


def test_fit_citest_rejects_bad_arguments_on_the_host():
    """pgm_fit_citest validates every argument before any HIP call: PGM_EINVAL, a message, no device."""
    from pgmpy_amd import _native as N
    from pgmpy_amd.estimators._fit import FitPlan

    lib = N.load_library()
    plan = FitPlan([([0, 1], [3, 2]), ([2, 0, 1], [2, 3, 2])])
    lone = FitPlan([([0, 1], [3, 2]), ([2], [2])])
    counts, stat, dof, p = np.zeros(18, dtype=np.int64), np.full(2, 7.0), np.full(2, 7, dtype=np.int64), np.full(2, 7.0)
    pc, ps, pd_, pp = (a.ctypes.data_as(ctypes.c_void_p) for a in (counts, stat, dof, p))
    for args, message in (
            ((None, pc, 1.0, 1, ps, pd_, pp, None), "null plan"),
            ((plan._h, None, 1.0, 1, ps, pd_, pp, None), "null counts"),
            ((plan._h, pc, 1.0, 1, None, pd_, pp, None), "null stat"),
            ((plan._h, pc, 1.0, 1, ps, None, pp, None), "null dof"),
            ((plan._h, pc, 1.0, 1, ps, pd_, None, None), "null pvalue"),
            ((plan._h, pc, float("nan"), 1, ps, pd_, pp, None), "not finite"),
            ((plan._h, pc, float("inf"), 0, ps, pd_, pp, None), "not finite"),
            ((plan._h, pc, 1.0, 2, ps, pd_, pp, None), "flags 2"),
            ((lone._h, pc, 1.0, 1, ps, pd_, pp, None), "family 1 has fewer than two variables")):
        assert lib.pgm_fit_citest(*args) == N.PGM_EINVAL, message
        assert message in N.last_error()
    assert (stat == 7.0).all() and (dof == 7).all() and (p == 7.0).all()


# ---------------------------------------------------------------------------- the sanitized host program
def test_ci_selftest_sanitized_and_the_measured_q_error(tmp_path):
    """pgm_igamc (the function the kernel calls) against the recorded chi2.sf grid, the CI work lists and
    fit_citest_check, under ASan + UBSan.  The largest relative error over p >= 1e-300 must stay within
    10 x the recorded measurement and under 1e-9."""
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe, grid = str(tmp_path / "ci_selftest"), str(tmp_path / "grid.txt")
    with open(grid, "w") as f:
        for k, x, sf in GOLDEN["sf_grid"]:
            f.write(f"{float(k).hex()} {float(x).hex()} {float(sf).hex()}\n")
    csrc = os.path.join(ROOT, "pgmpy_amd", "csrc")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tools", "ci_selftest.cpp"),
                            os.path.join(csrc, "pgmfit_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe, grid], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "ci_selftest ok" in run.stdout, run.stdout + run.stderr
    worst = float(re.search(r"max_rel_err (\S+)", run.stdout).group(1))
    print(run.stdout)
    assert C.Q_REL <= 1e-9 and worst <= C.Q_REL
    ks = {k for k, _, _ in GOLDEN["sf_grid"]}
    assert ks == {1, 2, 3, 10, 100, 1000, 5000} and min(sf for _, _, sf in GOLDEN["sf_grid"] if sf >= 1e-300) < 1e-298


def test_a_statistic_rounded_below_zero_counts_as_zero():
    """scipy's chi2.sf gives 1 for a negative argument; so do the restatement and (ci_selftest) pgm_igamc."""
    assert float(C.chi2_sf(-4.4e-16, 4)) == 1.0 and float(C.chi2_sf(0.0, 4)) == 1.0
    assert np.isnan(float(C.chi2_sf(float("nan"), 4)))


def test_long_double_q_reproduces_the_grid():
    """The restatement's own Q against scipy's, on every tenth point (lgammal through ctypes is rounded to
    fp64: half an ulp of lgamma(a) in the exponent, so 2^-53 * lgamma(a) relative)."""
    import math

    for k, x, sf in GOLDEN["sf_grid"][::10]:
        if sf >= 1e-300:
            tol = 1e-13 + 2.0 ** -52 * abs(math.lgamma(k / 2)) + 2.0 ** -52 * (x / 2 + (k / 2) * abs(math.log(x / 2)))
            assert abs(float(C.chi2_sf(x, k)) - sf) <= tol * sf, (k, x)


# ---------------------------------------------------------------------------- restatement == reference
def _check_tests(df, tests, state_names=None):
    """Every recorded (chi, p, dof) of the reference under the six lambdas."""
    tester = C.HostTester(df, state_names=state_names)
    checked = 0
    for name, lam in C.LAMBDAS.items():
        got = tester.tests([(t["X"], t["Y"], t["Z"]) for t in tests], lam)
        for t, (stat, dof, p, mag, cells) in zip(tests, got):
            chi, p_ref, dof_ref = t["results"][name]
            key = (t["X"], t["Y"], t["Z"], name)
            assert dof == dof_ref, key
            b = C.bound(cells, mag)
            assert C.same(stat, chi, b), (key, float(stat), chi, b)
            # a conditional test of the reference is 1 - cdf: it floors at 0 and carries an absolute 2^-53
            assert C.same(p, p_ref, C.p_bound(stat, dof, p, b) + (1e-15 if t["Z"] else 0.0)), (key, float(p), p_ref)
            checked += 1
    return checked


def test_restatement_reproduces_golden_tests_of_s():
    checked = _check_tests(C.frame_of(GOLDEN["s"]), GOLDEN["s"]["tests"])
    assert checked == 6 * 21 * 16


@pytest.mark.parametrize("key", sorted(GOLDEN["edge"]))
def test_restatement_reproduces_golden_edge_frames(key):
    case = GOLDEN["edge"][key]
    assert _check_tests(C.frame_of(case), case["tests"]) == 6 * len(case["tests"])


def test_edge_goldens_hold_the_cases_they_are_named_for():
    edge = GOLDEN["edge"]
    r = edge["total_dof0"]["tests"]
    assert r[0]["results"]["pearson"][0] == 0.0 and np.isnan(r[0]["results"]["pearson"][1]) and r[0]["results"]["pearson"][2] == 0
    assert r[1]["results"]["pearson"] == [0.0, 1.0, 0]
    z = edge["zero_cell"]["tests"][0]["results"]
    assert z["mod-log-likelihood"][0] == float("inf") and z["mod-log-likelihood"][1] == 0.0
    assert np.isnan(z["neyman"][0]) and np.isnan(z["neyman"][1])  # scipy: 0 * inf
    assert any(t["results"]["pearson"][2] == 1 for t in edge["two_by_two"]["tests"])


# ---------------------------------------------------------------------------- the kernel case table
KCASES = {c["name"]: c for c in C.kernel_cases()}


def _tables(name):
    return C.tables_of(KCASES[name]["codes"], KCASES[name]["families"])


def _reference(name, lam, yates):
    return [C.ci_ref(t, lam, yates, len(cols) > 2) for t, (cols, _) in zip(_tables(name), KCASES[name]["families"])]


def test_case_table_holds_what_it_is_for():
    """The shapes and contents the cases are named for ."""
    qz = [int(np.prod(cards[2:])) for _, cards in KCASES["qz_edges"]["families"]]
    assert qz[:6] == [1, 1, 2, C.CHUNK - 1, C.CHUNK, C.CHUNK + 1]
    assert any(cards[0] + cards[1] > C.SMALL and np.prod(cards[2:]) == 3 and cards[:2] == [40, 40]
               for _, cards in KCASES["general"]["families"])
    assert {c[0] + c[1] for _, c in KCASES["general"]["families"]} >= {C.SMALL, C.SMALL + 1}
    strata = [C.stratum_ref(_tables("strata")[0][:, :, z], 1.0) for z in range(6)]
    assert strata[4][3] == 0 and strata[1][1] == 0 and strata[1][3] == 0 and strata[2][1] == 1
    assert all(C.stratum_ref(t[:, :, z], 1.0)[1] == 1 for t in _tables("two_by_two") for z in range(t.shape[2]))
    t = _tables("zero_cells")[0][:, :, 0]
    assert t[0, 2] == 0 and t[2, 0] == 0 and t.sum(axis=0).min() > 0 and t.sum(axis=1).min() > 0
    refs = {lam: _reference("zero_cells", lam, True)[0] for lam in C.LAMBDAS.values()}
    assert np.isinf(float(refs[-1.0][0])) and float(refs[-1.0][2]) == 0.0 and np.isnan(float(refs[-2.0][0]))
    assert all(np.isfinite(float(refs[lam][0])) for lam in (1.0, 0.0, 2.0 / 3.0))
    assert all(r[1] == 0 for r in _reference("all_missing", 1.0, True))
    assert np.isnan(float(_reference("all_missing", 1.0, True)[1][2])) and float(_reference("all_missing", 1.0, True)[0][2]) == 1.0


# ---------------------------------------------------------------------------- PC under a host tester
def _skeleton_record(skeleton, sepsets):
    return (sorted(sorted(e) for e in skeleton.edges()), sorted([sorted(k), sorted(v)] for k, v in sepsets.items()))


def _pdag_record(pdag):
    return (sorted(pdag.nodes()), sorted(list(e) for e in pdag.directed_edges),
            sorted(sorted(e) for e in pdag.undirected_edges))


@pytest.fixture(scope="module")
def frame_s():
    return C.frame_of(GOLDEN["s"])


@pytest.mark.parametrize("name,lam", [("chi_square", 1.0), ("g_sq", 0.0)])
def test_pc_skeleton_and_pdag_of_s_under_a_host_tester(frame_s, name, lam):
    from pgmpy_amd.estimators.PC import PC, pc_skeleton

    want = GOLDEN["s"]["pc"][name]
    records = {}
    for variant in ("orig", "stable", "parallel"):
        tester = C.HostTester(frame_s, lam)
        skeleton, sepsets = pc_skeleton(list(frame_s.columns), tester, variant=variant, significance_level=ALPHA)
        records[variant] = _skeleton_record(skeleton, sepsets)
        assert records[variant] == (want["edges"], want["separating_sets"]), variant
        if variant != "orig":  # one batch per level
            assert len(tester.calls) == len({len(t[2]) for call in tester.calls for t in call})
    pdag = PC.orient_colliders(skeleton, sepsets).apply_meeks_rules(apply_r4=False).apply_meeks_rules(apply_r4=True)
    assert _pdag_record(pdag) == (want["pdag"]["nodes"], want["pdag"]["directed"], want["pdag"]["undirected"])
    assert want["pdag"]["directed"], "the frame has colliders to orient"


def test_pc_rounds_drop_later_candidates_and_keep_the_result(frame_s):
    from pgmpy_amd.estimators.PC import pc_skeleton

    whole = C.HostTester(frame_s)
    want = _skeleton_record(*pc_skeleton(list(frame_s.columns), whole, significance_level=ALPHA))
    split = C.HostTester(frame_s)
    assert _skeleton_record(*pc_skeleton(list(frame_s.columns), split, significance_level=ALPHA, max_tests=5)) == want
    assert all(len(call) <= 5 for call in split.calls) and len(split.calls) > len(whole.calls)
    assert sum(map(len, split.calls)) <= sum(map(len, whole.calls))


def test_pc_skeleton_exit_rule_and_knowledge(frame_s):
    from pgmpy_amd.estimators.PC import pc_skeleton

    cols = list(frame_s.columns)
    tester = C.HostTester(frame_s)
    skeleton, sepsets = pc_skeleton(cols, tester, significance_level=ALPHA, max_cond_vars=0)
    assert {len(t[2]) for call in tester.calls for t in call} == {0} and all(len(z) == 0 for z in sepsets.values())
    tester = C.HostTester(frame_s)
    skeleton, sepsets = pc_skeleton(cols, tester, significance_level=ALPHA, forbidden_edges=[("A", "C")],
                                    required_edges=[("A", "G")])
    assert not skeleton.has_edge("A", "C") and skeleton.has_edge("A", "G")
    tested = {frozenset(t[:2]) for call in tester.calls for t in call}
    assert frozenset(("A", "C")) not in tested and frozenset(("A", "G")) not in tested
    with pytest.raises(ValueError, match="variant"):
        pc_skeleton(cols, tester, variant="fast")


def test_orient_colliders():
    from pgmpy_amd.estimators import PC

    skeleton = nx.Graph([("A", "C"), ("B", "C"), ("C", "D")])
    pdag = PC.orient_colliders(skeleton, {frozenset(("A", "B")): (), frozenset(("A", "D")): ("C",),
                                          frozenset(("B", "D")): ("C",)})
    assert pdag.directed_edges == {("A", "C"), ("B", "C")} and pdag.undirected_edges == {("C", "D")}
    assert pdag.apply_meeks_rules().directed_edges == {("A", "C"), ("B", "C"), ("C", "D")}


# ---------------------------------------------------------------------------- PDAG
@pytest.mark.parametrize("i", range(len(GOLDEN["pdags"])))
def test_pdag_meek_rules_and_to_dag_match_the_reference(i):
    from pgmpy_amd.base import PDAG

    case = GOLDEN["pdags"][i]

    def make():
        return PDAG([tuple(e) for e in case["directed"]], [tuple(e) for e in case["undirected"]])

    for key, r4 in (("meek", False), ("meek_r4", True)):
        got = make().apply_meeks_rules(apply_r4=r4)
        if case["no_extension"]:
            # not the pattern of any DAG: the published rules may then orient an edge that closes a cycle, which
            # the reference's own extra guard on R1 refuses (a documented deviation); what it orients, they do
            assert {tuple(e) for e in case[key]["directed"]} <= got.directed_edges
            assert {frozenset(e) for e in got.edges()} == {frozenset(e) for e in make().edges()}
        else:
            assert _pdag_record(got) == (case[key]["nodes"], case[key]["directed"], case[key]["undirected"]), key
    start = make()
    assert start.apply_meeks_rules(inplace=True) is None
    assert start == make().apply_meeks_rules()
    # to_dag: which DAG of the class comes out depends on the order nodes are tried in (the reference: sorted
    # names; here: the order they were added), so the reference's DAG is compared in what every DAG of the
    # class shares: the skeleton and the unshielded colliders (no_extension: the skeleton only)
    dag = make().to_dag()
    got, want = set(dag.edges()), {tuple(e) for e in case["to_dag"]}
    assert {frozenset(e) for e in got} == {frozenset(e) for e in want} and len(got) == len(want)
    assert nx.is_directed_acyclic_graph(nx.DiGraph(list(got))) and {tuple(e) for e in case["directed"]} <= got
    if not case["no_extension"]:
        assert _colliders(got) == _colliders(want)


def _colliders(arcs):
    adjacent = set(arcs) | {(v, u) for u, v in arcs}
    return {(min(a, b), c, max(a, b)) for a, c in arcs for b, c2 in arcs if c2 == c and a != b and (a, b) not in adjacent}


def test_pdag_and_colliders_take_nodes_in_the_order_given():
    """Labels of mixed types cannot be sorted: every order is the order of the data columns.  Two
    v-structures that claim one edge in opposite directions leave it undirected."""
    from pgmpy_amd.base import PDAG
    from pgmpy_amd.estimators import PC

    skeleton = nx.Graph()
    skeleton.add_nodes_from([3, "b", 1, "d"])
    skeleton.add_edges_from([(3, 1), ("b", 1), (1, "d")])
    sep = {frozenset((3, "b")): (), frozenset((3, "d")): (1,), frozenset(("b", "d")): (1,)}
    pdag = PC.orient_colliders(skeleton, sep)
    assert list(pdag.nodes()) == [3, "b", 1, "d"] and pdag.directed_edges == {(3, 1), ("b", 1)}
    done = pdag.apply_meeks_rules()
    assert done.directed_edges == {(3, 1), ("b", 1), (1, "d")} and set(done.to_dag().edges()) == done.directed_edges
    assert set(PDAG([], [(3, "b"), ("b", 1), (1, "d"), ("d", 3)]).to_dag().edges()) == {(3, "b"), ("b", 1), (1, "d"), (3, "d")}
    # a - b - c - d with a, c and b, d not adjacent; colliders a -> b <- c and b -> c <- d both claim b - c
    chain = nx.Graph([("a", "b"), ("b", "c"), ("c", "d")])
    both = PC.orient_colliders(chain, {frozenset(("a", "c")): (), frozenset(("b", "d")): (), frozenset(("a", "d")): ()})
    assert both.directed_edges == {("a", "b"), ("d", "c")} and both.has_undirected_edge("b", "c")


def test_pdag_interface():
    from pgmpy_amd.base import PDAG
    from pgmpy_amd.models import DiscreteBayesianNetwork

    pdag = PDAG([("A", "C"), ("D", "C")], [("B", "A"), ("B", "D")])
    assert pdag.all_neighbors("A") == {"B", "C"} and pdag.undirected_neighbors("A") == {"B"}
    assert pdag.directed_children("A") == {"C"} and pdag.directed_parents("C") == {"A", "D"}
    assert pdag.has_directed_edge("A", "C") and not pdag.has_directed_edge("C", "A")
    assert pdag.has_undirected_edge("A", "B") and pdag.has_undirected_edge("B", "A") and not pdag.has_undirected_edge("A", "C")
    copy = pdag.copy()
    assert copy == pdag and copy is not pdag
    out = pdag.orient_undirected_edge("B", "A")
    assert out.has_directed_edge("B", "A") and not out.has_undirected_edge("A", "B") and pdag.has_undirected_edge("A", "B")
    assert out != pdag
    with pytest.raises(ValueError, match="not present"):
        pdag.orient_undirected_edge("A", "C")
    assert isinstance(pdag.to_dag(), DiscreteBayesianNetwork) and not pdag.to_dag().get_cpds()


# ---------------------------------------------------------------------------- the API's errors
FRAME = pd.DataFrame({"A": ["x", "y", "x", "y"], "B": ["u", "u", "v", "v"], "C": ["p", "q", "q", "p"]})


def test_get_callable_ci_test_names_and_errors():
    from pgmpy_amd.estimators import CITests as T

    for name in ("chi_square", "g_sq", "log_likelihood", "modified_log_likelihood", "power_divergence", "CHI_SQUARE"):
        assert T.get_callable_ci_test(name) is getattr(T, name.lower())
    assert T.get_callable_ci_test(None, data=FRAME) is T.chi_square
    assert T.get_callable_ci_test(len) is len
    with pytest.raises(ValueError, match="data is None"):
        T.get_callable_ci_test(None)
    for name in ("pearsonr", "gcm", "pillai", "independence_match"):
        with pytest.raises(ValueError, match="not built"):
            T.get_callable_ci_test(name)
    with pytest.raises(ValueError, match="must either be one of"):
        T.get_callable_ci_test("t_test")
    assert T.lambda_value("freeman-tukey") == -0.5 and T.lambda_value("cressie-read") == 2 / 3 and T.lambda_value(-2) == -2.0
    with pytest.raises(ValueError, match="invalid string"):
        T.lambda_value("freeman-tuckey")
    with pytest.raises(ValueError, match="finite"):
        T.lambda_value(float("nan"))


def test_ci_test_argument_errors_come_before_the_device():
    from pgmpy_amd.estimators import CITests as T

    for fn in (T.chi_square, T.g_sq, T.log_likelihood, T.modified_log_likelihood, T.power_divergence):
        with pytest.raises(ValueError, match="can't be in Z"):
            fn("A", "B", ["A"], FRAME, boolean=False)
        with pytest.raises(ValueError, match="can't be in Z"):
            fn("A", "B", ["C", "B"], FRAME, boolean=False)
    with pytest.raises(ValueError, match="iterable"):
        T.chi_square("A", "B", 3, FRAME)
    with pytest.raises(ValueError, match="can't be in Z"):
        T.CITester(FRAME).tests([("A", "B", []), ("A", "B", ["B"])])


def test_pc_api_errors():
    from pgmpy_amd.estimators import PC, ExpertKnowledge

    est = PC(FRAME)
    with pytest.raises(ValueError, match="variant"):
        est.estimate(variant="fast")
    with pytest.raises(ValueError, match="variant"):
        est.build_skeleton(variant="fast")
    with pytest.raises(ValueError, match="return_type"):
        est.estimate(return_type="graph")
    with pytest.raises(ValueError, match="must either be one of"):
        est.estimate(ci_test="t_test")
    with pytest.raises(ValueError, match="not built"):
        est.estimate(ci_test="pearsonr")
    with pytest.raises(NotImplementedError, match="enforce_expert_knowledge"):
        est.estimate(expert_knowledge=ExpertKnowledge(forbidden_edges=[("A", "B")]))
    with pytest.raises(NotImplementedError, match="temporal_order"):
        ExpertKnowledge(temporal_order=[["A"], ["B", "C"]])
    with pytest.raises(NotImplementedError, match="search_space"):
        ExpertKnowledge(search_space=[("A", "B")])
    with pytest.raises(NotImplementedError, match="independence assertions"):
        PC(FRAME, independencies=object())


def test_pc_estimate_with_a_callable_test_runs_without_a_device(frame_s):
    """A callable ci_test is called one test at a time with the reference's keyword arguments; with the
    restatement behind it estimate() reproduces the golden PDAG, the skeleton, and a DAG to fit."""
    from pgmpy_amd.estimators import PC
    from pgmpy_amd.models import DiscreteBayesianNetwork

    host = C.HostTester(frame_s)
    seen = []

    def ci_test(X, Y, Z, data=None, independencies=None, significance_level=None, **kwargs):
        assert data is frame_s and independencies is None and kwargs == {"extra": 1}
        seen.append((X, Y, tuple(Z)))
        return host.independent([(X, Y, Z)], significance_level)[0]

    want = GOLDEN["s"]["pc"]["chi_square"]
    for variant in ("orig", "stable", "parallel"):
        pdag = PC(frame_s).estimate(variant=variant, ci_test=ci_test, significance_level=ALPHA, extra=1)
        assert _pdag_record(pdag) == (want["pdag"]["nodes"], want["pdag"]["directed"], want["pdag"]["undirected"])
    skeleton, sepsets = PC(frame_s).estimate(ci_test=ci_test, return_type="skeleton", significance_level=ALPHA, extra=1)
    assert _skeleton_record(skeleton, sepsets) == (want["edges"], want["separating_sets"])
    dag = PC(frame_s).estimate(ci_test=ci_test, return_type="dag", significance_level=ALPHA, extra=1)
    assert isinstance(dag, DiscreteBayesianNetwork) and set(dag.nodes()) == set(frame_s.columns)
    assert {frozenset(e) for e in dag.edges()} == {frozenset(e) for e in want["edges"]}
    assert set(want["pdag"]["directed"] and map(tuple, want["pdag"]["directed"])) <= set(dag.edges())
    assert PC(frame_s).estimate(ci_test=ci_test, return_type="cpdag", significance_level=ALPHA, extra=1) == pdag
