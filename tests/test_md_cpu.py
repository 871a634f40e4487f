"""MirrorDescentEstimator without a device: the conditions the cases must meet (on the numpy reference alone), the
plan of pgm_md_plan_create, the tier, every host-side check of the library, and the host classes."""
import ctypes

import numpy as np
import pytest

from pgmpy_amd import _native as N
from pgmpy_amd.estimators import MarginalEstimator, MirrorDescentEstimator
from pgmpy_amd.estimators._md import MdPlan
from pgmpy_amd.factors import FactorDict
from tests import md_cases as C


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_cases_keep_clear_of_ties(name):
    """No Armijo comparison within 1e-6 of a tie and, under L1, no |d_j| below 1e-9 n: a flipped branch cannot hide."""
    case = C.CASES[name]
    for row in range(len(case["totals"])):
        ref = C.reference(name, row)[0]
        assert (case["stepsize"] is None) == bool(ref["armijo"])
        assert all(abs(l - r) >= 1e-6 * max(abs(l), abs(r)) for l, r in ref["armijo"])
        assert case["metric"] != "L1" or ref["d_min"] >= 1e-9 * case["totals"][row]
    assert name != "l1_rejects" or ref["rejected"] > 0


def plan_of(name):
    case = C.CASES[name]
    return MdPlan(case["card"], case["cliques"], case["edges"], case["marginals"])


def test_plan_of_the_star_and_of_the_two_cliques():
    p = plan_of("star_two_none")
    assert (p.parent, p.level, p.depth) == ([-1, 0, 1, 1], [0, 1, 2, 2], 2)
    assert (p.clique_offsets, p.sep_offsets) == ([0, 4, 8, 12, 16], [0, 0, 2, 4, 6])
    assert p.sep_strides[1:, :, 0].tolist() == [[2, 1], [2, 1], [2, 1]] and not p.sep_strides[:, :, 1:].any()
    assert (p.owner, p.y_offsets) == ([1, 1, 3], [0, 2, 6, 8]) and p.marginal_strides[:, :2].tolist() == [[1, 0], [2, 1], [1, 0]]
    p = plan_of("two")
    assert (p.parent, p.level, p.clique_offsets, p.sep_offsets) == ([-1, 0], [0, 1], [0, 24, 48], [0, 0, 12])
    assert p.sep_strides[1, :, :2].tolist() == [[6, 2], [1, 4]]  # (c, b): in (c, b, d), in (a, b, c)
    assert (p.owner, p.y_offsets) == ([0, 1, 0], [0, 8, 14, 17]) and p.marginal_strides[:, :2].tolist() == [[12, 1], [1, 2], [4, 0]]
    assert (p.n_cells, p.n_sep, p.n_y, int(p.info.state_len), int(p.info.n_phases)) == (48, 12, 17, 120, 6)


def test_tier_is_chosen_by_size_and_can_be_forced():
    small, big = plan_of("two"), MdPlan([6] * 8, [tuple(range(8))], [], [(0,)])
    assert small.tier == N.MD_TIER_LDS and small.info.lds_bytes == 8 * (120 + 4 * 17) + 64 and small.info.scratch_len == 0
    assert big.tier == N.MD_TIER_GLOBAL and big.info.lds_bytes == 8 * 4 * 6 + 64 and big.info.scratch_len == 2 * 6 ** 8
    wave = plan_of("wave65")
    assert wave.tier == N.MD_TIER_LDS and 65536 < wave.info.lds_bytes <= wave.info.lds_max
    small.set_tier(N.MD_TIER_GLOBAL)
    assert small.tier == N.MD_TIER_GLOBAL and small.info.scratch_len == 120
    small.set_tier(N.MD_TIER_AUTO)
    assert small.tier == N.MD_TIER_LDS
    for plan, tier, word in ((big, N.MD_TIER_LDS, "bytes of LDS"), (small, 3, "tier 3")):
        with pytest.raises(ValueError, match=word):
            plan.set_tier(tier)
        assert word in N.last_error()


@pytest.mark.parametrize("args, word", [
    (([2] * 9, [tuple(range(9))], [], [(0,)]), "9 variables"),
    (([255], [(0,)], [], [(0,)]), "cardinality 255"),
    (([2, 2], [(0, 0)], [], [(0,)]), "twice"),
    (([2, 2], [(0, 2)], [], [(0,)]), "out of range"),
    (([2, 2, 2], [(0, 1), (1, 2)], [], [(0,)]), "0 edges between 2 cliques"),
    (([2, 2, 2], [(0, 1), (1, 2), (0, 2)], [(0, 1), (0, 1)], [(0,)]), "not a tree"),
    (([2, 2, 2], [(0, 1), (1, 2)], [(0, 1)], [(0, 2)]), "no clique holds the scope of marginal 0"),
    (([2, 2], [(0, 1)], [], []), "0 marginals"),
    (([16] * 8, [tuple(range(8))], [], [(0,)]), "2\\^30"),
    (([254] * 8, [tuple(range(8))], [], [(0,)]), "2\\^30"),  # the product is past int64
    (([181] * 4, [(0, 1, 2, 3), (3, 2, 1, 0)], [(0, 1)], [(0,)]), "up to clique 1 have 2146566242 cells"),  # each fits, the sum does not
])
def test_plan_limits_are_checked_on_the_host(args, word):
    with pytest.raises(ValueError, match=word):
        MdPlan(*args)


@pytest.mark.parametrize("change, word", [
    ({0: None}, "null targets"), ({10: None}, "null theta_out"), ({3: 2}, "theta_in has 2 rows"), ({4: -1}, "-1 instances"),
    ({5: 3}, "metric 3"), ({6: -1}, "-1 iterations"), ({7: float("nan"), 8: 0}, "step size"), ({7: float("inf"), 8: 0}, "step size"),
    ({8: 3}, "step mode 3"), ({1: 4100}, "not 8-byte aligned"), ({13: 4098}, "not 4-byte aligned"), ({"tier": 2}, "scratch slab of 120"),
])
def test_run_arguments_are_checked_before_any_device_call(change, word):
    """No device here: a call that got past its checks would fail with PGM_EDEVICE, not PGM_EINVAL."""
    plan, L = plan_of("two"), N.load_library()
    # after the handle: targets, totals, theta_in, theta_rows, n_rows, metric, iterations, stepsize, step_mode, scratch, 4 outputs, stream
    args = [4096, 4096, 4096, 1, 3, N.MD_L2, 5, 0.0, 1, None, 4096, 4096, 4096, 4096, None]
    assert L.pgm_md_run(plan._h, *args[:4], 0, *args[5:]) == N.PGM_OK  # no instance: nothing to launch
    plan.set_tier(change.pop("tier", N.MD_TIER_AUTO))
    for k, v in change.items():
        args[k] = v
    assert L.pgm_md_run(plan._h, *args) == N.PGM_EINVAL and word in N.last_error()


def test_host_classes():
    import pandas as pd

    with pytest.raises(ValueError, match=r"Could not find a corresponding clique for marginal: \('a', 'c'\) out of cliques: \[\('a', 'b'\)\]"):
        MarginalEstimator._clique_to_marginal({("a", "c"): None}, [("a", "b")])
    df = pd.DataFrame({"a": [0, 0, 1, 1, 1], "b": ["x", "z", "x", "z", "z"]})
    fd = FactorDict.from_dataframe(df, [("a", "b"), ("b",)], state_names={"b": ["x", "y", "z"]})
    assert fd[("a", "b")].values.tolist() == [[1, 0, 1], [1, 0, 2]] and fd[("b",)].values.tolist() == [2, 0, 3]
    assert FactorDict.from_dataframe(df, [("b",)])[("b",)].values.tolist() == [2, 3]  # the reference's sizing by nunique
    with pytest.raises(ValueError, match="cannot contain None"):
        FactorDict.from_dataframe(pd.DataFrame({"a": [0, None]}), [("a",)])
    two = (2 * fd - fd + 1) - 1
    assert all(np.array_equal(two[k].values, fd[k].values) for k in fd) and fd.dot(fd) == 7 + 13
    est = MirrorDescentEstimator.__new__(MirrorDescentEstimator)
    loss, grad = est._marginal_loss(FactorDict({("a", "b"): fd[("a", "b")]}), {("a", "b"): [(2 * fd)[("b",)]]}, "L2")
    assert loss == 0.5 * (4 + 0 + 9) and grad[("a", "b")].values.tolist() == [[-2, 0, -3], [-2, 0, -3]]
    with pytest.raises(ValueError, match="Metric must be one of L1 or L2."):
        est._marginal_loss(FactorDict({("a", "b"): fd[("a", "b")]}), {("a", "b"): [fd[("b",)]]}, "L3")
