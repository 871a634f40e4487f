"""Mplp without a device: the exports, the plan's limits, and the level schedule against the sequential order."""
import numpy as np
import pytest

from tests import mplp_cases as M
from pgmpy_amd import _native as N
from pgmpy_amd.inference._mplp import MplpPlan


def test_exports():
    import pgmpy_amd.inference as inference

    assert "Mplp" in inference.__all__ and inference.Mplp.__name__ == "Mplp"
    for name in ("pgm_mplp_plan_create", "pgm_mplp_plan_destroy", "pgm_mplp_plan_info", "pgm_mplp_run"):
        assert name in N.EXPORTED and hasattr(N.load_library(), name)


def edges_plan(n_edges):
    """n_edges isolated binary edges: 8 fp64 entries each, no set, no staging."""
    return MplpPlan([2] * (2 * n_edges), [(2 * e, 2 * e + 1) for e in range(n_edges)])


def test_plan_limits():
    with pytest.raises(ValueError, match=r"4 variables \(2 \.\. 3\)"):
        MplpPlan([2] * 4, [(0, 1, 2, 3)])
    with pytest.raises(ValueError, match=r"cardinality 255 \(1 \.\. 254\)"):
        MplpPlan([2, 255], [(0, 1)])
    # LDS = 8 (state + staging) + 64 + 2 ceil8(nodes) <= 163584: 2404 edges need 163536 bytes, 2405 need 163616
    inside = edges_plan(2404)
    assert (inside.info.lds_bytes, inside.info.lds_max, inside.info.theta_in_lds) == (163536, 163584, 0)
    with pytest.raises(ValueError, match="163616 bytes of LDS, 163584 at most"):
        edges_plan(2405)


@pytest.mark.parametrize("name", ["grid", "chord"])
def test_level_order_is_the_sequential_order(name):
    card, _, clusters, n_trip = case = M.EXACT[name]
    plan = MplpPlan(card, [vs for vs, _ in clusters], n_trip)
    assert max(np.bincount(plan.levels)) > 1 and plan.n_levels == max(plan.levels) + 1  # a level with several clusters
    by_level = sorted(range(len(clusters)), key=lambda c: plan.levels[c])
    assert by_level != list(range(len(clusters)))
    a, b = M.run(case, 20), M.run(case, 20, order=by_level)
    assert np.array_equal(a["state"].view(np.int64), b["state"].view(np.int64)) and len(a["state"]) == plan.state_len
