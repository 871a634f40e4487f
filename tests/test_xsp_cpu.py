"""The exact edge posteriors without a device: the export and the host checks of pgm_xs_posterior (csrc/pgmxs_plan.cpp),
ExhaustiveSearch.edge_posteriors' own checks, and the two references of tests/xsp_cases.py against each other."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from pgmpy_amd import _native as N
from pgmpy_amd.estimators import ExhaustiveSearch, ExpertKnowledge
from pgmpy_amd.estimators._xs import XsPlan
from tests import xsp_cases as C


@pytest.mark.parametrize("nodes, masks, scores, missing, message", [
    ([0], [0], [0.0], 0, "null result"), ([0], [0], [0.0], 1, "null result"), ([0], [0], [0.0], 2, "null result"),
    ([0], [0], [0.0], 3, "null result"), ([3], [0], [0.0], None, "family 0: node 3 of 3"),
    ([1], [0b010], [0.0], None, "node 1 is among its own parents"), ([1], [0b1001], [0.0], None, "has a bit at or above 3"),
    ([0, 0], [0b110, 0b110], [1.0, -np.inf], None, "node 0 is given the parent mask 0x6 twice"),
])
def test_argument_checks_before_any_device_call(nodes, masks, scores, missing, message):
    assert "pgm_xs_posterior" in N.EXPORTED and N.load_library().pgm_xs_posterior.argtypes
    plan = XsPlan(3)  # the handle lives as long as the plan
    a = [np.ascontiguousarray(x, dtype=t) for x, t in ((nodes, np.int32), (masks, np.uint32), (scores, np.float64))]
    flag, outs = ctypes.c_int32(), [np.empty(9), np.empty(2), np.empty(3)]
    out = [o.ctypes.data for o in outs] + [ctypes.byref(flag)]
    for handle, text in ((None, "null handle"), (plan._h, message)):
        given = [None if i == missing and handle else o for i, o in enumerate(out)]
        rc = N.load_library().pgm_xs_posterior(handle, *(x.ctypes.data for x in a), len(nodes), *given, None, None)
        assert rc == N.PGM_EINVAL and N.last_error().startswith("xs_posterior: ") and text in N.last_error()


@pytest.mark.parametrize("kind", ["full", "pruned"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_the_recurrence_is_the_sum_over_orders(n, kind):
    """Reference (b) in longdouble against reference (a): they share only the inputs.  The bound is a float64 one, far
    above what longdouble leaves and far below any mistake in a recurrence."""
    a, b = C.brute(n, C.families(n, kind)), C.recurrence(n, C.families(n, kind), C.LD)
    assert C.gaps(b, a) <= C.FLOOR and abs(b["log_z"][1] - b["log_z"][0]) <= C.FLOOR * max(1, abs(a["log_z"]))
    assert np.abs(a["mass"] - 1).max() <= C.FLOOR and (np.diag(b["edge_post"]) == 0).all()


def test_edge_posteriors_rejects_before_any_device_call():
    data = pd.DataFrame(np.zeros((4, 3), dtype=int), columns=list("ABC"))
    with pytest.raises(ValueError, match="required_edges create a cycle"):
        ExhaustiveSearch(data).edge_posteriors(expert_knowledge=ExpertKnowledge(required_edges=[("A", "B"), ("B", "C"), ("C", "A")]))
    with pytest.raises(ValueError, match=r"not in the data: \['Z'\]"):
        ExhaustiveSearch(data).edge_posteriors(expert_knowledge=ExpertKnowledge(forbidden_edges=[("A", "Z")]))
    with pytest.raises(NotImplementedError, match="temporal_order and search_space are not built"):
        ExhaustiveSearch(data).edge_posteriors(expert_knowledge=SimpleNamespace(search_space={("A", "B")}))
    with pytest.raises(ValueError, match="25 variables; the exact search takes 24 at most"):
        ExhaustiveSearch(pd.DataFrame(np.zeros((2, 25), dtype=int))).edge_posteriors(max_indegree=1)
