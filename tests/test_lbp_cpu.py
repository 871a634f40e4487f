"""LoopyBeliefPropagation without a device: the exports, the restatement against brute force on trees, the plan's
pairs, unique tables and LDS tier, and every rejected argument."""
import ctypes

import numpy as np
import pytest

from tests import lbp_cases as C
from pgmpy_amd import _native as N
from pgmpy_amd.inference._lbp import LbpPlan


def test_exports():
    import pgmpy_amd.inference as inference

    assert "LoopyBeliefPropagation" in inference.__all__
    assert all(f"pgm_lbp_{n}" in N.EXPORTED for n in ("plan_create", "plan_destroy", "plan_info", "run"))


@pytest.mark.parametrize("name", sorted(C.TREES))
def test_restatement_is_exact_on_trees(name):
    (marg, fbel, logz), got = C.brute_force(C.CASES[name]), C.run(C.CASES[name], C.TREES[name] + 1, dtype=C.LD)
    tol = 64 * np.finfo(C.LD).eps * max(1.0, abs(float(logz)))
    assert max(np.abs(got["marginals"] - marg).max(), np.abs(got["factor_beliefs"] - fbel).max(), abs(got["logz"] - logz)) <= tol


def plan_of(case, dedup=True):
    theta = np.concatenate([t.ravel() for _, t in case[2]])
    return LbpPlan(case[0], [vs for vs, _ in case[2]], theta if dedup else None)


def potts(side=16, k=4):
    table = np.exp(0.5 * np.eye(k))
    return [k] * side * side, None, [(e, table) for e in C.grid_edges(side, side)]


@pytest.mark.parametrize("case, dedup, pairs, msg, unique, in_lds, lds", [
    ("star", True, 9, 25, 6, 1, 8 * (16 + 3 * 25 + 32) + 64),
    ("grid_6x6", True, 120, 360, 60, 1, 8 * (108 + 3 * 360 + 540) + 64),
    ("pair_70", True, 2, 140, 1, 1, 8 * (140 + 3 * 140 + 4900) + 64),
    ("chain_120", True, 4, 480, 2, 0, 8 * (360 + 3 * 480) + 64),   # 230,400 bytes of tables stay in global memory
    ("potts", True, 960, 3840, 1, 1, 8 * (1024 + 3 * 3840 + 16) + 64),
    ("potts", False, 960, 3840, 480, 1, 8 * (1024 + 3 * 3840 + 7680) + 64)])
def test_plan_info(case, dedup, pairs, msg, unique, in_lds, lds):
    info = plan_of(potts() if case == "potts" else C.CASES[case], dedup).info
    assert (info.n_pairs, info.n_msg, info.n_tables_unique, info.theta_in_lds) == (pairs, msg, unique, in_lds)
    assert (info.lds_bytes, info.state_len, info.lds_max, info.block) == (lds, msg, 163584, 256)


@pytest.mark.parametrize("card, scopes, message", [
    ([2, 2], [()], r"0 variables \(1 \.\. 3\)"),
    ([2] * 4, [(0, 1, 2, 3)], r"4 variables \(1 \.\. 3\)"),
    ([2, 2], [(0, 1, 0)], "lists node 0 twice"),
    ([2, 2], [(0, 2)], "node 2 is out of range"),
    ([2, 0], [(0, 1)], r"cardinality 0 \(1 \.\. 254\)"),
    ([2, 255], [(0, 1)], r"cardinality 255 \(1 \.\. 254\)"),
    # binary nodes with a unary factor each take 8 (2 + 3 * 2) bytes: 2555 fill the LDS, the 2556th node's term is over
    ([2] * 2556, [(v,) for v in range(2556)], r"up to factor 2554 needs 163600 bytes of LDS \(163584 at most\)")])
def test_rejected_plans(card, scopes, message):
    with pytest.raises(ValueError, match=message):
        LbpPlan(card, scopes)
    if len(card) == 2556:
        assert LbpPlan(card[:-1], scopes[:-1]).info.lds_bytes == 163584


@pytest.mark.parametrize("change, message", [
    ({}, None), ({"damping": 1.0}, "damping"), ({"damping": -0.1}, "damping"), ({"damping": np.nan}, "damping"),
    ({"tol": -1.0}, "tolerance"), ({"tol": np.nan}, "tolerance"), ({"n_iter": -1}, "iterations"), ({"n_rows": -1}, "instances"),
    ({"marginals": None}, "null"), ({"unaries": None}, "null"), ({"values": 4}, "aligned"), ({"iters": 2}, "aligned")])
def test_run_arguments_are_checked_on_the_host(change, message):
    """n_rows = 0 is PGM_OK and launches nothing; every error returns before a HIP call, so host buffers do here."""
    plan, buf = plan_of(C.CASES["chain"]), np.zeros(64)
    at = lambda shift: ctypes.c_void_p(buf.ctypes.data + shift)
    a = dict(unaries=0, theta=0, n_rows=0, n_iter=5, tol=0.0, damping=0.0, state=None, marginals=0, values=0, iters=0)
    a.update(change)
    p = {k: None if a[k] is None else at(a[k]) for k in ("unaries", "theta", "state", "marginals", "values", "iters")}
    rc = N.load_library().pgm_lbp_run(plan._h, p["unaries"], p["theta"], a["n_rows"], a["n_iter"], a["tol"], a["damping"],
                                      p["state"], p["marginals"], p["values"], p["iters"], None, None, None)
    assert rc == (N.PGM_OK if message is None else N.PGM_EINVAL)
    assert message is None or message in N.last_error()
