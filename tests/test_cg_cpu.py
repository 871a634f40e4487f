"""The host side of the conditional-Gaussian scores: the exported symbols, the plan's caps and layout, the
parameter counts and the dtype rule.  No device."""
import numpy as np
import pandas as pd
import pytest

from pgmpy_amd import _native as N
from pgmpy_amd.estimators._cg import CgPlan, CondGaussData
from tests import cg_cases as C


def test_symbols_and_abi():
    names = ("pgm_cg_plan_create", "pgm_cg_plan_destroy", "pgm_cg_plan_info", "pgm_cg_plan_set_slice", "pgm_cg_moments_info",
             "pgm_cg_moments", "pgm_cg_score")
    L = N.load_library()
    assert all(n in N.EXPORTED and hasattr(L, n) for n in names)
    assert L.pgm_version() == 25


@pytest.mark.parametrize("family, cap", [
    (([0], [2], list(range(8)), True), "PGM_CG_MAX_CONT = 7"),
    ((list(range(33)), [1] * 33, [], True), "PGM_MAX_DIMS = 32"),
    (([0, 1], [255, 17], [], True), "PGM_CG_MAX_ROWS = 4096"),   # 4335 configurations, mp 1
    (([0, 1], [19, 27], [0, 1, 2, 3], True), "PGM_CG_MAX_ROWS = 4096"),  # 513 x 8
    (([0, 0], [2, 2], [], True), "twice"),
    (([], [], [1, 1], False), "twice"),
    (([0], [0], [], True), "1 .. 255"),
    (([0], [256], [], True), "1 .. 255"),
    (([0], [2], [], False), "no continuous column"),
])
def test_plan_refuses(family, cap):
    with pytest.raises(ValueError, match=cap):
        CgPlan([family])


@pytest.mark.parametrize("m, mp", [(0, 1), (1, 2), (3, 4), (4, 8), (7, 8)])
def test_plan_layout(m, mp):
    """One family of Q = 37 configurations beside a one-configuration one: mp, operand rows, tiles, offsets, jobs."""
    p = CgPlan([([0, 1], [1, 37], list(range(m)), True), ([], [], [0], False)])
    a, b = p.layout
    assert (a["mp"], a["Q"], a["operand_rows"], a["tiles"], a["mom_off"], a["jobs"]) == (mp, 37, 37 * mp, -(-37 * mp // 16), 0, 37)
    assert (b["mp"], b["Q"], b["tiles"], b["mom_off"], b["jobs"]) == (2, 1, 1, 37 * mp * mp, 1)
    assert p.info.total_tiles == a["tiles"] + 1 and p.info.total_blocks == -(-a["tiles"] // N.CG_TILES_PER_WAVE) + 1
    assert p.moments_size == 37 * mp * mp + 4 and C.mp_of(m) == mp
    assert p.moments_info(193)[:2] == (N.CG_SLICE_MIN, 1)
    p.set_slice(50)  # rounded up to a whole step
    assert p.moments_info(193)[:3] == (64, 4, 1) and p.moments_info(1 << 20)[:2] == (4096, 256)
    assert p.moments_info(8, x_ptr=16, ld_x=10, row0=2)[3] and not p.moments_info(8, x_ptr=16, ld_x=11, row0=2)[3]


def _frame():
    return pd.DataFrame({"a": ["u", "v", "w", "u"], "b": pd.Categorical(["p", "p", "p", "p"]), "c": ["s", "t", "s", "t"],
                         "i": [1, 2, 3, 4], "x": [0.5, 1.5, 2.5, np.nan], "f": [True, False, True, True]})


def test_dtype_rule():
    d = CondGaussData(_frame())
    assert d.code_variables == ["a", "b", "c"] and d.value_variables == ["i", "x", "f"]
    assert d.cardinalities == [3, 1, 2]
    ordered = CondGaussData(pd.DataFrame({"o": pd.Categorical([1, 2, 1], ordered=True), "n": [1, 2, 1]}))
    assert ordered.code_variables == ["o"] and ordered.value_variables == ["n"]


@pytest.mark.parametrize("variable, parents, k", [
    ("x", ["a", "b", "c", "i"], 3 * 2 * 3),       # continuous: q (|C| + 2), the one-state parent b not counted
    ("a", ["c", "b"], 2 * (3 - 1)),               # discrete, C empty: q (r - 1)
    ("a", ["c", "x", "i"], 2 * (3 - 1) * 4),      # discrete with continuous parents: q (r - 1)(|C| + 2)
    ("x", [], 2),
])
def test_parameter_counts(variable, parents, k):
    d = CondGaussData(_frame())
    fam, shape = d.family(variable, parents)
    assert d.n_parameters(shape, [3, 1, 2]) == k
    assert fam[3] == (variable in d.code_variables)
    CgPlan([fam])
