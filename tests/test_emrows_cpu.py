"""The host side of the rows E-step (pgm_fit_estep_rows): exports, the host-only query, every PGM_EINVAL of the
argument check (made before any HIP call, so none needs a device), the keyword validation of the Python surface.
Of the caps the host decides the tile edge and 32 / 33 latents: here.  Those per row are decided on the device:
test_emrows_gpu.py's unobserved33, config_cap and family_caps cases sit at and past each."""
import ctypes

import pandas as pd
import pytest

FAMILIES = [([0], [2]), ([1, 0], [3, 2]), ([2, 1], [2, 3])]


def _plan(families=FAMILIES):
    from pgmpy_amd.estimators._fit import FitPlan

    return FitPlan(families)


def test_exports_and_info():
    from pgmpy_amd import _native as N

    assert {"pgm_fit_estep_rows", "pgm_fit_estep_rows_info"} <= set(N.EXPORTED)
    assert len(N._SIGS["pgm_fit_estep_rows"][0]) == 15 and ctypes.sizeof(N.EmrInfo) == 64
    info = _plan().estep_rows_info()
    assert (info.block, info.rows_per_block, info.tile, info.tile_bins, info.total_bins) == (256, 1024, 1, 4096, 14)
    assert (info.max_unobserved, info.max_configs, info.max_component_families, info.max_row_families) == (32, 4096, 32, 128)
    assert info.n_columns == 3 and info.n_families == 3 and info.lds_bytes > 14 * 8 and info.blocks_per_cu == 3
    # the tile tier ends where the plan's bins pass the fit plan's LDS tile
    at, past = _plan([([0, 1], [64, 64])]).estep_rows_info(), _plan([([0, 1], [64, 64]), ([2], [1])]).estep_rows_info()
    assert (at.tile, past.tile) == (1, 0) and at.lds_bytes - past.lds_bytes == 4096 * 8
    # 32 latents are accepted, 33 are not
    wide = _plan([([i], [2]) for i in range(40)])
    assert wide.estep_rows_info(range(32)).n_latent == 32
    with pytest.raises(ValueError, match="33 latent columns"):
        wide.estep_rows_info(range(33))


@pytest.mark.parametrize("change, message", [
    (dict(plan=None), "null plan"), (dict(values=None), "null values"), (dict(codes=None), "null codes"),
    (dict(tables=None, loglik=None), "null tables and null loglik"), (dict(latent=[1, 1]), "listed twice"),
    (dict(latent=[9]), "in no family"), (dict(latent=[0], families=[([0], [2]), ([1, 0], [2, 3])]), "has cardinality"),
    (dict(families=[([0], [2]), ([1, 0], [2, 3])]), "two cardinalities"), (dict(flags=2), "flags 2"),
    (dict(n_cols=2), "observed column 2"), (dict(row0=1), "outside ld"),
])
def test_every_argument_is_checked_before_any_device_call(change, message):
    from pgmpy_amd import _native as N

    L = N.load_library()
    plan = _plan(change.get("families", FAMILIES))
    latent = change.get("latent", [])
    arr = (ctypes.c_int32 * max(len(latent), 1))(*latent)
    buf = ctypes.c_void_p(64)  # never dereferenced: the check fails first
    a = dict(plan=plan._h, values=buf, codes=buf, tables=buf, loglik=buf, flags=0, n_cols=3, row0=0)
    a.update({k: v for k, v in change.items() if k in a})
    with pytest.raises(ValueError, match=message):
        N.check(L.pgm_fit_estep_rows(a["plan"], arr, len(latent), a["flags"], a["values"], a["codes"], a["n_cols"], 8,
                                     a["row0"], 8, a["tables"], a["loglik"], None, None, None), "fit_estep_rows")


def test_the_incomplete_keyword_is_validated():
    from pgmpy_amd.estimators import ExpectationMaximization
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.metrics import BayesianModelProbability
    from pgmpy_amd.models import DiscreteBayesianNetwork

    model = DiscreteBayesianNetwork([("A", "B")])
    with pytest.raises(ValueError, match="incomplete must be 'drop' or 'marginalize'"):
        ExpectationMaximization(model, pd.DataFrame({"A": [0, 1], "B": [1, 0]}), incomplete="raise")
    model.add_cpds(TabularCPD("A", 2, [[0.5], [0.5]]), TabularCPD("B", 2, [[0.5, 0.5], [0.5, 0.5]], evidence=["A"], evidence_card=[2]))
    with pytest.raises(ValueError, match="incomplete must be 'raise' or 'marginalize'"):
        BayesianModelProbability(model).log_probability_codes(None, incomplete="drop")

