"""The dynamic-network EM without a device: the numpy restatement of the E-step (tests/dbn_em_cases.py) against
brute-force enumeration of the unrolled network, the monotone log-likelihood of its iterations, the integer counts
of observed sequences, the symbol, the host-side argument checks of pgm_dbn_estep, the path pgm_dbn_estep_info
reports, and the input errors of DynamicBayesianNetwork.fit(estimator="EM")."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from tests import dbn_cases as C
from tests import dbn_em_cases as M


def _small_specs():
    return {"doc": C.doc_spec(), "two_iface": C.make_spec(seed=72, **C.TWO_IFACE), "cross": C.make_spec(seed=70, **C.CROSS)}


def _half_hidden(spec, T, B, seed, keep=()):
    ev = C.sample(spec, T, B, seed)
    gone = np.random.default_rng(seed + 1).random(ev.shape) < 0.5
    for v, name in enumerate(spec["names"]):
        if name in keep:
            gone[:, :, v] = False
    ev[gone] = C.MISSING
    return ev


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("name", ["doc", "two_iface", "cross"])
def test_restatement_equals_enumeration(name):
    """estep_ref (long double) equals the family posteriors summed from the unrolled joint, at T = 2 with half the
    cells hidden: nothing clamped, and the always-observed node Y clamped."""
    spec = _small_specs()[name]
    for clamped in ([], ["Y"]):
        evs = _half_hidden(spec, 2, 6, 500, keep=clamped)
        want0, want1, want_ll = 0, 0, []
        for ev in evs:
            t0, t1, ll = M.estep_enumerate(spec, ev)
            want0, want1 = want0 + t0, want1 + t1
            want_ll.append(ll)
        t0, t1, loglik, dead, n0, n1 = M.estep_ref(spec, clamped, evs)
        assert not dead.any()
        # 6 sequences x 3 slices of posteriors that are at most 1: 1e-17 per entry is long double's rounding
        assert float(np.abs(t0 - want0).max()) <= 1e-16 and float(np.abs(t1 - want1).max()) <= 1e-16
        assert float(np.abs(loglik - np.array(want_ll)).max()) <= 1e-16 * 8
        n = len(spec["card"])
        off0, off1, _, _ = M.layout(spec)
        for v in range(n):  # every family's table holds one unit of mass per sequence and slice
            assert abs(float(t0[off0[v]:off0[v] + spec["fam0"][v][1].size].sum()) - 6) <= 1e-15
            assert abs(float(t1[off1[v]:off1[v] + spec["fam1"][v][1].size].sum()) - 12) <= 1e-15
        # the terms counted per entry: at most one per sequence, slice and (i, x') that reaches it
        g = M._Geometry(spec, clamped)
        assert 0 < n0.max() <= 6 * g.J and 0 < n1.max() <= 12 * g.J * g.S


def test_em_loglik_never_decreases():
    """Five iterations of em_ref in long double on the HMM with its chain hidden: EM's guarantee."""
    spec = C.hmm_spec(states=3, n_obs=2)
    ev = C.sample(spec, 5, 60, 510)
    ev[:, :, 0] = C.MISSING
    start = C.hmm_spec(states=3, n_obs=2, seed=511)
    _, _, lls = M.em_ref(start, spec["names"][1:], ev, 5)
    assert len(lls) == 5 and all(b >= a for a, b in zip(lls, lls[1:])), lls
    assert lls[-1] > lls[0]


def test_observed_sequences_give_integer_counts():
    """Fully observed evidence: every weight is g / g = 1, the tables are the integer family counts, in fp64 and in
    long double, clamped or free."""
    spec = C.make_spec(seed=72, **C.TWO_IFACE)
    ev = C.sample(spec, 4, 40, 520)
    want0, want1 = M.observed_counts(spec, ev)
    assert want0.sum() == 40 * 4 and want1.sum() == 40 * 4 * 4
    for clamped in ([], spec["names"], ["W", "Y"]):
        for dtype in (np.float64, np.longdouble):
            t0, t1, _, dead, _, _ = M.estep_ref(spec, clamped, ev, dtype)
            assert not dead.any()
            assert np.array_equal(t0.astype(np.float64), want0) and np.array_equal(t1.astype(np.float64), want1)


def test_normalise_is_the_m_step():
    spec = C.doc_spec()
    t0, t1 = M.observed_counts(spec, C.sample(spec, 3, 50, 530))
    v0, v1 = M.normalise(spec, t0, t1)
    fitted = M.with_values(spec, v0, v1)
    for fams in (fitted["fam0"], fitted["fam1"]):
        for _, tab in fams:
            np.testing.assert_allclose(tab.sum(axis=0), 1.0, rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------ the library
def test_symbols_and_abi():
    import pgmpy_amd
    from pgmpy_amd import _native as N

    lib = N.load_library()
    assert "pgm_dbn_estep" in N.EXPORTED and len(lib.pgm_dbn_estep.argtypes) == 17
    assert "pgm_dbn_estep_info" in N.EXPORTED and len(lib.pgm_dbn_estep_info.argtypes) == 3
    assert ctypes.sizeof(N.DbnEstepInfo) == 4 * 4 + 3 * 8
    assert lib.pgm_version() == 25 and pgmpy_amd.ABI_VERSION == 25


def test_estep_refuses_bad_arguments_without_a_device():
    """Every host check of pgm_dbn_estep: those of pgm_dbn_run for a smoother, the tables, the flags."""
    from pgmpy_amd import _native as N
    from pgmpy_amd.inference._dbn import DbnPlan

    L = N.load_library()
    p = DbnPlan([2, 3], [0, 1], [0, 0], [([0], [2]), ([1], [3])], [([2, 0], [2, 2]), ([3, 1], [3, 3])])
    assert p.info.n_configs == 2 and p.info.n_interface == 2
    buf = np.zeros(8192, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 64
    need = 16 * 3 * (2 + 1) * 8  # n_rows x slices x (S + 1) doubles

    def run(plan=p._h, codes=base, n_cols=6, ld=16, row0=0, n_rows=16, n_slices=3, v0=base, v1=base, t0=base, t1=base,
            loglik=None, scratch=base, scratch_bytes=need, flags=0):
        return L.pgm_dbn_estep(plan, codes, n_cols, ld, row0, n_rows, n_slices, v0, v1, t0, t1, loglik, None, scratch,
                               scratch_bytes, flags, None)

    for kwargs in (
            dict(plan=None), dict(codes=None), dict(v0=None), dict(v1=None),
            dict(t0=None), dict(t1=None), dict(t0=base + 4), dict(t1=base + 2),
            dict(flags=2), dict(flags=3), dict(flags=0x80000000),
            dict(v0=base + 4), dict(v1=base + 2), dict(loglik=base + 4), dict(scratch=base + 4),
            dict(n_cols=5), dict(n_slices=2), dict(n_slices=0, n_cols=0), dict(n_slices=65536, n_cols=131072),
            dict(row0=1), dict(n_rows=17), dict(row0=-1), dict(n_rows=-1), dict(ld=-1),
            dict(scratch_bytes=need - 8), dict(scratch=None), dict(scratch_bytes=-1), dict(scratch_bytes=0)):
        assert run(**kwargs) == N.PGM_EINVAL, kwargs
    # nothing to launch: PGM_OK without a device, with and without the flag
    assert run(n_rows=0, scratch=None, scratch_bytes=0) == N.PGM_OK
    assert run(n_rows=0, row0=16, flags=N.DBN_ESTEP_DIRECT) == N.PGM_OK
    info = N.DbnEstepInfo()
    assert L.pgm_dbn_estep_info(None, 0, ctypes.byref(info)) == N.PGM_EINVAL
    assert L.pgm_dbn_estep_info(p._h, 2, ctypes.byref(info)) == N.PGM_EINVAL
    assert L.pgm_dbn_estep_info(p._h, 0, None) == N.PGM_OK


def test_estep_info_reports_the_path():
    from pgmpy_amd import _native as N

    _plan = M.plan_of
    p = _plan(C.doc_spec(), ["X", "Y"])
    state = (int(p.info.lds_bytes) + 7) // 8 * 8
    tile = 8 * (int(p.info.values0) + int(p.info.values1))
    i = p.estep_info()
    assert (i.path, i.tile_fits, i.tile_bytes, i.lds_bytes) == (N.DBN_ESTEP_TILE, 1, tile, state + tile)
    assert i.blocks_per_cu == 32 and i.max_blocks == 256 * 32
    d = p.estep_info(direct=True)
    assert (d.path, d.tile_fits, d.lds_bytes, d.max_blocks, d.blocks_per_cu) == (N.DBN_ESTEP_DIRECT, 1, p.info.lds_bytes, 0, 0)
    # the large-table case: 20,655 transition entries do not fit 160 KiB
    case = M.large_table_case()
    big = _plan(case["spec"], case["clamped"])
    assert big.info.values1 == 9 * 9 * 255 + 255 and big.info.n_configs == 9  # X' | X, C and C' itself
    i = big.estep_info()
    assert (i.path, i.tile_fits, i.lds_bytes, i.max_blocks) == (N.DBN_ESTEP_DIRECT, 0, big.info.lds_bytes, 0)
    assert i.tile_bytes > N.DBN_LDS_MAX
    # a tile that takes most of a CU's LDS: fewer workgroups per CU, a smaller grid
    mid = C.make_spec(names=["C", "X"], card=[100, 9], intra=[("C", "X")], inter=[("X", "X")], seed=152)
    i = _plan(mid, ["C"]).estep_info()
    assert i.path == N.DBN_ESTEP_TILE and i.blocks_per_cu == N.DBN_LDS_MAX // i.lds_bytes == 2 and i.max_blocks == 512


# ------------------------------------------------------------------------------------------------ fit: input errors
def test_fit_em_input_errors():
    spec = C.hmm_spec(states=3, n_obs=2)
    model = C.to_model(spec)
    frame = pd.DataFrame({("O0", 0): [0, 1], ("O0", 1): [1, 1], ("O1", 0): [0, 0], ("O1", 1): [1, 0]})
    frame.columns = pd.Index(list(frame.columns), tupleize_cols=False)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="max_iter"):
            model.fit(frame, estimator="EM", max_iter=bad)
    with pytest.raises(ValueError, match="atol"):
        model.fit(frame, estimator="EM", atol=-1.0)
    for bad in ("zeros", "Random", {}):
        with pytest.raises(ValueError, match="init_cpds"):
            model.fit(frame, estimator="EM", init_cpds=bad)
    with pytest.raises(ValueError, match="Only Maximum Likelihood.*EM"):
        model.fit(frame, estimator="Bayes")
    with pytest.raises(ValueError, match="start from time slice 0"):
        model.fit(frame.loc[:, [("O0", 1), ("O1", 1)]], estimator="EM")
    # a model that lacks a CPD: the node is named
    from pgmpy_amd.models import DynamicBayesianNetwork

    bare = DynamicBayesianNetwork()
    bare.add_edges_from([(("H", 0), ("O0", 0)), (("H", 0), ("O1", 0)), (("H", 0), ("H", 1))])
    bare.add_cpds(*[c for c in model.get_cpds() if c.variable != ("H", 1)])
    with pytest.raises(ValueError, match=r"No CPD associated with \(H, 1\)"):
        bare.fit(frame, estimator="EM")
    with pytest.raises(ValueError, match="n_time_slices"):
        import torch

        model.fit_codes(torch.zeros((5, 4), dtype=torch.uint8), 2)
