"""Gibbs sampling without a GPU: the numpy restatement (the sweep coordinate of the stream, the exact sweep
transition matrix, the distribution), the host plan unit (tools/gibbs_plan_selftest.cpp over
pgmpy_amd/csrc/pgmgibbs_plan.cpp, plain and with ASan + UBSan), the plan rejections and the argument
checks of the pgm_gibbs_* entry points through the library, the Python argument checks, and no compute
without a device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import gibbs_cases as G
from tests import sample_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- the stream
def test_sweep_zero_is_the_forward_stream():
    rows = np.array([0, 1, 12345, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3], dtype=np.uint64)
    for col in (0, 1, 36, 1040):
        assert (G.uniform3_bits(77, rows, col, 0) == S.uniform_bits(77, rows, col)).all()
        assert (G.uniform3_bits(77, rows, col, 1) != S.uniform_bits(77, rows, col)).all()


def test_sweep_is_the_fourth_counter_word():
    x = S.philox4x32_10((7, 1, 3, 0xffffffff), (9, 2))
    seed, chain = (2 << 32) | 9, (1 << 32) | 7
    assert int(G.uniform3_bits(seed, [chain], 6, 2 ** 32 - 1)[0]) == (int(x[0]) << 21) | (int(x[1]) >> 11)
    assert int(G.uniform3_bits(seed, [chain], 7, 2 ** 32 - 1)[0]) == (int(x[2]) << 21) | (int(x[3]) >> 11)
    u = G.uniforms3(5, np.arange(4096, dtype=np.uint64), 3, 9)
    assert ((u >= 0) & (u < 1)).all() and 0.45 < u.mean() < 0.55


# ---------------------------------------------------------------------------- the restatement
def test_restatement_clamp_records_and_split():
    """Clamped columns never change, records are the states after every thin-th sweep, and sweeps split
    over calls continue the same chains."""
    nodes, fams, tables, card = G.bn_factors(S.hand_model())
    start = S.sample_ref(fams, tables, 64, seed=3)[0]
    clamp = [0, 0, 0, 1]
    full, recs, undrawn, bad = G.gibbs_ref(fams, tables, card, start, 7, seed=3, clamp=clamp, thin=2)
    assert not undrawn and not bad and len(recs) == 3 and (full[3] == start[3]).all()
    a = G.gibbs_ref(fams, tables, card, start, 2, seed=3, clamp=clamp)[0]
    assert (a == recs[0]).all()
    b = G.gibbs_ref(fams, tables, card, a, 5, seed=3, clamp=clamp, first_sweep=3)[0]
    assert (b == full).all()
    part = G.gibbs_ref(fams, tables, card, start[:, 10:20], 7, seed=3, clamp=clamp, first_chain=10)[0]
    assert (part == full[:, 10:20]).all()
    assert (full[:3] != start[:3]).any()


def test_restatement_reports_bad_codes_and_zero_totals():
    factors = [([0], [2]), ([1, 0], [2, 2])]
    tables = [np.array([0.5, 0.5]), np.array([1.0, 0.0, 0.0, 1.0])]  # X1 = X0, deterministic
    start = np.array([[0, 1, 0], [1, 0, 7]], dtype=np.uint8)  # chain 0 has probability 0, chain 2 a bad code
    out, _, undrawn, bad = G.gibbs_ref(factors, tables, [2, 2], start, 1, seed=1)
    assert bad and (out[:, 2] == start[:, 2]).all()
    assert not undrawn  # X0 | X1 is a point mass, so the chain moves to a state of positive probability
    tables[1] = np.array([0.0, 0.0, 1.0, 1.0])  # P(X1 = 0 | .) = 0: X1 = 0 has no drawable conditional for X0
    out, _, undrawn, bad = G.gibbs_ref(factors, tables, [2, 2], start[:, 1:2], 1, seed=1)
    assert undrawn and not bad and out[0, 0] == start[0, 1]


def test_sweep_matrix_is_stochastic_and_keeps_the_posterior():
    for case in (G.hand_posterior, G.triangle_posterior):
        _, _, _, _, joint, burn = case()
        T = G.sweep_matrix(joint, [0, 1, 2])
        assert joint.size == 12 and np.allclose(T.sum(axis=1), 1, atol=1e-13)
        assert np.allclose(joint.reshape(-1) @ T, joint.reshape(-1), atol=1e-13)
        print(f"burn-in {burn}")
        assert 1 <= burn <= 64


def _distribution(case, evidence_col=None):
    nodes, factors, tables, card, joint, burn = case()
    n = G.N_DIST
    if evidence_col is None:
        start, clamp = G.start_ref(card, n, seed=G.SEED_DIST), None
    else:
        given = np.full((len(card), n), 255, dtype=np.uint8)
        given[evidence_col] = 0
        modes = [S.GIVEN if cols[0] == evidence_col else S.FREE for cols, _ in factors]
        start = S.sample_ref(factors, tables, n, seed=G.SEED_DIST, given=given, modes=modes)[0]
        clamp = [int(c == evidence_col) for c in range(len(card))]
    out, _, undrawn, bad = G.gibbs_ref(factors, tables, card, start, burn, seed=G.SEED_DIST, clamp=clamp)
    assert not undrawn and not bad
    return S.six_sigma_cells(out[:3], joint, n)


def test_restatement_matches_the_posterior_with_evidence():
    """hand_model() given D = d0: 8,192 chains after the computed burn-in, every cell of the joint over
    A, B, C within six sigma of the exact posterior."""
    worst = _distribution(G.hand_posterior, evidence_col=3)
    print(f"worst cell deviation {worst:.2f} sigma")
    assert worst <= 6.0


def test_restatement_matches_the_triangle_network():
    worst = _distribution(G.triangle_posterior)
    print(f"worst cell deviation {worst:.2f} sigma")
    assert worst <= 6.0


# ---------------------------------------------------------------------------- the host plan unit
def _build_selftest(tmp_path_factory, flags):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gibbs_plan") / "gibbs_plan_selftest")
    csrc = os.path.join(ROOT, "pgmpy_amd", "csrc")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "include"), "-I", csrc,
                            os.path.join(ROOT, "tools", "gibbs_plan_selftest.cpp"),
                            os.path.join(csrc, "pgmgibbs_plan.cpp"), os.path.join(csrc, "pgmfit_plan.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    return _build_selftest(tmp_path_factory, [])


def test_gibbs_plan_selftest(selftest):
    run = subprocess.run([selftest], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "gibbs_plan_selftest ok" in run.stdout, run.stdout + run.stderr


def test_gibbs_plan_selftest_sanitized(tmp_path_factory):
    """The same stand-alone host program under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only)."""
    exe = _build_selftest(tmp_path_factory, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "gibbs_plan_selftest ok" in run.stdout, run.stdout + run.stderr


UNIFORM3_POINTS = [(0, 0, 0, 1), (0, 0, 1, 1), (7, 5, 3, 2), (2 ** 64 - 1, 2 ** 32 - 1, 1040, 2 ** 32 - 1),
                   (12345, 2 ** 32, 36, 17), (0xDEADBEEFCAFEF00D, 2 ** 62 + 17, 2 ** 31 + 1, 2 ** 31)]


def test_host_stream_equals_restatement(selftest):
    """pgm_sample.h's sample_uniform3 (the code the kernel compiles) against the numpy restatement: chains
    past 2^32, an odd and an even column, the last sweep; and sweep 0 is sample_uniform."""
    def run(*args):
        out = subprocess.run([selftest, *map(str, args)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        return int(out.stdout)

    for seed, chain, col, sweep in UNIFORM3_POINTS:
        assert run("--uniform3", seed, chain, col, sweep) == int(G.uniform3_bits(seed, [chain], col, sweep)[0])
    for seed, chain, col, _ in UNIFORM3_POINTS:
        assert run("--uniform3", seed, chain, col, 0) == int(S.uniform_bits(seed, [chain], col)[0])


def test_sample_selftest_prints_the_same_sweep_zero(tmp_path_factory):
    """sweep = 0 equals sample_uniform as the forward sampler's own self-test prints it."""
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "pgmpy_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("sample_plan") / "sample_plan_selftest")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                            os.path.join(ROOT, "tools", "sample_plan_selftest.cpp"),
                            os.path.join(csrc, "pgmsample_plan.cpp"), os.path.join(csrc, "pgmfit_plan.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    gibbs = _build_selftest(tmp_path_factory, [])
    for seed, chain, col, _ in UNIFORM3_POINTS[2:5]:
        a = subprocess.run([exe, "--uniform", str(seed), str(chain), str(col)], capture_output=True, text=True, timeout=120)
        b = subprocess.run([gibbs, "--uniform3", str(seed), str(chain), str(col), "0"], capture_output=True, text=True,
                           timeout=120)
        assert a.returncode == 0 and b.returncode == 0 and int(a.stdout) == int(b.stdout)


# ---------------------------------------------------------------------------- the library, no device
def _factors(N, factors):
    arr = (N.FitFamily * max(len(factors), 1))()
    for f, (cols, cards) in enumerate(factors):
        arr[f].n_vars = len(cols)
        for v, (c, k) in enumerate(zip(cols[:N.PGM_MAX_DIMS], cards[:N.PGM_MAX_DIMS])):
            arr[f].col[v], arr[f].card[v] = c, k
    return arr


def _cards(card):
    return (ctypes.c_int32 * max(len(card), 1))(*card)


REJECTED_PLANS = [
    ("column_in_no_factor", [([0], [2])], [2, 2], "column 1 is in no factor"),
    ("cardinality_differs_from_card", [([0], [2])], [3], "factor 0 column 0 cardinality 2, the column has 3"),
    ("cardinality_differs_between_factors", [([0, 1], [2, 2]), ([1], [3])], [2, 2],
     "factor 1 column 1 cardinality 3, the column has 2"),
    ("cardinality_255", [([0], [255])], [255], "column 0 cardinality 255 (1 .. 254)"),
    ("cardinality_0", [([0], [0])], [0], "column 0 cardinality 0 (1 .. 254)"),
    ("33_columns", [(list(range(33)), [2] * 33)], [2] * 33, "factor 0 has 33 columns (1 .. 32)"),
    ("no_columns", [([], [])], [2], "factor 0 has 0 columns (1 .. 32)"),
    ("2_to_31_entries", [(list(range(31)), [2] * 31)], [2] * 31, "table exceeds 2^31 - 1 bins"),
    ("column_twice", [([0, 1, 0], [2, 2, 2])], [2, 2], "factor 0 lists column 0 twice"),
    ("column_out_of_range", [([2], [2])], [2, 2], "column 2 (0 .. 1)"),
]


@pytest.mark.parametrize("name,factors,card,msg", REJECTED_PLANS, ids=[r[0] for r in REJECTED_PLANS])
def test_plan_validation_through_the_library(name, factors, card, msg):
    from pgmpy_amd import _native as N

    lib = N.load_library()
    h = ctypes.c_void_p()
    rc = lib.pgm_gibbs_plan_create(_factors(N, factors), len(factors), _cards(card), len(card), ctypes.byref(h))
    assert rc == N.PGM_EINVAL and not h.value
    assert msg in N.last_error()


def test_gibbs_entry_points_reject_bad_arguments_on_the_host():
    """pgm_gibbs_* validate every argument before any HIP call: PGM_EINVAL with no device present."""
    from pgmpy_amd import _native as N

    lib = N.load_library()
    h = ctypes.c_void_p()
    EINVAL = N.PGM_EINVAL
    good, card = [([0], [3]), ([2, 0], [2, 3]), ([1, 2], [2, 2])], [3, 2, 2]
    create = lib.pgm_gibbs_plan_create
    assert create(None, 3, _cards(card), 3, ctypes.byref(h)) == EINVAL
    assert create(_factors(N, good), 3, None, 3, ctypes.byref(h)) == EINVAL
    assert create(_factors(N, good), 3, _cards(card), 3, None) == EINVAL
    assert create(_factors(N, good), 0, _cards(card), 3, ctypes.byref(h)) == EINVAL
    assert create(_factors(N, good), 3, _cards(card), 0, ctypes.byref(h)) == EINVAL
    assert create(_factors(N, good), 3, _cards(card), 3, ctypes.byref(h)) == N.PGM_OK
    try:
        codes = np.full((3, 8), 1, dtype=np.uint8)
        values, trace = np.full(13, 0.5), np.full((3, 16), 9, dtype=np.uint8)
        pc, pv, pt = (a.ctypes.data_as(ctypes.c_void_p) for a in (codes, values, trace))
        sw = lib.pgm_gibbs_sweep
        #            plan values codes n_cols ld row0 n first_chain first_sweep n_sweeps seed clamp trace ld_trace thin uniforms stream
        assert sw(None, pv, pc, 3, 8, 0, 8, 0, 1, 2, 1, None, None, 0, 1, None, None) == EINVAL    # null plan
        assert sw(h, None, pc, 3, 8, 0, 8, 0, 1, 2, 1, None, None, 0, 1, None, None) == EINVAL     # null values
        assert sw(h, pv, None, 3, 8, 0, 8, 0, 1, 2, 1, None, None, 0, 1, None, None) == EINVAL     # null codes
        assert sw(h, pv, pc, 3, 7, 0, 8, 0, 1, 2, 1, None, None, 0, 1, None, None) == EINVAL       # ld < n_chains
        assert sw(h, pv, pc, 3, 8, -1, 4, 0, 1, 2, 1, None, None, 0, 1, None, None) == EINVAL      # negative row0
        assert sw(h, pv, pc, 3, 8, 5, 4, 0, 1, 2, 1, None, None, 0, 1, None, None) == EINVAL       # the window leaves ld
        assert sw(h, pv, pc, 3, 8, 0, -1, 0, 1, 2, 1, None, None, 0, 1, None, None) == EINVAL      # negative n_chains
        assert sw(h, pv, pc, 3, 8, 0, 8, -1, 1, 2, 1, None, None, 0, 1, None, None) == EINVAL      # negative first_chain
        assert sw(h, pv, pc, 3, 8, 0, 8, 2 ** 63 - 4, 1, 2, 1, None, None, 0, 1, None, None) == EINVAL  # the stream ends
        assert sw(h, pv, pc, 2, 8, 0, 8, 0, 1, 2, 1, None, None, 0, 1, None, None) == EINVAL       # codes lacks a column
        assert "codes has 2" in N.last_error()
        assert sw(h, pv, pc, 3, 8, 0, 8, 0, 0, 2, 1, None, None, 0, 1, None, None) == EINVAL       # sweep 0 is forward's
        assert "outside 1 .. 2^32 - 1" in N.last_error()
        assert sw(h, pv, pc, 3, 8, 0, 8, 0, 1, -1, 1, None, None, 0, 1, None, None) == EINVAL      # negative n_sweeps
        assert sw(h, pv, pc, 3, 8, 0, 8, 0, 2 ** 32 - 1, 2, 1, None, None, 0, 1, None, None) == EINVAL  # past the last sweep
        assert sw(h, pv, pc, 3, 8, 0, 8, 0, 2 ** 32, 1, 1, None, None, 0, 1, None, None) == EINVAL
        assert sw(h, pv, pc, 3, 8, 0, 8, 0, 1, 2, 1, None, None, 0, 0, None, None) == EINVAL       # thin 0
        assert sw(h, pv, pc, 3, 8, 0, 8, 0, 1, 4, 1, None, pt, 15, 2, None, None) == EINVAL        # 2 records x 8 > 15
        assert "exceed ld_trace 15" in N.last_error()
        assert sw(h, pv, pc, 3, 8, 0, 0, 0, 1, 2, 1, None, None, 0, 1, None, None) == N.PGM_OK     # no chains: no launch
        assert sw(h, pv, pc, 3, 8, 0, 8, 0, 1, 0, 1, None, None, 0, 1, None, None) == N.PGM_OK     # no sweeps: no launch
        st = lib.pgm_gibbs_start
        assert st(None, pc, 3, 8, 0, 8, 0, 1, None) == EINVAL
        assert st(h, None, 3, 8, 0, 8, 0, 1, None) == EINVAL
        assert st(h, pc, 3, 8, 1, 8, 0, 1, None) == EINVAL
        assert st(h, pc, 2, 8, 0, 8, 0, 1, None) == EINVAL
        assert st(h, pc, 3, 8, 0, 8, -1, 1, None) == EINVAL
        assert st(h, pc, 3, 8, 0, 0, 0, 1, None) == N.PGM_OK
        assert lib.pgm_gibbs_plan_info(None, 8, None, None, None, None, None) == EINVAL
        assert lib.pgm_gibbs_plan_info(h, -1, None, None, None, None, None) == EINVAL
        assert (codes == 1).all() and (trace == 9).all()
    finally:
        assert lib.pgm_gibbs_plan_destroy(h) == N.PGM_OK
    assert lib.pgm_gibbs_plan_destroy(None) == N.PGM_OK
    assert ctypes.sizeof(N.GibbsInfo) == 2 * 4 + 3 * 8 + 8 * 4


def test_plan_info_layout_and_path_choice():
    """pgm_gibbs_plan_info: the fit plan's layout, the incidence lists, the launch geometry and the path."""
    from pgmpy_amd import _native as N
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.sampling._gibbs import GLOBAL, LDS, GibbsPlan

    factors = [([3], [2]), ([0, 3], [3, 2]), ([2, 3], [4, 2]), ([1, 0, 2], [2, 3, 4])]
    plan = GibbsPlan(factors, [3, 2, 4, 2])
    fit = FitPlan(factors)
    assert (plan.offsets, plan.sizes, plan.total_entries) == (fit.offsets, fit.sizes, fit.total_bins) == ([0, 2, 8, 16], [2, 6, 8, 24], 40)
    assert plan.inc_off == [0, 2, 3, 5, 8]
    assert plan.incident == [[(1, 0), (3, 1)], [(3, 0)], [(2, 0), (3, 2)], [(0, 0), (1, 1), (2, 1)]]
    assert plan.incident == G.incident(factors, 4)
    i = plan.launch_info(1030)
    assert (i.n_factors, i.n_cols, i.total_incidences, i.max_degree, i.max_card) == (4, 4, 8, 3, 4)
    assert i.block == 256 and i.blocks == 5 and i.path == LDS and i.lds_bytes == 4 * i.block
    assert i.lds_bytes <= i.lds_budget <= 160 * 1024 and i.reg_card >= 2
    assert plan.launch_info(0).blocks == 0 and plan.launch_info(256).blocks == 1
    # the threshold between the paths, read from the plan itself
    edge = i.lds_budget // i.block
    for n, path in ((edge, LDS), (edge + 1, GLOBAL)):
        f, _, card = G.chain_network(n)
        info = GibbsPlan(f, card).launch_info(130)
        assert info.path == path and info.lds_bytes == (n * info.block if path == LDS else 0), n
    assert (LDS, GLOBAL) == (N.GIBBS_LDS, N.GIBBS_GLOBAL) == (0, 1)


def test_new_symbols_are_bound_and_the_abi_version_stays():
    from pgmpy_amd import _native as N

    for name in ("pgm_gibbs_plan_create", "pgm_gibbs_plan_destroy", "pgm_gibbs_plan_info", "pgm_gibbs_start",
                 "pgm_gibbs_sweep"):
        assert name in N.EXPORTED and hasattr(N.load_library(), name)
    assert N.load_library().pgm_version() == 25


# ---------------------------------------------------------------------------- Python: errors first
def test_gibbs_argument_checks():
    from pgmpy_amd.sampling import GibbsSampling, State

    with pytest.raises(TypeError, match="Model expected type: DiscreteBayesianNetwork or DiscreteMarkovNetwork"):
        GibbsSampling(object())
    with pytest.raises(TypeError, match="Model expected type"):
        GibbsSampling()
    for m in (S.hand_model(), G.triangle_model()):
        g = GibbsSampling(m)
        full = {v: 0 for v in m.nodes()}
        with pytest.raises(ValueError, match="Evidence variable Z not in the model"):
            g.sample(size=2, evidence=[("Z", 0)])
        with pytest.raises(ValueError, match="Evidence variable Z not in the model"):
            g.sample_codes(4, 2, evidence=[State("Z", 0)])
        with pytest.raises(ValueError, match="start_state must cover every variable of the model; missing: \\['C'\\]"):
            g.sample(start_state={v: 0 for v in m.nodes() if v != "C"}, size=2)
        with pytest.raises(ValueError, match="start_state must cover every variable"):
            g.sample(start_state=[State("A", 0)], size=2)
        with pytest.raises(ValueError, match="start_state variable Z not in the model"):
            g.sample(start_state=dict(full, Z=0), size=2)
        with pytest.raises(ValueError, match="start_state of A must be a state number"):
            g.sample(start_state=dict(full, A=-1), size=2)
        with pytest.raises(ValueError, match="start_state must cover every variable"):
            next(g.generate_sample(start_state={"A": 0}, size=2))
        for bad in ({"size": 0}, {"thin": 0}, {"n_chains": 0}, {"size": -3}, {"thin": 1.5}):
            with pytest.raises(ValueError, match=f"{next(iter(bad))} must be a positive integer"):
                g.sample(**bad)
        with pytest.raises(ValueError, match="burn_in must be a non-negative integer"):
            g.sample(size=2, burn_in=-1)
        with pytest.raises(ValueError, match="size must be a positive integer"):
            next(g.generate_sample(size=0))
        with pytest.raises(ValueError, match="n_chains must be a positive integer"):
            g.sample_codes(0, 2)
        with pytest.raises(ValueError, match="must lie in 1 .. 2\\^32 - 1"):
            g.sample_codes(4, 2, first_sweep=0)
        with pytest.raises(ValueError, match="must lie in 1 .. 2\\^32 - 1"):
            g.sample_codes(4, 2, first_sweep=2 ** 32 - 1)
    with pytest.raises(KeyError, match="state: zz is an unknown for variable: D"):
        GibbsSampling(S.hand_model()).sample(size=2, evidence=[("D", "zz")])


def test_gibbs_without_gpu_raises_native_unavailable():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pgmpy_amd._native import NativeUnavailable
    from pgmpy_amd.sampling import GibbsSampling

    for m, ev in ((S.hand_model(), [("D", "d0")]), (G.triangle_model(), [("A", 0)])):
        g = GibbsSampling(m)
        start = {v: 0 for v in m.nodes()}
        for call in (lambda: g.sample(size=3, seed=1), lambda: g.sample(start_state=start, size=3, n_chains=2),
                     lambda: g.sample_codes(8, 2, seed=1), lambda: g.sample_codes(8, 2, seed=1, evidence=ev),
                     lambda: g.sample_codes(2, 1, start_codes=np.zeros((len(start), 2), dtype=np.uint8)),
                     lambda: list(g.generate_sample(size=2, seed=1))):
            with pytest.raises(NativeUnavailable):
                call()
