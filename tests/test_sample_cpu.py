"""Forward sampling without a GPU: the numpy restatement (stream, selection rule, statistics), the host
plan unit (tools/sample_plan_selftest.cpp over pgmpy_amd/csrc/pgmsample_plan.cpp, plain and with
ASan + UBSan), the argument checks of the pgm_sample_* entry points, the Python argument checks of
simulate / do / rejection_sample / partial_samples, and no compute without a device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

from tests import sample_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- the stream
@pytest.mark.parametrize("counter,key,want", S.KNOWN_ANSWERS, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    got = S.philox4x32_10(counter, key)
    assert tuple(int(x) for x in got) == want


def test_uniforms_are_53_bits_below_one():
    rows = np.arange(4096, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    for col in (0, 1, 2, 37, 1040):
        bits = S.uniform_bits(0xDEADBEEFCAFEF00D, rows, col)
        assert (bits < np.uint64(1) << np.uint64(53)).all()
        u = S.uniforms(0xDEADBEEFCAFEF00D, rows, col)
        assert ((u >= 0) & (u < 1)).all() and (u * 2.0 ** 53 == bits.astype(np.float64)).all()
        assert 0.45 < u.mean() < 0.55
    # the largest 53-bit integer maps below 1
    assert float(np.uint64((1 << 53) - 1)) * 2.0 ** -53 == 1 - 2.0 ** -53 < 1


def test_column_pairs_share_one_call():
    rows = np.array([0, 1, 12345, 2 ** 40 + 3], dtype=np.uint64)
    seed = 77
    for k in (0, 5, 520):
        x = S.philox4x32_10((rows & S.LO32, rows >> S.S32, np.full(4, k, np.uint64), np.zeros(4, np.uint64)),
                            (seed, 0))
        even, odd = S.uniform_bits(seed, rows, 2 * k), S.uniform_bits(seed, rows, 2 * k + 1)
        assert (even == ((x[0] << np.uint64(21)) | (x[1] >> np.uint64(11)))).all()
        assert (odd == ((x[2] << np.uint64(21)) | (x[3] >> np.uint64(11)))).all()
        assert (even != odd).all()


def test_row_high_word_is_the_second_counter_word():
    lo, hi = np.uint64(2 ** 32 - 1), np.uint64(2 ** 32)
    a = S.philox4x32_10((0xffffffff, 0, 3, 0), (9, 0))
    b = S.philox4x32_10((0, 1, 3, 0), (9, 0))
    assert int(S.uniform_bits(9, [lo], 6)[0]) == (int(a[0]) << 21) | (int(a[1]) >> 11)
    assert int(S.uniform_bits(9, [hi], 6)[0]) == (int(b[0]) << 21) | (int(b[1]) >> 11)
    assert S.uniform_bits(9, [lo], 6)[0] != S.uniform_bits(9, [hi], 6)[0]
    # the seed's high word is the second key word
    c = S.philox4x32_10((5, 0, 0, 0), (1, 2))
    assert int(S.uniform_bits((2 << 32) | 1, [5], 0)[0]) == (int(c[0]) << 21) | (int(c[1]) >> 11)


# ---------------------------------------------------------------------------- the selection rule
@pytest.mark.parametrize("name,p", S.BOUNDARY_COLUMNS, ids=[c[0] for c in S.BOUNDARY_COLUMNS])
def test_selection_rule_at_boundaries(name, p):
    """u at, just below and just above every boundary, 0 and 1 - 2^-53: the vectorised restatement picks
    what the rule spelled out in plain floats picks, and never a state of probability 0."""
    us = S.boundary_uniforms(p)
    n = len(us)
    explicit = us[None, :]
    codes, _, bad = S.sample_ref([([0], [len(p)])], [np.array(p).reshape(-1, 1)], n, explicit=explicit)
    want = [S.expected_state(p, u) for u in us]
    assert not bad and codes[0].tolist() == want
    assert all(p[s] > 0 for s in codes[0])
    assert codes[0][0] == next(s for s, x in enumerate(p) if x > 0)       # u = 0: the first state with mass
    assert codes[0][1] == max(s for s, x in enumerate(p) if x > 0)        # u = 1 - 2^-53: the last one


def test_selection_rule_known_cases():
    p = [0.25, 0.5, 0.25]
    pick = lambda u, q=p: S.expected_state(q, u)
    assert [pick(0.0), pick(np.nextafter(0.25, 0)), pick(0.25), pick(np.nextafter(0.25, 1))] == [0, 0, 1, 1]
    assert [pick(np.nextafter(0.75, 0)), pick(0.75), pick(1 - 2.0 ** -53)] == [1, 2, 2]
    assert [pick(u, [1.5, 0.75, 0.75]) for u in (0.0, np.nextafter(0.5, 0), 0.5, 0.75, 1 - 2.0 ** -53)] == [0, 0, 1, 2, 2]
    assert [pick(u, [0.5, 0.5, 0.0]) for u in (0.5, 1 - 2.0 ** -53)] == [1, 1]
    assert pick(0.999, [1.0]) == 0


def test_modes_in_the_restatement():
    """GIVEN takes the code, a given 255 is drawn, OBSERVED multiplies the weight, a bad code kills the row."""
    fams = [([0], [2]), ([1, 0], [3, 2])]
    tables = [np.array([[0.25], [0.75]]), np.array([[0.2, 0.5], [0.3, 0.25], [0.5, 0.25]])]
    n = 64
    free, _, _ = S.sample_ref(fams, tables, n, seed=3)
    given = np.full((2, n), 255, dtype=np.uint8)
    given[1, ::2] = 2
    got, w, bad = S.sample_ref(fams, tables, n, seed=3, given=given, modes=[S.FREE, S.OBSERVED], weights=True)
    assert not bad and (got[0] == free[0]).all() and (got[1, ::2] == 2).all() and (got[1, 1::2] == free[1, 1::2]).all()
    assert np.allclose(w[::2].astype(float), np.where(got[0, ::2] == 0, 0.5, 0.25)) and (w[1::2] == 1).all()
    given[0, 5] = 2
    got, w, bad = S.sample_ref(fams, tables, n, seed=3, given=given, modes=[S.GIVEN, S.OBSERVED], weights=True)
    assert bad and got[0, 5] == 2 and got[1, 5] == 255 and w[5] == 0 and (np.delete(got[1], 5) != 255).all()


# ---------------------------------------------------------------------------- statistics
N_STAT = 2 ** 18


@pytest.fixture(scope="module")
def hand():
    m = S.hand_model()
    nodes, order, fams, tables = S.model_plan(m)
    joint = S.joint_of(fams, tables, (2, 3, 2, 3))
    return m, nodes, order, fams, tables, joint


def test_restatement_is_statistically_right(hand):
    """N = 2^18 rows of the hand-made network, fixed seed: every one of the 36 joint cell counts within
    6 sqrt(N p (1 - p)) of N p (all p >= 0.002; a false alarm has probability < 1e-7)."""
    _, nodes, _, fams, tables, joint = hand
    assert nodes == ["A", "B", "C", "D"] and joint.size == 36 and joint.min() >= 0.002
    assert abs(joint.sum() - 1) < 1e-12
    codes, _, bad = S.sample_ref(fams, tables, N_STAT, seed=20261019)
    assert not bad
    worst = S.six_sigma_cells(codes, joint, N_STAT)
    print(f"worst cell deviation {worst:.2f} sigma")
    assert worst <= 6.0


def test_likelihood_weighting_is_statistically_right(hand):
    """P(A = a0 | D = d2) from N = 2^18 weighted rows: within 6 sigma of the enumerated posterior, sigma
    from the weighted variance of the ratio estimator, sum w^2 (x - mu)^2 / (sum w)^2."""
    _, nodes, order, fams, tables, joint = hand
    given = np.full((4, N_STAT), 255, dtype=np.uint8)
    given[3] = 2
    modes = [S.OBSERVED if v == "D" else S.FREE for v in order]
    codes, w, bad = S.sample_ref(fams, tables, N_STAT, seed=5, given=given, modes=modes, weights=True)
    assert not bad and (codes[3] == 2).all()
    w = w.astype(np.float64)
    x = (codes[0] == 0).astype(np.float64)
    est = (w * x).sum() / w.sum()
    exact = joint[0, :, :, 2].sum() / joint[:, :, :, 2].sum()
    sigma = np.sqrt((w ** 2 * (x - exact) ** 2).sum()) / w.sum()
    print(f"estimate {est:.6f} exact {exact:.6f} sigma {sigma:.2e}")
    assert abs(est - exact) <= 6 * sigma
    # the weights are p(d2 | c)
    assert set(np.round(w, 12)) <= {0.5, 0.2}


# ---------------------------------------------------------------------------- the host plan unit
def _build_selftest(tmp_path_factory, flags):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("sample_plan") / "sample_plan_selftest")
    csrc = os.path.join(ROOT, "pgmpy_amd", "csrc")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "include"), "-I", csrc,
                            os.path.join(ROOT, "tools", "sample_plan_selftest.cpp"),
                            os.path.join(csrc, "pgmsample_plan.cpp"), os.path.join(csrc, "pgmfit_plan.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    return _build_selftest(tmp_path_factory, [])


def test_sample_plan_selftest(selftest):
    run = subprocess.run([selftest], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "sample_plan_selftest ok" in run.stdout, run.stdout + run.stderr


def test_sample_plan_selftest_sanitized(tmp_path_factory):
    """The same stand-alone host program under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only)."""
    exe = _build_selftest(tmp_path_factory, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "sample_plan_selftest ok" in run.stdout, run.stdout + run.stderr


def test_host_stream_equals_restatement(selftest):
    """pgm_sample.h's sample_uniform (the code the kernel compiles) against the numpy restatement."""
    for seed, row, col in [(0, 0, 0), (0, 0, 1), (7, 5, 3), (2 ** 64 - 1, 2 ** 32 - 1, 1040), (12345, 2 ** 32, 36),
                           (0xDEADBEEFCAFEF00D, 2 ** 62 + 17, 2 ** 31 + 1)]:
        run = subprocess.run([selftest, "--uniform", str(seed), str(row), str(col)], capture_output=True, text=True,
                             timeout=120)
        assert run.returncode == 0, run.stderr
        assert int(run.stdout) == int(S.uniform_bits(seed, [row], col)[0]), (seed, row, col)


# ---------------------------------------------------------------------------- the library, no device
def _families(N, fams):
    arr = (N.FitFamily * len(fams))()
    for f, (cols, cards) in enumerate(fams):
        arr[f].n_vars = len(cols)
        for v, (c, k) in enumerate(zip(cols[:N.PGM_MAX_DIMS], cards[:N.PGM_MAX_DIMS])):
            arr[f].col[v], arr[f].card[v] = c, k
    return arr


REJECTED_PLANS = [
    ("node_twice", [([0], [2]), ([1, 0], [2, 2]), ([0, 1], [2, 2])], "column 0 is the node of families 0 and 2"),
    ("parent_later", [([1, 0], [2, 2]), ([0], [2])], "parent column 0 is not the node of an earlier family"),
    ("parent_nowhere", [([0], [2]), ([1, 5], [2, 2])], "parent column 5 is not the node of an earlier family"),
    ("parent_card", [([0], [3]), ([1, 0], [2, 2])], "parent column 0 cardinality 2, its own family 0 has 3"),
    ("no_vars", [([], [])], "has 0 variables (1 .. 32)"),
    ("33_vars", [(list(range(33)), [2] * 33)], "has 33 variables (1 .. 32)"),
    ("card_0", [([0], [0])], "cardinality 0 (1 .. 255)"),
    ("card_256", [([0], [256])], "cardinality 256 (1 .. 255)"),
    ("31_binary_parents", [([v], [2]) for v in range(31)] + [([31] + list(range(31)), [2] * 32)],
     "table exceeds 2^31 - 1 bins"),
]


@pytest.mark.parametrize("name,fams,msg", REJECTED_PLANS, ids=[r[0] for r in REJECTED_PLANS])
def test_plan_validation_through_the_library(name, fams, msg):
    from pgmpy_amd import _native as N

    lib = N.load_library()
    h = ctypes.c_void_p()
    assert lib.pgm_sample_plan_create(_families(N, fams), len(fams), ctypes.byref(h)) == N.PGM_EINVAL and not h.value
    assert msg in N.last_error()


def test_sample_entry_points_reject_bad_arguments_on_the_host():
    """pgm_sample_* validate every argument before any HIP call: PGM_EINVAL with no device present."""
    from pgmpy_amd import _native as N

    lib = N.load_library()
    h = ctypes.c_void_p()
    EINVAL = N.PGM_EINVAL
    good = [([0], [3]), ([2, 0], [2, 3])]
    assert lib.pgm_sample_plan_create(None, 1, ctypes.byref(h)) == EINVAL
    assert lib.pgm_sample_plan_create(_families(N, good), 2, None) == EINVAL
    assert lib.pgm_sample_plan_create(_families(N, good), 0, ctypes.byref(h)) == EINVAL
    assert lib.pgm_sample_plan_create(_families(N, good), 2, ctypes.byref(h)) == N.PGM_OK
    try:
        codes = np.full((3, 8), 7, dtype=np.uint8)
        values, cdf, w = np.zeros(9), np.zeros(9), np.zeros(8)
        pc, pv, pf, pw = (a.ctypes.data_as(ctypes.c_void_p) for a in (codes, values, cdf, w))
        fwd = lib.pgm_sample_forward
        assert fwd(None, pv, pf, None, pc, 3, 8, 0, 8, 0, 1, None, None, None) == EINVAL    # null plan
        assert fwd(h, pv, None, None, pc, 3, 8, 0, 8, 0, 1, None, None, None) == EINVAL     # null cdf
        assert fwd(h, pv, pf, None, None, 3, 8, 0, 8, 0, 1, None, None, None) == EINVAL     # null codes
        assert fwd(h, None, pf, None, pc, 3, 8, 0, 8, 0, 1, pw, None, None) == EINVAL       # weights without values
        assert fwd(h, pv, pf, None, pc, 3, 7, 0, 8, 0, 1, None, None, None) == EINVAL       # ld < n_rows
        assert fwd(h, pv, pf, None, pc, 3, 8, -1, 4, 0, 1, None, None, None) == EINVAL      # negative row0
        assert fwd(h, pv, pf, None, pc, 3, 8, 5, 4, 0, 1, None, None, None) == EINVAL       # the window leaves ld
        assert fwd(h, pv, pf, None, pc, 3, 8, 0, 8, -1, 1, None, None, None) == EINVAL      # negative first_row
        assert fwd(h, pv, pf, None, pc, 3, 8, 0, 8, 2 ** 63 - 4, 1, None, None, None) == EINVAL  # the stream ends
        assert fwd(h, pv, pf, None, pc, 2, 8, 0, 8, 0, 1, None, None, None) == EINVAL       # the plan writes column 2
        assert "codes has 2 columns" in N.last_error()
        modes = np.array([0, 3], dtype=np.uint8)
        assert fwd(h, pv, pf, modes.ctypes.data_as(ctypes.c_void_p), pc, 3, 8, 0, 8, 0, 1, None, None, None) == EINVAL
        assert "mode 3" in N.last_error()
        assert fwd(h, pv, pf, None, pc, 3, 8, 0, 0, 0, 1, None, None, None) == N.PGM_OK     # nothing to draw: no launch
        assert lib.pgm_sample_cdf(None, pv, pf, None) == EINVAL
        assert lib.pgm_sample_cdf(h, None, pf, None) == EINVAL
        assert lib.pgm_sample_cdf(h, pv, None, None) == EINVAL
        assert lib.pgm_sample_plan_info(None, None, 0, 0, None, None, None, None, None) == EINVAL
        assert (codes == 7).all() and not cdf.any()
    finally:
        assert lib.pgm_sample_plan_destroy(h) == N.PGM_OK
    assert lib.pgm_sample_plan_destroy(None) == N.PGM_OK
    assert ctypes.sizeof(N.SampleInfo) == 4 * 4 + 2 * 8 + 4 * 4


def test_plan_info_layout_and_path_choice():
    """pgm_sample_plan_info: the fit plan's layout, the launch geometry and the path a launch takes."""
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.sampling._sample import SamplePlan

    fams = [([3], [2]), ([0, 3], [3, 2]), ([2, 3], [4, 2]), ([1, 0, 2], [2, 3, 4])]
    plan = SamplePlan(fams)
    fit = FitPlan(fams)
    assert (plan.offsets, plan.sizes, plan.total_bins) == (fit.offsets, fit.sizes, fit.total_bins) == ([0, 2, 8, 16], [2, 6, 8, 24], 40)
    assert plan.info.n_families == 4 and plan.info.n_cols == 4 and plan.info.total_columns == 17
    assert plan.info.block == 256 and plan.info.rows_per_block == 1024 and plan.info.vec4 == 0
    for codes, ld, row0, vec4 in [(0x1000, 64, 0, 1), (0x1000, 64, 4, 1), (0x1004, 8, 4, 1), (0x1000, 64, 1, 0),
                                  (0x1000, 63, 0, 0), (0x1002, 64, 0, 0), (0x1001, 63, 3, 0), (None, 64, 0, 0)]:
        assert plan.launch_info(codes, ld, row0).vec4 == vec4, (codes, ld, row0)
    i = plan.launch_info(0x1000, 64, 0, weights=0x2000)
    assert (i.weighted, i.explicit_uniforms) == (1, 0)
    i = plan.launch_info(0x1000, 64, 0, uniforms=0x2000)
    assert (i.weighted, i.explicit_uniforms) == (0, 1)


def test_new_symbols_are_bound_and_the_abi_version_stays():
    from pgmpy_amd import _native as N

    for name in ("pgm_sample_plan_create", "pgm_sample_plan_destroy", "pgm_sample_plan_info", "pgm_sample_cdf",
                 "pgm_sample_forward"):
        assert name in N.EXPORTED and hasattr(N.load_library(), name)
    assert N.load_library().pgm_version() == 25


# ---------------------------------------------------------------------------- Python: errors first
def _latent_model():
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.models import DiscreteBayesianNetwork

    m = DiscreteBayesianNetwork([("L", "X")], latents={"L"})
    m.add_cpds(TabularCPD("L", 2, [[0.5], [0.5]]), TabularCPD("X", 2, [[0.9, 0.2], [0.1, 0.8]], ["L"], [2]))
    return m


def test_simulate_argument_checks():
    """The reference's validation (DiscreteBayesianNetwork.py:1553-1659), before the device is touched."""
    from pgmpy_amd.factors.discrete import TabularCPD

    m = S.hand_model()
    with pytest.raises(ValueError, match="Evidence state: zz for A doesn't exist"):
        m.simulate(5, evidence={"A": "zz"})
    with pytest.raises(ValueError, match="Do state: zz for B doesn't exist"):
        m.simulate(5, do={"B": "zz"})
    with pytest.raises(ValueError, match="Variable can't be in both do and evidence"):
        m.simulate(5, do={"A": "a0"}, evidence={"A": "a1"})
    with pytest.raises(ValueError, match="Evidence provided for variable which is not in the model"):
        m.simulate(5, virtual_evidence=[TabularCPD("Z", 2, [[0.5], [0.5]])])
    with pytest.raises(ValueError, match="Virtual evidence should be defined on individual variables"):
        m.simulate(5, virtual_evidence=[TabularCPD("A", 2, [[0.5, 0.5], [0.5, 0.5]], ["C"], [2])])
    with pytest.raises(ValueError, match="The number of states/cardinality for the evidence should be same"):
        m.simulate(5, virtual_intervention=[TabularCPD("A", 3, [[0.5], [0.25], [0.25]])])
    with pytest.raises(ValueError, match="missing_prob should be TabularCPD. Got <class 'dict'>"):
        m.simulate(5, missing_prob={})
    with pytest.raises(ValueError, match="missing_prob must be a list of TabularCPD objects. Got <class 'int'>"):
        m.simulate(5, missing_prob=[3])
    with pytest.raises(ValueError, match=r"Got A. TabularCPD variable should end with \* symbol"):
        m.simulate(5, missing_prob=TabularCPD("A", 2, [[0.5], [0.5]]))
    with pytest.raises(ValueError, match=r"Got Z\*. TabularCPD variable not in model nodes."):
        m.simulate(5, missing_prob=[TabularCPD("Z*", 2, [[0.5], [0.5]])])
    with pytest.raises(ValueError, match="Got cardinality of variable = 3"):
        m.simulate(5, missing_prob=TabularCPD("A*", 3, [[0.5], [0.25], [0.25]]))
    with pytest.raises(ValueError, match="TabularCPD evidence Q not in model nodes."):
        m.simulate(5, missing_prob=TabularCPD("A*", 2, [[0.5, 0.5], [0.5, 0.5]], ["Q"], [2]))
    with pytest.raises(ValueError, match="partial_samples must have 5 rows"):
        m.simulate(5, partial_samples=pd.DataFrame({"A": ["a0", "a1"]}))


def test_do_and_sampler_argument_checks():
    from pgmpy_amd.sampling import BayesianModelSampling, State

    m = S.hand_model()
    with pytest.raises(ValueError, match="Nodes not found in the model: {'Z'}"):
        m.do(["A", "Z"])
    with pytest.raises(ValueError, match="Nodes not found in the model"):
        m.do("Z", inplace=True)
    assert sorted(m.edges()) == [("A", "C"), ("B", "C"), ("C", "D")]
    with pytest.raises(TypeError, match="Model expected type: DiscreteBayesianNetwork"):
        BayesianModelSampling(object())
    s = BayesianModelSampling(m)
    assert State("A", "a0") == ("A", "a0") and State(var="A", state="a0").state == "a0"
    with pytest.raises(ValueError, match="partial_samples must have 3 rows"):
        s.forward_sample(3, partial_samples=pd.DataFrame({"A": ["a0"]}))
    with pytest.raises(ValueError, match="partial_samples has columns that are not nodes of the model"):
        s.forward_sample(1, partial_samples=pd.DataFrame({"Z": ["a0"]}))
    with pytest.raises(KeyError, match="state: zz is an unknown for variable: A"):
        s.rejection_sample(evidence=[State("A", "zz")], size=2)
    with pytest.raises(ValueError, match="Evidence variable Z not in the model"):
        s.rejection_sample(evidence=[State("Z", "a0")], size=2)
    with pytest.raises(KeyError, match="state: zz is an unknown for variable: D"):
        s.likelihood_weighted_sample(evidence=[("D", "zz")], size=2)
    with pytest.raises(ValueError, match="size and first_row must be non-negative"):
        s.forward_sample_codes(-1)
    with pytest.raises(ValueError, match="Node Z not in the model"):
        s.forward_sample_codes(4, partial_codes={"Z": 0})
    with pytest.raises(ValueError, match="a mode is given for A but no codes"):
        s.forward_sample_codes(4, modes={"A": 1})


def test_sampling_without_gpu_raises_native_unavailable():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pgmpy_amd._native import NativeUnavailable
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.sampling import BayesianModelSampling, State

    m = S.hand_model()
    s = BayesianModelSampling(m)
    for call in (lambda: s.forward_sample(4, seed=1), lambda: s.forward_sample_codes(4, seed=1),
                 lambda: s.likelihood_weighted_sample(evidence=[State("D", "d0")], size=4),
                 lambda: s.rejection_sample(evidence=[State("D", "d0")], size=4),
                 lambda: s.forward_sample(2, partial_samples=pd.DataFrame({"A": ["a0", "a1"]})),
                 lambda: m.simulate(4, seed=1), lambda: m.simulate(4, evidence={"A": "a0"}),
                 lambda: m.simulate(4, do={"C": "c0"}),
                 lambda: m.simulate(4, virtual_evidence=[TabularCPD("A", 2, [[0.8], [0.2]], state_names={"A": ["a0", "a1"]})]),
                 lambda: m.simulate(4, missing_prob=TabularCPD("A*", 2, [[0.5], [0.5]])),
                 lambda: _latent_model().simulate(3, include_latents=True)):
        with pytest.raises(NativeUnavailable):
            call()
