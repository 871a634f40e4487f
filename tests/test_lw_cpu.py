"""The likelihood-weighted posterior without a device: the exported symbols, the geometry
pgm_sample_posterior_info reports (K, LDS bytes, the 256 -> 128 -> 64 step-down and the refusal), every host
argument check of pgm_sample_posterior (they run before any HIP call, so they answer here on fake
addresses), the long-double restatement (tests/lw_cases.py) against the exact posteriors of oracle/ on
alarm, the integer scheme against the unquantised restatement, and the golden values recorded from the
reference's get_distribution / map_query (tests/golden/make_golden_approx.py) against the restatement's
plain counting."""
import ctypes
import functools
import json
import os
import re

import numpy as np
import pytest

from tests import lw_cases as LW
from tests import sample_cases as SC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL = -1
P = ctypes.c_void_p
A = 0x10000  # a fake, 8-byte aligned address


def _plans(sample=None, targets=None):
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.sampling._sample import SamplePlan

    return (SamplePlan(sample or [([1], [2]), ([0, 1], [3, 2])]), FitPlan(targets or [([0], [3]), ([1, 0], [2, 3])]))


def test_symbols_bound_and_version():
    from pgmpy_amd import _native as N

    for name in ("pgm_sample_posterior", "pgm_sample_posterior_info"):
        assert name in N.EXPORTED and hasattr(N.load_library(), name)
    assert N.load_library().pgm_version() == 25
    assert ctypes.sizeof(N.LwInfo) == 6 * 4 + 4 * 8
    assert (N.LW_CHUNK, N.LW_MAX_SAMPLES, N.LW_LDS_BUDGET) == (LW.CHUNK, 1 << 20, 160 * 1024)


def test_info_k_chunks_and_workgroups():
    sp, tp = _plans()
    for S, K, chunks in [(1, 52, 1), (2, 52, 1), (1024, 52, 1), (1025, 51, 2), (2048, 51, 2), (2051, 50, 3),
                         (4096, 50, 4), (1 << 20, 42, 1024)]:
        i = sp.posterior_info(tp, 7, S)
        assert (i.k, i.chunks_per_row, i.workgroups, i.chunk) == (K, chunks, 7 * chunks, LW.CHUNK), S
        assert K == LW.k_of(S)
        assert i.rows_per_launch == min(65536 // chunks, 65535)
        # 9 bins, 2 columns: everything fits the largest workgroup
        assert (i.block, i.lds_bytes, i.lds_budget, i.n_cols, i.total_bins) == (256, 8 * 9 + 2048 + 2 * 256, 163840, 2, 9)
    assert sp.posterior_info(tp, 0, 5).workgroups == 0


def test_info_block_steps_down_and_refuses():
    """LDS = 8 * total_bins + 2048 + n_cols * block against 163,840 bytes: 400 columns leave room for
    (163840 - 2048 - 400 * block) / 8 bins."""
    sp, _ = _plans(sample=[([i], [2]) for i in range(400)])
    from pgmpy_amd.estimators._fit import FitPlan

    def bins(n):  # n bins: families of two bins over column 0
        return FitPlan([([0], [2])] * (n // 2))

    edge = {b: (163840 - 2048 - 400 * b) // 8 for b in (256, 128, 64)}
    assert edge == {256: 7424, 128: 13824, 64: 17024}
    for n, block in [(2, 256), (7424, 256), (7426, 128), (13824, 128), (13826, 64), (17024, 64)]:
        i = sp.posterior_info(bins(n), 1, 100)
        assert (i.block, i.lds_bytes) == (block, 8 * n + 2048 + 400 * block), n
        assert i.lds_bytes <= i.lds_budget
    with pytest.raises(ValueError, match=r"17026 target bins.*400 code columns.*163840"):
        sp.posterior_info(bins(17026), 1, 100)
    # a forced size is not stepped down
    assert sp.posterior_info(bins(2), 1, 100, block=64).block == 64
    assert sp.posterior_info(bins(7426), 1, 100, block=128).block == 128
    with pytest.raises(ValueError, match=r"workgroup of 256, the budget is 163840"):
        sp.posterior_info(bins(7426), 1, 100, block=256)


def _posterior(sp, tp, **kw):
    from pgmpy_amd import _native as N

    a = dict(plan=sp._h, targets=tp._h, values=P(A), cdf=P(A), modes=None, evidence=P(A), n_cols=2, ld=16, row0=0,
             n_rows=4, n_samples=100, first_row=0, seed=1, block=0, acc=P(A), scale=P(A), post=P(A), log_evidence=P(A),
             ess=P(A))
    a.update(kw)
    modes = a["modes"]
    if modes is not None:
        modes = (ctypes.c_uint8 * len(modes))(*modes)
    return N.load_library().pgm_sample_posterior(
        a["plan"], a["targets"], a["values"], a["cdf"], modes, a["evidence"], a["n_cols"], a["ld"], a["row0"],
        a["n_rows"], a["n_samples"], a["first_row"], a["seed"], a["block"], a["acc"], a["scale"], a["post"],
        a["log_evidence"], a["ess"], None)


BAD_ARGUMENTS = [
    (dict(plan=None), "null plan"), (dict(targets=None), "null targets"), (dict(values=None), "null values"),
    (dict(cdf=None), "null cdf"), (dict(evidence=None), "null evidence"), (dict(acc=None), "null acc"),
    (dict(scale=None), "null scale"),
    (dict(values=P(A + 4)), "8-byte aligned"), (dict(cdf=P(A + 1)), "8-byte aligned"), (dict(acc=P(A + 4)), "8-byte aligned"),
    (dict(scale=P(A + 2)), "8-byte aligned"), (dict(post=P(A + 4)), "8-byte aligned"),
    (dict(log_evidence=P(A + 4)), "8-byte aligned"), (dict(ess=P(A + 4)), "8-byte aligned"),
    (dict(n_cols=1), r"the plan reads column 1, evidence has 1 columns"),
    (dict(n_rows=-1), r"n_rows -1"), (dict(row0=-1), r"row0 -1"),
    (dict(row0=14), r"rows \[14, 18\) outside ld 16"), (dict(n_rows=17), r"outside ld 16"),
    (dict(n_samples=0), r"n_samples 0 \(1 \.\. 1048576\)"), (dict(n_samples=(1 << 20) + 1), r"n_samples 1048577"),
    (dict(first_row=-1), r"stream rows \[-1"), (dict(first_row=2 ** 63 - 300), r"stream rows"),
    (dict(block=32), r"block 32"), (dict(block=512), r"block 512"), (dict(block=-64), r"block -64"),
    (dict(modes=[0, 3]), r"family 1 mode 3"),
]


@pytest.mark.parametrize("kwargs,message", BAD_ARGUMENTS, ids=[f"{list(k)[0]}-{i}" for i, (k, _) in enumerate(BAD_ARGUMENTS)])
def test_posterior_argument_checks_need_no_device(kwargs, message):
    """Every argument of pgm_sample_posterior is checked on the host before any HIP call: the fake addresses
    are never touched and the answer is PGM_EINVAL with a message, with or without a device."""
    from pgmpy_amd import _native as N

    sp, tp = _plans()
    assert _posterior(sp, tp, **kwargs) == EINVAL
    assert re.search(message, N.last_error()), N.last_error()


def test_posterior_target_checks_need_no_device():
    from pgmpy_amd import _native as N

    sp, _ = _plans()
    for targets, n_cols, message in [
            ([([2], [2])], 3, r"target 0 column 2 is the node of no family of the sample plan"),
            ([([0], [3]), ([1, 0], [2, 4])], 2, r"target 1 column 0 cardinality 4, the sample plan has 3"),
            ([([0], [3]), ([5], [2])], 2, r"the targets read column 5, evidence has 2 columns")]:
        _, tp = _plans(targets=targets)
        assert _posterior(sp, tp, n_cols=n_cols) == EINVAL
        assert re.search(message, N.last_error()), N.last_error()
    # no rows: nothing to launch, and no device is asked for
    _, tp = _plans()
    assert _posterior(sp, tp, n_rows=0) == 0


def test_info_argument_checks():
    from pgmpy_amd import _native as N

    sp, tp = _plans()
    L = N.load_library()
    info = N.LwInfo()
    for args, message in [((None, tp._h, 1, 1, 0, ctypes.byref(info)), "null plan"),
                          ((sp._h, None, 1, 1, 0, ctypes.byref(info)), "null targets"),
                          ((sp._h, tp._h, 1, 1, 0, None), "null info"),
                          ((sp._h, tp._h, -1, 1, 0, ctypes.byref(info)), "n_rows -1"),
                          ((sp._h, tp._h, 1, 1, 100, ctypes.byref(info)), "block 100")]:
        assert L.pgm_sample_posterior_info(*args) == EINVAL
        assert message in N.last_error(), N.last_error()


# ---------------------------------------------------------------------------- the restatement
ALARM_SEED = 3  # chosen here, on the CPU, so that all 8 rows pass the 6-sigma bound below
ALARM_S = 4096


@functools.lru_cache(maxsize=None)
def alarm_case():
    from pgmpy_amd.utils import get_example_model

    with open(os.path.join(GOLDEN, "alarm_predict.json")) as f:
        g = json.load(f)
    m = get_example_model("alarm")
    nodes, order, fams, tables = SC.model_plan(m)
    col = {v: i for i, v in enumerate(nodes)}
    rows = g["rows"][:8]
    ev = np.full((len(nodes), len(rows)), LW.MISSING, dtype=np.uint8)
    for r, row in enumerate(rows):
        for v, s in zip(g["columns"], row):
            ev[col[v], r] = list(m.states[v]).index(s)
    targets = [([col[v]], [len(m.states[v])]) for v in g["missing"]]
    return m, g, nodes, fams, tables, ev, targets


def test_restatement_matches_exact_posteriors_on_alarm():
    """The restatement's marginals on 8 golden alarm rows (34 observed columns, S = 4096) lie within
    6 sqrt(p (1 - p) / ESS) of oracle/'s exact posteriors, ESS from the restatement's own weights."""
    from oracle import ve as OVE
    from oracle.network import load_network

    m, g, nodes, fams, tables, ev, targets = alarm_case()
    net = load_network("alarm")
    modes = [LW.OBSERVED] * len(fams)
    got = LW.posterior_ref(fams, tables, modes, ev, targets, ALARM_S, seed=ALARM_SEED)
    worst = 0.0
    for r, row in enumerate(g["rows"][:8]):
        exact = OVE.query(net, g["missing"], dict(zip(g["columns"], row)), joint_out=False)
        p = np.concatenate([exact[v] for v in g["missing"]])
        ess = float(got[r]["ess"])
        assert ess > 50, (r, ess)
        bound = 6 * np.sqrt(p * (1 - p) / ess)
        err = np.abs(got[r]["post"].astype(np.float64) - p)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (r, err, bound)
    assert worst <= 1.0


def test_api_seed_leaves_no_near_tie():
    """The seed of the public-API case (tests/test_lw_gpu.py) is chosen here: under it no row's two largest
    joint cells lie within 1e-9 relative, so the MAP of every one of the 16 rows is compared."""
    m, g, nodes, fams, tables, keep, missing, ev = LW.alarm_api_case()
    cards = [len(m.states[v]) for v in missing]
    joint = LW.posterior_ref(fams, tables, [LW.OBSERVED] * len(fams), ev, [([nodes.index(v) for v in missing], cards)],
                             LW.API_S, seed=LW.API_SEED)
    for r in range(LW.API_ROWS):
        top = np.sort(joint[r]["post"].astype(np.float64))[-2:]
        assert top[1] - top[0] > 1e-9 * top[1], r


def test_integer_scheme_matches_the_unquantised_restatement():
    """acc_ref / sum q against posterior_ref at the derived tolerance, on the plan-order net; and the
    scheme's invariants: every family's bins add up to sum q, the largest sample adds exactly 2^K."""
    fams, tables, n_cols = LW.plan_order_net()
    ev = LW.PLAN_ORDER_EVIDENCE
    for S in (1, 65, LW.CHUNK + 1):
        ref = LW.posterior_ref(fams, tables, LW.PLAN_ORDER_MODES, ev, LW.PLAN_ORDER_TARGETS, S, seed=5)
        layout, total = LW.target_layout(LW.PLAN_ORDER_TARGETS)
        for r in range(ev.shape[1]):
            acc, M, sq, sq1, sq2 = LW.acc_ref(fams, tables, LW.PLAN_ORDER_MODES, ev[:, r], LW.PLAN_ORDER_TARGETS,
                                              ref[r]["codes"])
            for off, size in layout:
                assert int(acc[off:off + size].sum()) == sq
            assert sq >= 1 << LW.k_of(S) and sq <= S << LW.k_of(S)
            tol = LW.tolerance(S, LW.n_observed(fams, LW.PLAN_ORDER_MODES, ev[:, r]))
            post = acc.astype(np.longdouble) / np.longdouble(sq)
            assert np.abs(post - ref[r]["post"]).max() <= tol
            le = M + np.log(np.ldexp(float(sq), -LW.k_of(S)) / S)
            assert abs(le - float(ref[r]["log_evidence"])) <= tol * max(1.0, abs(float(ref[r]["log_evidence"])))
            assert abs(sq1 * sq1 / sq2 - float(ref[r]["ess"])) <= 1e-3 * float(ref[r]["ess"])


def test_restatement_zero_probability_and_bad_code():
    fams, tables, ev = LW.zero_net()
    targets = [([0], [2]), ([1], [2])]
    ref = LW.posterior_ref(fams, tables, [LW.OBSERVED, LW.OBSERVED], ev, targets, 64, seed=2)
    assert np.isnan(ref[0]["post"].astype(np.float64)).all() and ref[0]["log_evidence"] == -np.inf and ref[0]["ess"] == 0
    assert np.array_equal(ref[1]["post"].astype(np.float64), [0.0, 1.0, 0.0, 1.0])
    w = ref[1]["w"]
    assert set(np.unique(w.astype(np.float64))) == {0.0, 0.75}
    bad = ev.copy()
    bad[1, 1] = 2
    assert LW.posterior_ref(fams, tables, [LW.OBSERVED, LW.OBSERVED], bad, targets, 8)[1]["bad"]


# ---------------------------------------------------------------------------- the golden
def test_golden_distributions_are_plain_frequencies():
    """The reference's get_distribution on the recorded 500 rows is count / 500 (joint and per variable)
    and its map_query the lowest flat index of the joint's maximum: the semantics the device path keeps."""
    with open(os.path.join(GOLDEN, "approx_cases.json")) as f:
        g = json.load(f)
    with open(os.path.join(GOLDEN, "metrics_cases.json")) as f:
        meta = json.load(f)
    states = meta["states"]
    nodes = sorted(states)
    codes = np.load(os.path.join(GOLDEN, "metrics_cases.npz"))["net5_codes1000"][:, :g["n_rows"]]
    j = g["joint"]
    cols = [nodes.index(v) for v in j["variables"]]
    flat = np.ravel_multi_index(tuple(codes[c].astype(np.int64) for c in cols), j["cardinality"])
    want = np.bincount(flat, minlength=int(np.prod(j["cardinality"]))) / g["n_rows"]
    assert np.array_equal(np.asarray(j["values"]), want)
    idx = np.unravel_index(int(np.argmax(want)), j["cardinality"])
    assert g["map_joint"] == {v: states[v][k] for v, k in zip(j["variables"], idx)}
    for v, f in g["marginals"].items():
        assert np.array_equal(np.asarray(f["values"]), np.bincount(codes[nodes.index(v)], minlength=len(states[v])) / g["n_rows"])


def test_approx_inference_rejects_other_models():
    from pgmpy_amd.inference import ApproxInference
    from pgmpy_amd.models import DiscreteMarkovNetwork

    with pytest.raises(ValueError, match="model should either be a Bayesian Network or Dynamic Bayesian Network"):
        ApproxInference(DiscreteMarkovNetwork())
    with pytest.raises(ValueError, match="model should either be"):
        ApproxInference("alarm")


def test_predict_argument_errors_need_no_device():
    import pandas as pd

    from pgmpy_amd.inference import ApproxInference

    m = SC.hand_model()
    data = pd.DataFrame({"A": ["a0", "a1"], "B": ["b0", "b2"]})
    with pytest.raises(NotImplementedError):
        m.predict(data, algo=ApproxInference, stochastic=True)
    with pytest.raises(TypeError, match="Algorithm should be a valid pgmpy inference method"):
        m.predict(data, algo=dict)
    with pytest.raises(TypeError, match="unexpected arguments"):
        m.predict(data, algo=ApproxInference, samples=3)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_lw_plan_selftest(tmp_path, flags):
    """The geometry and the argument checks from C++, as a stand-alone host program
    (tools/lw_plan_selftest.cpp over the host units alone), plain and under AddressSanitizer +
    UndefinedBehaviorSanitizer."""
    import shutil
    import subprocess

    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "pgmpy_amd", "csrc")
    exe = str(tmp_path / "lw_plan_selftest")
    build = subprocess.run([cxx, "-std=c++17", "-g", *flags, "-I", os.path.join(root, "include"), "-I", csrc,
                            os.path.join(root, "tools", "lw_plan_selftest.cpp"), os.path.join(csrc, "pgmlw_plan.cpp"),
                            os.path.join(csrc, "pgmsample_plan.cpp"), os.path.join(csrc, "pgmfit_plan.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "lw_plan_selftest ok" in run.stdout, run.stdout + run.stderr
