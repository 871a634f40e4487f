"""The per-row log-probability on the device: pgm_fit_logprob on every path (K1-K3), pgm_fit_log_values
(K4), the public API (P1-P5).

The reference is tests/logp_cases.py's long-double restatement, which tests/test_logp_cpu.py pins to values
recorded from the reference.  A device row is compared with the long-double sum at
n_fam * 2^-52 * sum_f |log theta_f| (logp_cases' docstring: one ulp per device logarithm plus the running
sum), and with fp64 values the reference recorded at twice that.  The bound rests on the device logarithm
being within 1 ulp: test_log_values measures it over every table used here and asserts it.  Totals are
compared bit for bit with the fixed-order sum of the device's own rows.

One case of the issue cannot exist: a node with 31 BINARY parents (logp_cases.plan)."""
import functools
import json
import os

import numpy as np
import pandas as pd
import pytest

from tests import logp_cases as LC
from tests import sample_cases as S

pytestmark = pytest.mark.gpu

R = LC.ROWS_PER_BLOCK
ROW_COUNTS = [1, 3, 4, 5, R - 1, R, R + 1, 2 * R + 3]
SENTINEL = -7.25
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dev(a):
    from pgmpy_amd import engine as E

    return E.to_device_raw(np.ascontiguousarray(a))


def _host(t):
    from pgmpy_amd.inference.batch import download

    return download(t)


@functools.lru_cache(maxsize=None)
def device_plan(name):
    """(FitPlan, device log tables) of a named plan, built once."""
    from pgmpy_amd.estimators._fit import FitPlan

    fams, tables = LC.plan(name)
    plan = FitPlan(fams)
    return plan, plan.log_values(_dev(LC.flat_values(tables)))


@functools.lru_cache(maxsize=None)
def case(name, n=2 * R + 3):
    """(codes [n_cols, n], the restatement of them), computed once and left unchanged."""
    fams, tables = LC.plan(name)
    if name == "alarm":  # rows the model can produce: uniform codes would hit its zero cells in most rows
        codes = S.sample_ref(fams, tables, n, seed=29)[0]
    else:
        codes = LC.random_codes(fams, n, np.random.default_rng(29))
    ref = LC.restate(fams, tables, codes)
    for a in (codes,) + ref[:4]:
        a.flags.writeable = False
    return codes, ref


def run_device(name, codes, row0=0, ld=None, windows=None, expect_vec4=None, raises=None, want_total=True):
    """pgm_fit_logprob over a sentinel-filled logp [ld]: (rows of the window, total, n_skipped) of the last
    call.  Asserts that no entry outside [row0, row0 + n) was written.  windows: [(begin, end)] row ranges
    covered by one call each (default: one call)."""
    import torch

    plan, logv = device_plan(name)
    n_cols, n = codes.shape
    ld = row0 + n + 5 if ld is None else ld
    buf = np.full((n_cols, ld), 0xAB, dtype=np.uint8)  # a code that is no state anywhere
    buf[:, row0:row0 + n] = codes
    d_codes = _dev(buf)
    logp = torch.full((ld,), SENTINEL, dtype=torch.float64, device=d_codes.device)
    if expect_vec4 is not None:
        assert plan.logprob_info(d_codes.data_ptr(), ld, row0, n).vec4 == int(expect_vec4)
    total = skipped = err = None
    for a, b in (windows or [(0, n)]):
        try:
            _, total, skipped = plan.logprob(logv, d_codes, n_rows=b - a, row0=row0 + a, logp=logp, total=want_total)
        except IndexError as e:
            err = e
    assert (err is not None) == bool(raises), err
    out = _host(logp)
    outside = np.ones(ld, dtype=bool)
    outside[row0:row0 + n] = False
    assert (out[outside] == SENTINEL).all(), "entries outside the row window were written"
    return out[row0:row0 + n], (None if total is None else _host(total)[0]), skipped


def assert_rows(name, got, ref, factor=1):
    """Device rows against the restatement: the bound where the value is finite, exactly -inf / NaN elsewhere."""
    fams, _ = LC.plan(name)
    _, exact, mag, skipped, _ = ref
    assert np.array_equal(np.isnan(got), skipped)
    inf = ~skipped & np.isinf(exact.astype(np.float64))
    assert (got[inf] == -np.inf).all()
    fin = ~skipped & ~inf
    assert np.isfinite(got[fin]).all()
    err = np.abs(got[fin].astype(np.longdouble) - exact[fin])
    bound = factor * LC.row_bound(len(fams), mag[fin])
    if fin.any():
        print(f"{name}: worst row error / bound = {float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()):.3f}")
    assert (err <= bound).all()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


# ---------------------------------------------------------------------------- K1: per-row values
@pytest.mark.parametrize("row0", [0, 1], ids=["four_rows", "one_row"])
@pytest.mark.parametrize("name", LC.PLANS)
def test_plans_match_the_restatement(gpu, name, row0):
    """K1: every synthetic plan and alarm over 2 R + 3 rows (three workgroups, a tail of 3), on both paths."""
    codes, ref = case(name)
    got, total, skipped = run_device(name, codes, row0=row0, ld=(codes.shape[1] + row0 + 11) // 4 * 4, expect_vec4=row0 == 0)
    assert_rows(name, got, ref)
    assert skipped == 0
    assert same_bits(total, LC.total_fixed_order(got))
    if name == "zeros":
        assert np.isinf(got).any() and total == -np.inf
    else:
        assert np.isfinite(got).all()


@pytest.mark.parametrize("row0", [0, 1], ids=["four_rows", "one_row"])
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_alarm_row_counts(gpu, n, row0):
    """K1: alarm at every row count around the workgroup size, the first n rows of one shared case."""
    codes, ref = case("alarm")
    got, total, skipped = run_device("alarm", codes[:, :n], row0=row0, ld=(n + row0 + 11) // 4 * 4, expect_vec4=row0 == 0)
    assert_rows("alarm", got, tuple(r[:n] if isinstance(r, np.ndarray) else r for r in ref))
    assert skipped == 0 and same_bits(total, LC.total_fixed_order(got))


# ---------------------------------------------------------------------------- K2: exactness
@pytest.mark.parametrize("name", ["alarm", "chain_300", "zeros"])
def test_bits_do_not_depend_on_the_path_or_the_split(gpu, name):
    """K2: a row's bits are the same on the four-rows and the one-row path, in one call and split over two
    calls (the second starting on a dword boundary or not), with another ld; the total's bits are the same
    on both paths and from run to run."""
    codes, _ = case(name)
    n = codes.shape[1]
    a, total_a, _ = run_device(name, codes, row0=0, ld=n + 5, expect_vec4=True)
    b, total_b, _ = run_device(name, codes, row0=1, ld=n + 6, expect_vec4=False)
    a2, total_a2, _ = run_device(name, codes, row0=4, ld=n + 9, expect_vec4=True)
    assert same_bits(a, b) and same_bits(a, a2)
    assert same_bits(total_a, total_b) and same_bits(total_a, total_a2)
    for k in (R, R + 6, 7):
        c, total_c, _ = run_device(name, codes, row0=0, ld=n + 5, windows=[(0, k), (k, n)])
        assert same_bits(a, c)
        assert same_bits(total_c, LC.total_fixed_order(a[k:]))  # the last call's window


# ---------------------------------------------------------------------------- K3: edge cases
def test_missing_codes_skip_the_row(gpu):
    """K3: 255 in a node column and in a parent column: those rows are NaN and counted, the total is the
    fixed-order sum of the others, the status is PGM_OK."""
    fams, _ = LC.plan("alarm")
    codes, ref = case("alarm")
    codes = codes.copy()
    node_col, parent_col = next(cols for cols, _ in fams if len(cols) >= 3)[:2]
    rows = {5: node_col, 6: parent_col, R + 1: node_col, 2 * R + 2: parent_col}
    for r, c in rows.items():
        codes[c, r] = LC.MISSING
    for row0 in (0, 1):
        got, total, skipped = run_device("alarm", codes, row0=row0)
        assert skipped == len(rows) and np.isnan(got[list(rows)]).all() and np.isnan(got).sum() == len(rows)
        keep = np.ones(codes.shape[1], dtype=bool)
        keep[list(rows)] = False
        assert_rows("alarm", got[keep], tuple(r[keep] if isinstance(r, np.ndarray) else r for r in ref))
        assert same_bits(total, LC.total_fixed_order(got)) and np.isfinite(total)


def test_a_code_that_is_no_state_raises_index_error(gpu):
    """K3: a code equal to the cardinality never indexes a table: IndexError, the row NaN, the others right."""
    fams, _ = LC.plan("alarm")
    codes, ref = case("alarm")
    codes = codes.copy()
    cols, cards = fams[10]
    codes[cols[0], 9] = cards[0]
    codes[cols[-1], R + 2] = 200
    for row0 in (0, 1):
        got, _, _ = run_device("alarm", codes, row0=row0, raises=True)
        assert np.isnan(got[[9, R + 2]]).all() and np.isnan(got).sum() == 2
        keep = np.ones(codes.shape[1], dtype=bool)
        keep[[9, R + 2]] = False
        assert_rows("alarm", got[keep], tuple(r[keep] if isinstance(r, np.ndarray) else r for r in ref))


def test_zero_cell_is_minus_infinity(gpu):
    """K3: a row with a zero-probability cell is -inf, so is the total; no NaN, nothing skipped."""
    fams, tables = [([0], [2]), ([1, 0], [3, 2])], [np.array([[0.25], [0.75]]), np.array([[0.5, 0.0], [0.25, 1.0], [0.25, 0.0]])]
    from pgmpy_amd.estimators._fit import FitPlan

    plan = FitPlan(fams)
    logv = plan.log_values(_dev(LC.flat_values(tables)))
    codes = np.array([[0, 1, 1, 0, 1, 1, 0], [2, 1, 0, 0, 2, 1, 1]], dtype=np.uint8)
    _, exact, mag, _, _ = LC.restate(fams, tables, codes)
    fin = np.array([True, True, False, True, False, True, True])
    for row0 in (0, 1):
        buf = np.zeros((2, 12), dtype=np.uint8)
        buf[:, row0:row0 + 7] = codes
        logp, total, skipped = plan.logprob(logv, _dev(buf), n_rows=7, row0=row0, total=True)
        got = _host(logp)[row0:row0 + 7]
        assert (got[~fin] == -np.inf).all() and not np.isnan(got).any()
        assert (np.abs(got[fin].astype(np.longdouble) - exact[fin]) <= LC.row_bound(2, mag[fin])).all()
        assert _host(total)[0] == -np.inf and skipped == 0


def test_no_rows(gpu):
    import torch

    plan, logv = device_plan("single")
    codes = torch.zeros((1, 8), dtype=torch.uint8, device=logv.device)
    logp, total, skipped = plan.logprob(logv, codes, n_rows=0, row0=3, total=True)
    assert _host(total)[0] == 0.0 and skipped == 0 and np.isnan(_host(logp)).all()


def test_plan_stays_usable_after_score_and_ci_launches(gpu):
    """The log-probability stage is built beside the score and CI stages of one handle."""
    import torch

    from pgmpy_amd import _native as N
    from pgmpy_amd.estimators._fit import FitPlan

    fams, tables = LC.plan("zeros")
    codes, ref = case("zeros")
    plan = FitPlan(fams[1:])  # every family has two variables: a CI test each
    d_codes = _dev(codes)
    counts = plan.count(d_codes)
    plan.score(counts, N.SCORE_LL)
    plan.citest(counts, 1.0)
    logv = plan.log_values(_dev(LC.flat_values(tables[1:])))
    logp, total, skipped = plan.logprob(logv, d_codes, total=True)
    want = LC.restate(fams[1:], tables[1:], codes)
    got = _host(logp)
    fin = np.isfinite(want[0])
    assert np.array_equal(np.isfinite(got), fin) and skipped == 0
    assert (np.abs(got[fin].astype(np.longdouble) - want[1][fin]) <= LC.row_bound(2, want[2][fin])).all()
    plan.score(counts, N.SCORE_LL)
    assert same_bits(_host(plan.logprob(logv, d_codes, total=True)[1]), _host(total))


# ---------------------------------------------------------------------------- K4: log tables
def test_log_values(gpu):
    """K4: the device logarithm over every table of every plan used here against the long-double log: the
    measured worst error in ulps is printed and must be within 1 ulp, which the row bound rests on.
    0 gives -inf, in place works, a negative or NaN entry raises ValueError."""
    import torch

    worst = 0.0
    for name in LC.PLANS:
        fams, tables = LC.plan(name)
        plan, logv = device_plan(name)
        v = LC.flat_values(tables)
        got = _host(logv)
        zero = v == 0.0
        assert (got[zero] == -np.inf).all() and np.isfinite(got[~zero]).all()
        want = np.log(v[~zero].astype(np.longdouble))
        ulp = np.spacing(np.abs(want.astype(np.float64))).astype(np.longdouble)
        err = np.abs(got[~zero].astype(np.longdouble) - want) / ulp
        worst = max(worst, float(err.max()))
        inplace = _dev(v)
        assert plan.log_values(inplace, out=inplace) is inplace and same_bits(_host(inplace), got)
    print(f"device log: worst error {worst:.4f} ulp over the test tables")
    assert worst <= 1.0
    plan, _ = device_plan("zeros")
    v = LC.flat_values(LC.plan("zeros")[1])
    for poison in (-1e-300, np.nan, -np.inf):
        bad = v.copy()
        bad[7] = poison
        with pytest.raises(ValueError, match="negative or NaN"):
            plan.log_values(_dev(bad))
    with pytest.raises(ValueError, match="values must be a contiguous fp64 device tensor"):
        plan.log_values(torch.zeros(3, dtype=torch.float64, device="cuda"))


# ---------------------------------------------------------------------------- P: the public API
@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "metrics_cases.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "metrics_cases.npz"))


def _net5(meta, edges=None):
    from tests.test_logp_cpu import net5

    return net5(meta, edges)


def _frame(meta, codes, columns=None):
    from tests.test_logp_cpu import frame

    return frame(meta, codes, columns)


def _model_bounds(model, codes_sorted):
    """(fp64 restatement rows on the normalised tables, twice the row bound) for codes in sorted-node order."""
    _, _, fams, tables = S.model_plan(model)
    _, exact, mag, skipped, invalid = LC.restate(fams, LC.normalized(tables), codes_sorted)
    assert not skipped.any() and not invalid
    return exact, 2 * LC.row_bound(len(fams), mag)


def _score_bound(rows, bound):
    """Both sides add n rounded rows: the rows' own bounds, plus (n - 1) 2^-53 sum |row| for each summation."""
    return float(bound.sum()) + len(rows) * 2.0 ** -52 * float(np.abs(rows).sum())


def test_net5_matches_the_reference(gpu, golden):
    """P1: log_probability, score and log_likelihood_score against the values recorded from the reference,
    with a DataFrame whose columns are shuffled and with an array plus ordering."""
    from pgmpy_amd.metrics import BayesianModelProbability, log_likelihood_score

    meta, arrays = golden
    m = _net5(meta)
    codes = arrays["net5_codes200"]
    _, bound = _model_bounds(m, codes)
    want = arrays["net5_logp200"]
    bmp = BayesianModelProbability(m)
    shuffled = ["D", "A", "E", "C", "B"]
    df = _frame(meta, codes, shuffled)
    got = bmp.log_probability(df)
    assert got.shape == (200,) and got.dtype == np.float64
    assert (np.abs(got.astype(np.longdouble) - want) <= bound).all()
    got_array = bmp.log_probability(df.values, ordering=shuffled)
    assert same_bits(got, got_array)
    topo = bmp.topological_order
    assert same_bits(got, bmp.log_probability(df[topo].values))
    tol = _score_bound(want, bound)
    assert abs(bmp.score(df) - meta["score200"]) <= tol
    assert abs(bmp.score(df.values, ordering=shuffled) - meta["score200_array"]) <= tol
    assert abs(log_likelihood_score(m, df) - meta["loglik200"]) <= tol
    assert same_bits(bmp.score(df), LC.total_fixed_order(got))
    assert bmp.log_probability(df.iloc[:0]).shape == (0,) and bmp.score(df.iloc[:0]) == 0.0


def test_alarm_matches_the_reference(gpu, golden):
    """P1: the 1,000 alarm rows of fit_alarm.npz; alarm's HREKG and HRSAT columns sum to 0.9999999 in the
    file and are normalised as the reference normalises them."""
    from pgmpy_amd.metrics import BayesianModelProbability, log_likelihood_score
    from pgmpy_amd.utils import get_example_model

    meta, arrays = golden
    m = get_example_model("alarm")
    codes = np.load(os.path.join(GOLDEN, "fit_alarm.npz"))["codes"]
    nodes = sorted(m.nodes())
    df = S.frame_of(m, codes, nodes)
    _, bound = _model_bounds(m, codes)
    want = arrays["alarm_logp"]
    got = BayesianModelProbability(m).log_probability(df)
    assert (np.abs(got.astype(np.longdouble) - want) <= bound).all()
    assert abs(log_likelihood_score(m, df) - meta["alarm_loglik"]) <= _score_bound(want, bound)


def test_sample_fit_score_stays_on_the_device(gpu):
    """P2: forward_sample_codes -> fit -> log_probability_codes on alarm at 4,096 rows: the codes tensor goes
    in as it is (same storage, on the device), the CPDs fit left on the device are not downloaded, and the
    rows equal the DataFrame path's on the downloaded frame bit for bit.  P3: after another fit the cached
    log tables are rebuilt."""
    from pgmpy_amd.metrics import BayesianModelProbability
    from pgmpy_amd.models import DiscreteBayesianNetwork
    from pgmpy_amd.sampling import BayesianModelSampling, compiled
    from pgmpy_amd.utils import get_example_model

    truth = get_example_model("alarm")
    n = 4 * R
    codes, nodes = BayesianModelSampling(truth).forward_sample_codes(n, seed=11)
    assert codes.is_cuda and nodes == sorted(truth.nodes())
    data = S.frame_of(truth, _host(codes), nodes)
    learner = DiscreteBayesianNetwork(list(truth.edges()))
    learner.fit(data, state_names={v: list(truth.states[v]) for v in nodes})
    assert all(c._dev is not None for c in learner.cpds)
    bmp = BayesianModelProbability(learner)
    ptr, before = codes.data_ptr(), _host(codes).copy()
    on_device_only = [c._host is None for c in learner.cpds]
    assert any(on_device_only)
    logp, total = bmp.log_probability_codes(codes)
    assert logp.is_cuda and total.is_cuda and tuple(logp.shape) == (n,) and tuple(total.shape) == (1,)
    assert codes.data_ptr() == ptr and np.array_equal(_host(codes), before)
    assert [c._host is None for c in learner.cpds] == on_device_only and all(c._dev is not None for c in learner.cpds)
    got = _host(logp)
    assert same_bits(got, bmp.log_probability(data)) and same_bits(_host(total)[0], LC.total_fixed_order(got))
    exact, bound = _model_bounds(learner, before)
    assert (np.abs(got.astype(np.longdouble) - exact) <= bound / 2).all()
    # a window of the same buffer
    part, part_total = bmp.log_probability_codes(codes, n_rows=R + 3, row0=5)
    assert same_bits(_host(part)[5:R + 8], got[5:R + 8]) and np.isnan(_host(part)[:5]).all()
    assert same_bits(_host(part_total)[0], LC.total_fixed_order(got[5:R + 8]))
    # P3: new data, new CPDs, new log tables
    tables_before = compiled(learner)._logp[1]
    learner.fit(data.iloc[:500], state_names={v: list(truth.states[v]) for v in nodes})
    again = _host(bmp.log_probability_codes(codes)[0])
    assert compiled(learner)._logp[1] is not tables_before and not same_bits(again, got)
    exact, bound = _model_bounds(learner, before)
    fin = np.isfinite(exact.astype(np.float64))
    assert (np.abs(again[fin].astype(np.longdouble) - exact[fin]) <= bound[fin] / 2).all() and (again[~fin] == -np.inf).all()


def test_correlation_score_and_fisher_c_match_the_reference(gpu, golden):
    """P4: on the 1,000 net5 rows, for the true DAG and the DAG without two edges.  Labels are exact (the
    generator refused p-values within a factor of 2 of the level).  Fisher's p-value: the reference
    computes 1 - chi2.cdf, whose cancellation leaves an absolute error of a few 2^-53; the batched tests'
    p-values agree with scipy's to about 1e-12 relative, which C = -2 sum log p hands on: 1e-9 relative
    plus 4 * 2^-53 absolute."""
    from pgmpy_amd.estimators.CITests import chi_square
    from pgmpy_amd.metrics import correlation_score, fisher_c

    meta, arrays = golden
    df = _frame(meta, arrays["net5_codes1000"])
    for name, want in meta["dags"].items():
        dag = _net5(meta) if name == "true" else _net5(meta, want["edges"])
        summary = correlation_score(dag, df, test="chi_square", significance_level=meta["significance_level"], return_summary=True)
        by_pair = {frozenset((u, v)): (s, d) for u, v, s, d in zip(*(want["summary"][k] for k in ("var1", "var2", "stat_test", "d_connected")))}
        assert len(summary) == 10 and list(summary.columns) == ["var1", "var2", "stat_test", "d_connected"]
        for u, v, s, d in zip(summary["var1"], summary["var2"], summary["stat_test"], summary["d_connected"]):
            assert (bool(s), bool(d)) == by_pair[frozenset((u, v))], (name, u, v)
        assert correlation_score(dag, df, test=chi_square, significance_level=meta["significance_level"]) == pytest.approx(want["f1"], abs=1e-15)
        p, rmsea = fisher_c(dag, df, "chi_square", compute_rmsea=True, show_progress=False)
        print(name, p, want["fisher_p"], rmsea, want["fisher_rmsea"])
        assert abs(p - want["fisher_p"]) <= 1e-9 * want["fisher_p"] + 4 * 2.0 ** -53
        assert abs(rmsea - want["fisher_rmsea"]) <= 1e-9 * want["fisher_rmsea"]
        assert fisher_c(dag, df, chi_square, show_progress=False) == p


def test_value_errors_on_the_device_path(gpu, golden):
    """P5: a NaN cell raises ValueError naming the number of rows; a category that is no state raises
    KeyError; a model with latents raises ValueError."""
    from pgmpy_amd.metrics import BayesianModelProbability

    meta, arrays = golden
    m = _net5(meta)
    df = _frame(meta, arrays["net5_codes200"]).astype(object)
    holes = df.copy()
    holes.loc[3, "B"] = np.nan
    holes.loc[17, "E"] = np.nan
    holes.loc[17, "A"] = np.nan
    with pytest.raises(ValueError, match="2 rows have a missing value"):
        BayesianModelProbability(m).log_probability(holes)
    with pytest.raises(ValueError, match="2 rows have a missing value"):
        BayesianModelProbability(m).score(holes)
    unknown = df.copy()
    unknown.loc[0, "C"] = "c9"
    with pytest.raises(KeyError):
        BayesianModelProbability(m).log_probability(unknown)
    from tests.test_logp_cpu import _latent_model

    with pytest.raises(ValueError, match="without latent variables"):
        BayesianModelProbability(_latent_model())
