"""The statistic kernels on crafted device buffers at workload-scale arguments (tests/crafted_cases.py): the
chi-square p-value of k_fit_ci_finish and the Pearson p-value of the k_lgs kernels against mpmath at the device's
own argument, Gaussian and structure scores at counts up to 2^40, the CI statistic where R C is past 2^53, MI and
EMI where the sum starts at a + b - N, and k_fit_count's one rule for bad codes.  Every table is written by hand
into the buffer the kernel reads: no rows are counted."""
import math

import numpy as np
import pytest

from tests import ci_cases as C
from tests import crafted_cases as K
from tests import fit_cases as F
from tests import pair_cases as PC
from tests import score_cases as S

pytestmark = pytest.mark.gpu

# (lambda, Yates): the six named lambdas with the correction, Pearson and G without (tests/test_ci_gpu.py)
COMBOS = [(lam, True) for lam in C.LAMBDAS.values()] + [(1.0, False), (0.0, False)]


def _dev(a):
    from pgmpy_amd import engine as E

    return E.to_device_raw(np.ascontiguousarray(a))


def _host(t):
    from pgmpy_amd.inference.batch import download

    return download(t.contiguous())


def _fit_plan(families):
    from pgmpy_amd.estimators._fit import FitPlan

    return FitPlan(families)


def _citest(cases, lam, yates):
    fams, counts = K.families_of(cases)
    stat, dof, p = _fit_plan(fams).citest(_dev(counts), lam, yates=yates)
    return _host(stat), _host(dof), _host(p)


def _worst_p(cases, stat, dof, p):
    """The largest |p - Q(dof / 2, stat / 2)| / bound over the cases, Q by mpmath at the device's own stat and dof;
    asserts every one."""
    worst = (0.0, None)
    for i, c in enumerate(cases):
        want, tol = K.q_tol(int(dof[i]), float(stat[i]))
        err = abs(float(p[i]) - want)
        assert err <= tol, (c["cards"], c["target"], float(stat[i]), float(p[i]), want, tol)
        if tol and err / tol >= worst[0]:
            worst = (err / tol, (c["target"], float(stat[i]), float(p[i]), want, tol))
    return worst


# ---------------------------------------------------------------------------- the chi-square p-value
@pytest.mark.parametrize("dof", K.DOFS)
def test_chi2_p_value_is_mpmath_q_at_the_device_statistic(gpu, dof):
    """pgm_igamc as the device runs it (its lgamma, log and exp): p of k_fit_ci_finish against the 50-digit
    Q(dof / 2, stat / 2) at the device's OWN stat, so nothing of the statistic's slack enters, under
    crafted_cases.q_tol.  dof 2 x 2 strata at stat / dof = 0 .. 20 and a tail point with p below 1e-300; dof is
    exact and every achieved ratio is within 10 % of its target.
    Measured on an MI355X, 2026-10-21, worst error / bound per dof in the order of crafted_cases.DOFS: 0.27, 0.094,
    0.14, 0.093, 0.12, 0.070, 0.099, 0.15, 0.11, 0.12; largest relative errors 1.7e-12 at dof 5,000, 1.2e-11 at
    20,000, 3.3e-11 at 65,025, 5.6e-11 at 100,000 (DESIGN.md "CI tests", "Precision, measured")."""
    cases = K.chi2_cases(dof)
    stat, got_dof, p = _citest(cases, 1.0, False)
    for i, c in enumerate(cases):
        assert int(got_dof[i]) == dof
        assert abs(float(stat[i]) / dof - c["target"]) <= 0.1 * c["target"], (dof, c["target"], float(stat[i]))
    assert float(p[0]) == 1.0 and float(stat[0]) == 0.0
    worst = _worst_p(cases, stat, got_dof, p)
    print(f"device dof {dof}: worst error / bound {worst[0]:.3g} at (target, stat, p, mpmath, bound) {worst[1]}")


def test_chi2_p_value_of_the_general_path(gpu):
    """One [254, 254] stratum with every row and column occupied: dof = 253^2 through the general path.  Measured on
    an MI355X, 2026-10-21: worst error / bound 0.0092 (relative error 2.6e-12 at stat / dof = 1)."""
    cases = K.general_cases()
    stat, dof, p = _citest(cases, 1.0, False)
    for i, c in enumerate(cases):
        assert int(dof[i]) == 253 ** 2 and abs(float(stat[i]) / 253 ** 2 - c["target"]) <= 0.1 * c["target"]
        ref = C.ci_ref(c["table"], 1.0, False)
        assert C.same(stat[i], ref[0], C.bound(ref[4], ref[3]))
    worst = _worst_p(cases, stat, dof, p)
    print(f"device dof 64009 (general path): worst error / bound {worst[0]:.3g} at {worst[1]}")


# ---------------------------------------------------------------------------- the CI statistic at large counts
def test_ci_statistic_where_r_c_is_past_2_to_the_53(gpu):
    """Cells of 10^11: every R C (4 10^22 and more) is rounded before the division.  stat and dof against
    ci_cases.ci_ref under ci_cases.bound for every lambda, with and without Yates; p against mpmath at the device's
    own stat as above."""
    cases = K.large_ci_cases()
    worst = 0.0
    for lam, yates in COMBOS:
        stat, dof, p = _citest(cases, lam, yates)
        for i, (c, (s, d, _, mag, cells)) in enumerate(zip(cases, K.large_ci_reference(lam, yates))):
            key = (c["cards"], c["target"], lam, yates)
            assert int(dof[i]) == d == c["dof"], key
            b = C.bound(cells, mag)
            assert C.same(stat[i], s, b), (key, float(stat[i]), float(s), b)
        worst = max(worst, _worst_p(cases, stat, dof, p)[0])
    print(f"device, large counts: worst p error / bound {worst:.3g}")


# ---------------------------------------------------------------------------- k_fit_count: bad codes
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("ld_kind", ["odd", "mult4"])
@pytest.mark.parametrize("path", ["lds", "global"])
def test_a_bad_code_after_a_missing_one_is_index_error(gpu, path, ld_kind, where):
    """A row whose family holds MISSING in an earlier column and a code equal to the cardinality in a later one
    raises IndexError on every path: the one-row kernel (odd ld), four rows per lane (ld a multiple of 4) and the
    one-row tail of that launch (its last row), in LDS and in global tables.  The tables are the restatement's
    with the row skipped and the memory around them is untouched."""
    import torch

    fams, codes, n_rows, row = K.bad_code_case(path, ld_kind, where)
    plan = _fit_plan(fams)
    d_codes = _dev(codes)
    pad, sentinel = 1024, -0x0123456789ABCDEF
    buf = torch.full((plan.total_bins + 2 * pad,), sentinel, dtype=torch.int64, device=gpu)
    tables = buf[pad:pad + plan.total_bins]
    tables.zero_()
    with pytest.raises(IndexError):
        plan.count(d_codes, n_rows=n_rows, tables=tables)
    got = _host(buf)
    assert (got[:pad] == sentinel).all() and (got[pad + plan.total_bins:] == sentinel).all()
    assert np.array_equal(got[pad:pad + plan.total_bins], F.count_ref(codes, fams, n_rows=n_rows, bad="skip"))


# ---------------------------------------------------------------------------- MI and EMI
def _pair_stats_of(table):
    """(mi, hu, hv, n, emi) of one table written into the count tensor of a two-variable plan."""
    import torch

    from pgmpy_amd.estimators._pairs import PairPlan

    table = np.asarray(table, dtype=np.int64)
    plan = PairPlan([0, 1], list(table.shape))
    counts = torch.zeros((1, plan.Sp, plan.Sp), dtype=torch.int64, device="cuda")
    plan.block(counts, 0, 1).copy_(_dev(table))
    mi, hu, hv, n = (_host(t) for t in plan.mi(counts))
    return float(mi[0, 0]), float(hu[0, 0]), float(hv[0, 0]), int(n[0, 0]), float(_host(plan.emi(counts))[0, 0])


def _assert_pair(name, table):
    st = K.pair_reference(name)
    mi, hu, hv, n, emi = _pair_stats_of(table)
    assert n == st["N"]
    for key, got in (("mi", mi), ("hu", hu), ("hv", hv)):
        print(name, key, got, float(st[key][0]), PC.bound(st[key]))
        assert abs(got - float(st[key][0])) <= PC.bound(st[key]), (name, key)
    print(name, "emi", emi, float(st["emi"][0]), PC.emi_bound(st["emi"]))
    assert abs(emi - float(st["emi"][0])) <= PC.emi_bound(st["emi"]), (name, "emi")


@pytest.mark.parametrize("name", list(K.PAIR_TABLES))
def test_emi_where_the_sum_starts_at_a_plus_b_minus_n(gpu, name):
    """Small tables with a_i + b_j > N + 1 in a cell (k_pair_emi's shifted start, which no counted fixture reaches),
    with a_i + b_j - N exactly 1 and 2, and with a marginal equal to N: MI, both entropies and the EMI against
    pair_cases.pair_stats under its bounds.  tests/test_crafted_cpu.py shows that a sum started one step late lies
    outside them."""
    _assert_pair(name, K.PAIR_TABLES[name])


@pytest.mark.parametrize("name", ["scale", "scale_skewed"])
def test_pair_statistics_at_two_to_the_20_rows(gpu, name):
    """A 4 x 4 table of N = 2^20 (and a skewed one with a_0 + b_0 > N) under the same bounds.  At this N the bound
    of the EMI (3.2e-6) is of the size of the EMI itself (4.3e-6): it is taken from the sum of the terms'
    magnitudes, and the signed terms cancel.  So this is a guard on scale (the ranges of n, lgamma at 10^6), not on
    the last digits; the small tables above are the guard on those.  MI and the entropies keep 10 digits."""
    _assert_pair(name, K.scale_tables()[name])


# ---------------------------------------------------------------------------- the Pearson p-value
def test_pearson_p_value_is_mpmath_ibeta_at_crafted_moments(gpu):
    """pgm_ibeta_half as the device runs it, through pgm_lgs_pcorr on G = [[1, r, 0], [r, 1, 0], [0, 0, n]] with both
    job shapes (an intercept in K; the ones column as third target): coef carries the bits of r, rank counts the
    ones column, and p is lgs_cases.ibeta_half((n - 2) / 2, fl(r r)) within ibeta_rel p (+ 2 u where p > 0.1) for n up
    to 10^8 (a = 5 10^7; the counted cases stop at a = 127.5), |r| = 1, both sides of the switch of fractions, and
    NaN for n <= 2.  Measured on an MI355X, 2026-10-21, worst error / bound per n in the order of PEARSON_N: 0.13,
    0.088, 0.39, 0.28, 0.44, 0.78 (n = 10^6, t = 10, relative error 6.9e-12), 0.59 (n = 10^8, t = 10, relative error
    5.2e-10); the host build beside them in DESIGN.md "Gaussian structure learning"."""
    import torch

    from pgmpy_amd.models._lg import SchurJobs

    shapes = ((SchurJobs(2, [([2], [0, 1])]), True, 1), (SchurJobs(2, [([], [0, 1, 2])]), False, 0))
    shift = torch.zeros(2, dtype=torch.float64, device="cuda")
    worst = {}
    for n, r, tag in K.pearson_grid():
        want, tol = K.pearson_reference(n, r)
        G = _dev(K.pearson_G(n, r))
        for jobs, intercept, rank in shapes:
            coef, p, got_rank = (_host(t) for t in jobs.pcorr(G, shift, intercept=intercept))
            key = (n, tag, intercept)
            assert int(got_rank[0]) == rank, key
            if n <= 2:
                assert math.isnan(coef[0]) and math.isnan(p[0]), key
                continue
            assert np.float64(coef[0]).tobytes() == np.float64(r).tobytes(), key
            err = abs(float(p[0]) - want)
            assert err <= tol, (key, float(p[0]), want, tol)
            if tol and err / tol >= worst.get(n, (-1.0,))[0]:
                worst[n] = (err / tol, tag, err / want if want else 0.0)
    for n, w in worst.items():
        print(f"device n {n}: worst error / bound {w[0]:.3g} at {w[1]} (relative error {w[2]:.3g})")


# ---------------------------------------------------------------------------- Gaussian scores
@pytest.mark.parametrize("n", K.SCORE_N)
def test_gaussian_scores_at_large_n(gpu, n):
    """lgs_score_finish at n = 259, 10^6 and 10^8 in G[d][d] on a moment matrix whose Schur complements are exact: rss
    carries the exact bits, rank counts the ones column and the parents, and ll / bic / aic are the closed form by
    mpmath within 4 u (|llf| + n) + 2 u penalty, on 0, 1 and 2 parents."""
    import torch

    from pgmpy_amd.models._lg import SchurJobs

    jobs = SchurJobs(3, K.SCORE_JOBS)
    G, shift = _dev(K.score_G(n)), torch.zeros(3, dtype=torch.float64, device="cuda")
    for kind in ("ll", "bic", "aic"):
        score, rss, rank = (_host(t) for t in jobs.score(G, shift, kind))
        for parents in range(3):
            want, tol, want_rss = K.score_reference(n, parents, kind)
            key = (n, kind, parents)
            assert np.float64(rss[parents]).tobytes() == np.float64(want_rss).tobytes(), key
            assert int(rank[parents]) == parents + 1, key
            print(key, float(score[parents]), want, tol)
            assert abs(float(score[parents]) - want) <= tol, key


# ---------------------------------------------------------------------------- structure scores
def test_structure_scores_at_counts_up_to_2_to_the_40(gpu):
    """k_fit_score on tables with entries log-uniform up to 2^40, zeros, a family of 2^40 in every bin, a column with
    a single non-zero bin, empty columns, 129 columns (a chunk and a tail) and 254 states: LL, K2 and BDeu with and
    without SKIP_EMPTY against score_cases.score_ref under score_cases.bound at 2 x U_DEVICE_LARGE (the device's
    lgamma and log measured at these very arguments, tools/lgamma_ulp.hip --args: 1.355 ulp at lgamma(9), MI355X,
    2026-10-21; the largest error then was 0.073 of the bound), and the observed columns and states."""
    from pgmpy_amd import _native as N

    plan = _fit_plan(K.SCORE_FAMILIES)
    host = K.score_counts()
    counts = _dev(host)
    runs = [("ll", N.SCORE_LL, S.LL, None, None)]
    for kind in ("k2", "bdeu"):
        alpha, beta = K.score_params(kind)
        runs += [(kind, N.SCORE_BD, S.BD, alpha, beta),
                 (kind + "+skip", N.SCORE_BD | N.SCORE_SKIP_EMPTY, S.BD | S.SKIP_EMPTY, alpha, beta)]
    for name, dev_mode, ref_mode, alpha, beta in runs:
        args = () if alpha is None else (_dev(alpha), _dev(beta))
        scores, observed = plan.score(counts, dev_mode, *args, want_observed=True)
        scores, observed = _host(scores), _host(observed)
        want, mag, terms, want_obs = S.score_ref(host, K.SCORE_FAMILIES, ref_mode, alpha, beta)
        tol = S.bound(terms, mag, 2 * S.U_DEVICE_LARGE)
        err = np.abs(scores - want.astype(np.float64))
        print(name, "error / bound", (err / tol).tolist())
        assert np.array_equal(observed, want_obs), name
        assert (err <= tol).all(), (name, scores.tolist(), want.astype(np.float64).tolist(), tol.tolist())
    occupied = int((K.score_tables()[3].sum(axis=0) > 0).sum())  # of 129 columns; 7 and 128 are empty by construction
    assert observed.tolist()[2:] == [1, occupied, 4, 1] and occupied <= 127
    want_states = [int((t.sum(axis=1) > 0).sum()) for t in K.score_tables()]
    assert _host(plan.states_observed(counts)).tolist() == want_states and want_states[4:] == [3, 4]
