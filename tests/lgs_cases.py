"""Partial correlations and Gaussian family scores restated in np.longdouble FROM THE ROWS, independently of the
C++ (pgmpy_amd/csrc/pgmlgs.hip, pgm_ibeta.h) and of pgmpy_amd/models/_lg.py, the error bounds of the comparisons
and the fixtures the CPU and GPU tests share (tests/golden/lgs_cases.json + .npz, made by
tests/golden/make_golden_lgs.py from the reference).

A value matrix is an fp64 ndarray X[d, n] (column-major like the device's); a job is (K, T), positions 0 .. d with
d the ones column, as pgm_lgs_jobs_create takes them.  u = 2^-53.

Restatement.  The residual of a target on K comes from the rows: the normal equations are formed and solved in
long double (lg_cases.solve_ld, partial pivoting; K must not be collinear, a case with a twin column is restated
without the twin), the residual vector is x - Z'b row by row.  pearsonr centres the two residual vectors and
correlates them; the p-value is I_{1 - r^2}((n - 2) / 2, 1 / 2) by mpmath at 40 digits (its error is nil next to
every bound below).  A score is the SUM over the rows of the Gaussian log-density of the residual at sigma^2 =
rss / n, not the closed form; test_lgs_cpu checks that the two agree.

Bounds, from lg_cases.gram_bound on.  The device sees the rows only through the shifted Gram matrix G~ (entries
against the ones column included), whose entries carry |dG~_uv| <= gram_bound = (n + 2) u sum_k |a_k b_k|.
  1. The sub-block.  With an intercept in K, or K empty, the block is G~ itself.  Otherwise the device forms raw
     moments M_uv = G~_uv + c_u g~_v + c_v g~_u + n c_u c_v with four more roundings, each relative to a partial sum
     that is at most T_uv = |G~_uv| + |c_u g~_v| + |c_v g~_u| + n |c_u c_v|.  The shift is exact data, so dG~ and
     dg~ pass through: |dM_uv| <= gram_bound_uv + |c_u| gram_bound_v1 + |c_v| gram_bound_u1 + 4 u T_uv.  T_uv is
     where the raw-moment cancellation factor enters: for a column with |mean| = rho sd it is (1 + rho_u)(1 + rho_v)
     times the centred scale, so a result that is later centred again loses 1 + max |mean| / sd digits per factor.
     By Cauchy-Schwarz gram_bound_uv <= (n + 2) u sqrt(G~_uu G~_vv): scaled to unit diagonal this is the
     2 (n + 2) u per entry of lg_cases (the factor 2 covering the conversion), kept here entry by entry.
  2. The factorisation.  Cholesky in any order has the backward error |dM_uv| <= (m + 2) u sqrt(M_uu M_vv) (Higham,
     Accuracy and Stability, Thm 10.3 with |R'||R|_uv <= sqrt(a_uu a_vv)), m = |K| + |T|; the scaling to unit diagonal
     adds 3 u of the same form.  Both are added to dM.
  3. The Schur complement.  R = V' M V with V = [-W; I], W = M_KK^-1 M_KT (long double, from the rows), so to first
     order |dR| <= |V|' |dM| |V| entry by entry.  The neglected second-order terms are at most eps kappa / (1 - eps
     kappa) of that, eps = m max_uv |dM_uv| / sqrt(M_uu M_vv) and kappa the condition number of the unit-diagonal
     M_KK, RECORDED WITH THE CASE from the rows and not recomputed from a result; a case needs eps kappa < 0.1 and the
     bound is multiplied by 1 / (1 - eps kappa).
  4. pearsonr.  cov_ab = R_ab - R_a1 R_b1 / n (without an intercept; R itself with one):
         |dcov_ab| <= |dR_ab| + (|R_a1| |dR_b1| + |R_b1| |dR_a1|) / n + 3 u (|R_ab| + |R_a1 R_b1| / n),
     coef = cov_xy / sqrt(cov_xx cov_yy):  |dcoef| <= |dcov_xy| / sqrt(cov_xx cov_yy) + |coef| (|dcov_xx| / cov_xx +
     |dcov_yy| / cov_yy) / 2 + 4 u, and through dp / dcoef = -2 sign(r) (1 - r^2)^(a - 1) / B(a, 1/2), a = (n - 2) / 2,
     as ci_cases.p_bound does for the chi-square:  |dp| <= |dp / dcoef| |dcoef| + P_REL p (+ 2 u where p > 0.1: there
     the function returns 1 minus a fraction), the derivative taken at the end of [|r| - dcoef, |r| + dcoef] where it
     is largest.  P_REL is the relative error of pgm_ibeta_half itself, derived at ibeta_rel.
  5. Scores.  rss = R_vv; llf = -n/2 (log(2 pi rss / n) + 1):  |dllf| <= n |drss| / (2 rss) + 4 u (|llf| + n).  The
     penalties are exact up to 2 u of their size.
The bound is no blanket: every kernel case carries a NEGATIVE CONTROL, the restatement of the same job with one
conditioning column left out, which must lie OUTSIDE the bound of the true job (negative_control; checked on the CPU
for every case the GPU tests use).
"""
import json
import os

import numpy as np

from tests import lg_cases as LC

LD = np.longdouble
U = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RCOND = 1e-11
N_ROWS = 257
_CACHE = {}


def golden():
    if "json" not in _CACHE:
        with open(os.path.join(GOLDEN, "lgs_cases.json")) as f:
            _CACHE["json"] = json.load(f)
        _CACHE["npz"] = dict(np.load(os.path.join(GOLDEN, "lgs_cases.npz")))
    return _CACHE["json"], _CACHE["npz"]


def frame(name):
    import pandas as pd

    g, z = golden()
    return pd.DataFrame(z[f"{name}_frame"], columns=g["frames"][name]["columns"])


# ---------------------------------------------------------------------- the incomplete beta function
def ibeta_half(a, y):
    """I_{1 - y}(a, 1/2) as a float, from mpmath at 40 digits."""
    import mpmath as mp

    with mp.workdps(40):
        y = mp.mpf(float(y))
        return float(mp.betainc(mp.mpf(float(a)), mp.mpf(0.5), 0, 1 - y, regularized=True))


def ibeta_rel(a, y):
    """Relative error bound of pgm_ibeta_half(a, y) = p.  The prefactor: its exponent a log1p(-y) + log(y) / 2 + the
    lgamma part carries 4 u of each of its three terms (fused products included) and exp turns the absolute error of the
    exponent into a relative one.  The continued fraction: it stops at 2 u, its product of ~ sqrt(a) + 10 factors
    converges geometrically (16 u in all), and every coefficient is five products and a quotient of exact numbers
    and the argument, 8 u with the argument's own rounding; the argument multiplies every coefficient, so those
    roundings act like a relative change of 8 u in the argument itself and come back multiplied by S = |d log cf /
    d log argument|.  With front = (1 - y)^a sqrt(y) / B(a, 1/2) and x = 1 - y:
        x below (a + 1) / (a + 5/2):  p = front cf(x) / a,      S = |front / (y p) - a + x / (2 y)|
        otherwise:                    1 - p = 2 front cf'(y),   S' = |front / (x (1 - p)) - 1 / 2 + a y / x|,
    the second case's error being relative to 1 - p, hence (1 - p) / p times larger relative to p.  S reaches a few
    tenths of a where a y is of order 1: the function loses about log10(a) digits there (pgm_ibeta.h says so)."""
    from math import exp, lgamma, log, log1p

    a, y = float(a), float(y)
    x = 1.0 - y
    lg = abs(0.5 * log(a)) + 1.0 if a >= 32 else abs(lgamma(a + 0.5)) + abs(lgamma(a))
    front = exp(a * log1p(-y) + 0.5 * log(y) + lgamma(a + 0.5) - lgamma(a) - lgamma(0.5))
    p = ibeta_half(a, y)
    base = 32 + 4 * a * abs(log1p(-y)) + 2 * abs(log(y)) + 4 * lg
    if x < (a + 1.0) / (a + 2.5):
        return (base + 8 * abs(front / (y * p) - a + x / (2 * y))) * U
    import mpmath as mp

    with mp.workdps(40):
        q = float(mp.betainc(mp.mpf(0.5), mp.mpf(a), 0, mp.mpf(y), regularized=True))  # 1 - p without the subtraction
    return (base + 8 * abs(front / (x * q) - 0.5 + a * y / x)) * U * (q / p if p > 0 else 1.0)


def _lgamma(x):
    from math import lgamma

    return lgamma(x)


def pearson_p(r, n):
    return ibeta_half((n - 2) / 2.0, float(r) ** 2)


def dp_dcoef(r, n):
    """|dp / dcoef| = 2 (1 - r^2)^(a - 1) / B(a, 1/2) at a = (n - 2) / 2."""
    from math import exp, lgamma, log1p

    a = (n - 2) / 2.0
    r2 = min(float(r) ** 2, 1.0 - 1e-300)
    return 2.0 * exp((a - 1) * log1p(-r2) + lgamma(a + 0.5) - lgamma(a) - lgamma(0.5))


# ---------------------------------------------------------------------- the restatement, from the rows
def _rows(X, cols, shift=None):
    """The rows of positions `cols` (d: the ones column) as long double [len(cols), n], minus `shift` when given."""
    X = np.asarray(X, dtype=np.float64)
    d, n = X.shape
    Z = np.ones((len(cols), n), dtype=LD)
    for i, c in enumerate(cols):
        if c != d:
            Z[i] = X[c].astype(LD) - (LD(0) if shift is None else LD(shift[c]))
    return Z


def residuals(X, K, T):
    """Residual vectors [len(T), n] (long double) of the targets after least squares on the columns K."""
    Zt = _rows(X, T)
    if not len(K):
        return Zt
    Zk = _rows(X, K)
    A = Zk @ Zk.T
    out = np.empty_like(Zt)
    for i in range(len(T)):
        b = LC.solve_ld(A, Zk @ Zt[i])
        out[i] = Zt[i] - b @ Zk
    return out


def pcorr_ld(X, K, T):
    """(coef, p) of the job: T = (X, Y, d) without an intercept, (X, Y) with one (d in K).  The residuals are
    centred either way (with an intercept they are centred already)."""
    n = np.asarray(X).shape[1]
    rx, ry = residuals(X, K, T[:2])
    rx, ry = rx - rx.sum(dtype=LD) / n, ry - ry.sum(dtype=LD) / n
    coef = float((rx @ ry) / np.sqrt((rx @ rx) * (ry @ ry)))
    coef = max(-1.0, min(1.0, coef))
    return coef, (pearson_p(coef, n) if n > 2 else float("nan"))


def score_ld(X, K, T, kind):
    """(score, rss, llf by the closed form): the score from the SUMMED log-density of the residuals at rss / n."""
    from math import log

    n = np.asarray(X).shape[1]
    r = residuals(X, K, T[:1])[0]
    rss = r @ r
    s2 = rss / n
    ll = (-(LD(0.5)) * np.log(2 * LC.PI_LD * s2) - r * r / (2 * s2)).sum(dtype=LD)
    closed = -(LD(n) / 2) * (np.log(2 * LC.PI_LD * rss / n) + 1)
    df = len([c for c in K if c != np.asarray(X).shape[0]])
    pen = {"ll": 0.0, "bic": 0.5 * (df + 2) * log(n), "aic": float(df + 2)}[kind]
    return float(ll - pen), float(rss), float(closed)


# ---------------------------------------------------------------------- the bounds
def job_condition(X, shift, K):
    """kappa of the unit-diagonal conditioning block in the device's representation (raw moments when K has no ones
    column, the shifted columns otherwise); 1 for an empty K.  Recorded with a case when it is built."""
    d = np.asarray(X).shape[0]
    if not len(K):
        return 1.0
    Z = _rows(X, K, None if d not in K else shift).astype(np.float64)
    M = Z @ Z.T
    dg = np.sqrt(np.diag(M))
    w = np.linalg.eigvalsh(M / np.outer(dg, dg))
    return float(w[-1] / w[0])


def schur_bound(X, shift, K, T, kappa):
    """(R, dR) long double / fp64 [t, t]: the Schur complement in the device's representation and its bound (module
    docstring 1 - 3).  Raises AssertionError for a case whose eps kappa is not below 0.1."""
    X = np.asarray(X, dtype=np.float64)
    d, n = X.shape
    cols = list(K) + list(T)
    m, k = len(cols), len(K)
    raw = k > 0 and d not in K
    # the shifted Gram matrix and its |a||b| sums, as the device's Gram kernel forms them
    data = [c for c in cols if c != d]
    G, A = LC.gram_ld(X, data, [shift[c] for c in data])
    pos = {c: i for i, c in enumerate(data)}
    pos[d] = len(data)
    ix = [pos[c] for c in cols]
    Gs, dG = G[np.ix_(ix, ix)], LC.gram_bound(A, n)[np.ix_(ix, ix)]
    g1 = G[ix, len(data)]
    c = np.array([0.0 if (col == d or not raw) else shift[col] for col in cols], dtype=LD)
    M = Gs + np.outer(c, g1) + np.outer(g1, c) + n * np.outer(c, c)
    Tm = np.abs(Gs) + np.abs(np.outer(c, g1)) + np.abs(np.outer(g1, c)) + n * np.abs(np.outer(c, c))
    dg = np.sqrt(np.abs(np.diag(M)).astype(np.float64))
    dg1, ca = LC.gram_bound(A, n)[ix, len(data)], np.abs(c).astype(np.float64)
    dM = dG + np.outer(ca, dg1) + np.outer(dg1, ca) + (4 * U * Tm).astype(np.float64) * (1 if raw else 0) \
        + (m + 5) * U * np.outer(dg, dg)
    eps = m * float(np.max(dM / np.maximum(np.outer(dg, dg), 1e-300)))
    assert eps * kappa < 0.1, (eps, kappa)
    V = np.zeros((m, m - k), dtype=LD)
    V[k:] = np.eye(m - k, dtype=LD)
    if k:
        for j in range(m - k):
            V[:k, j] = -LC.solve_ld(M[:k, :k], M[:k, k + j])
    R = V.T @ M @ V
    dR = (np.abs(V).T.astype(np.float64) @ dM @ np.abs(V).astype(np.float64)) / (1 - eps * kappa)
    return R, dR


def pcorr_bound(X, shift, K, T, kappa):
    """(coef tolerance, p tolerance) of a pgm_lgs_pcorr job against pcorr_ld (module docstring 4)."""
    n = np.asarray(X).shape[1]
    R, dR = schur_bound(X, shift, K, T, kappa)
    R = R.astype(np.float64)
    if len(T) == 3:
        cov = R[:2, :2] - np.outer(R[:2, 2], R[:2, 2]) / n
        dcov = np.empty((2, 2))
        for a in range(2):
            for b in range(2):
                dcov[a, b] = (dR[a, b] + (abs(R[a, 2]) * dR[b, 2] + abs(R[b, 2]) * dR[a, 2]) / n
                              + 3 * U * (abs(R[a, b]) + abs(R[a, 2] * R[b, 2]) / n))
    else:
        cov, dcov = R, dR + 0.0
    s = np.sqrt(cov[0, 0] * cov[1, 1])
    coef = cov[0, 1] / s
    dcoef = dcov[0, 1] / s + abs(coef) * (dcov[0, 0] / cov[0, 0] + dcov[1, 1] / cov[1, 1]) / 2 + 4 * U
    lo = max(abs(coef) - dcoef, 0.0)  # |dp / dcoef| decreases with |r| for a > 1
    a = (n - 2) / 2.0
    slope = dp_dcoef(lo if a > 1 else min(abs(coef) + dcoef, 1.0), n)
    p = pearson_p(coef, n)
    return dcoef, slope * dcoef + ibeta_rel(a, min(coef * coef, 1.0)) * p + (2 * U if p > 0.1 else 0.0)


def score_bound(X, shift, K, T, kappa):
    """(score tolerance, rss tolerance) of a pgm_lgs_score job against score_ld (module docstring 5)."""
    from math import log

    n = np.asarray(X).shape[1]
    R, dR = schur_bound(X, shift, K, T, kappa)
    rss, drss = float(R[0, 0]), float(dR[0, 0])
    llf = -0.5 * n * (log(2 * np.pi * rss / n) + 1)
    return n * drss / (2 * rss) + 4 * U * (abs(llf) + n + (len(K) + 2) * log(n)), drss + 2 * U * rss


def negative_control(X, shift, K, T, kappa, kind=None):
    """For conditioning columns other than the ones column (all of up to three): the restatement WITHOUT it must lie outside the
    bound of the true job (a bound that lets a wrong conditioning set pass is a blanket).  Returns the smallest
    ratio |difference| / tolerance, which must exceed 1."""
    d = np.asarray(X).shape[0]
    worst = np.inf
    data = [z for z in K if z != d]
    for z in sorted({data[0], data[len(data) // 2], data[-1]}) if data else ():  # a large K: its first, middle and last
        Kz = [c for c in K if c != z]
        if kind is None:
            tol, _ = pcorr_bound(X, shift, K, T, kappa)
            diff = abs(pcorr_ld(X, Kz, T)[0] - pcorr_ld(X, K, T)[0])
        else:
            _, tol = score_bound(X, shift, K, T, kappa)
            diff = abs(score_ld(X, Kz, T, kind)[1] - score_ld(X, K, T, kind)[1])
        worst = min(worst, diff / tol)
    return worst


# ---------------------------------------------------------------------- kernel cases (n = 257, seeded)
def dense_data(d, seed, n=N_ROWS, shift_cols=(), rho=1e6):
    """X[d, n]: column j = sum of 0.5^(j - i) x_i over the earlier columns (every column depends on every other, so
    leaving any one out of a conditioning set changes the answer) plus unit noise; `shift_cols` get mean rho sd."""
    rng = np.random.default_rng(seed)
    X = np.zeros((d, n))
    for j in range(d):
        X[j] = rng.standard_normal(n)
        for i in range(max(0, j - 6), j):
            X[j] += 0.5 ** (j - i) * X[i] * (1 if (i + j) % 2 else -1)
        X[j] /= X[j].std()
    for j in shift_cols:
        X[j] += rho
    return np.ascontiguousarray(X)


def shift_of(X):
    return LC.colmean(X, list(range(np.asarray(X).shape[0])))


def pcorr_job(Z, x, y, d, intercept=False):
    return ([d] + list(Z), [x, y]) if intercept else (list(Z), [x, y, d])


def score_job(parents, v, d):
    return ([d] + list(parents), [v])


# The kernel cases the GPU tests run and the CPU tests check the negative controls of: (name, d, seed, shifted
# columns, job, score kind or None).  |K| covers 0, 1, 2, the last lane-path size 7, the first wave-path size 8 and
# the cap 64 (which needs d = 67: 64 conditioning columns and the targets, listed once each); targets 0 and d - 1;
# K with and without the ones column; a permuted K; a target 10^6 sd from 0 with and without an intercept.
def kernel_cases():
    if "cases" in _CACHE:
        return _CACHE["cases"]
    out = []

    def add(name, d, seed, job, kind=None, shifted=()):
        out.append({"name": name, "d": d, "seed": seed, "shifted": tuple(shifted), "K": job[0], "T": job[1], "kind": kind})

    add("d2-k0", 2, 21, pcorr_job([], 0, 1, 2))
    add("d2-k0-icpt", 2, 21, pcorr_job([], 1, 0, 2, True))
    for z in (1, 2, 7, 8):
        add(f"d17-k{z}", 17, 22, pcorr_job(range(1, 1 + z), 0, 16, 17))
        add(f"d17-k{z}-icpt", 17, 22, pcorr_job(range(1, 1 + z), 16, 0, 17, True))
    add("d17-k7-permuted", 17, 22, pcorr_job([5, 2, 7, 1, 4, 6, 3], 0, 16, 17))
    add("d37-k8-permuted", 37, 23, pcorr_job([30, 2, 17, 9, 4, 36, 3, 11], 0, 35, 37))
    add("d37-k9", 37, 23, pcorr_job(range(20, 29), 36, 0, 37))
    add("d67-k64", 67, 24, pcorr_job(range(1, 65), 0, 66, 67))
    add("d67-k64-icpt", 67, 24, pcorr_job(range(2, 65), 0, 66, 67, True))
    add("shifted-k2", 17, 25, pcorr_job([2, 3], 0, 16, 17), shifted=(0,))
    add("shifted-k2-icpt", 17, 25, pcorr_job([2, 3], 0, 16, 17, True), shifted=(0,))
    add("shifted-k8-icpt", 17, 25, pcorr_job(range(2, 10), 0, 16, 17, True), shifted=(0, 2, 3, 16))
    add("score-d1", 1, 26, score_job([], 0, 1), "ll")
    for p, kind in ((0, "bic"), (1, "ll"), (2, "aic"), (6, "bic"), (7, "aic"), (8, "ll")):
        add(f"score-d37-p{p}", 37, 23, score_job(range(1, 1 + p), 0, 37), kind)
        add(f"score-d37-p{p}-last", 37, 23, score_job(range(36 - p, 36), 36, 37), kind)
    for kind in ("ll", "bic", "aic"):
        add(f"score-full-indegree-{kind}", 17, 22, score_job(range(1, 17), 0, 17), kind)
    add("score-d67-p63", 67, 24, score_job(range(1, 64), 0, 67), "bic")
    for c in out:
        c["X"] = case_data(c["d"], c["seed"], c["shifted"])
        c["shift"] = shift_of(c["X"])
        c["kappa"] = job_condition(c["X"], c["shift"], c["K"])
    _CACHE["cases"] = out
    return out


def case_data(d, seed, shifted=()):
    key = ("X", d, seed, tuple(shifted))
    if key not in _CACHE:
        _CACHE[key] = dense_data(d, seed, shift_cols=shifted)
    return _CACHE[key]


def case_reference(c):
    """(first output, second output, tolerance of each) of a kernel case from the restatement; cached."""
    if "ref" not in c:
        if c["kind"] is None:
            c["ref"] = pcorr_ld(c["X"], c["K"], c["T"]) + pcorr_bound(c["X"], c["shift"], c["K"], c["T"], c["kappa"])
        else:
            s, rss, _ = score_ld(c["X"], c["K"], c["T"], c["kind"])
            c["ref"] = (s, rss) + score_bound(c["X"], c["shift"], c["K"], c["T"], c["kappa"])
    return c["ref"]
