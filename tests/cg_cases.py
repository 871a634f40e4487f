"""The conditional-Gaussian scores restated in np.longdouble from the definition (include/pgmhip.h "conditional-
Gaussian scores"): rows are grouped in plain numpy and every density comes from the rows of its group, not from
moments, so nothing here shares the kernels' algebra.  Data generators for tests/test_cg_cpu.py and
tests/test_cg_gpu.py."""
import numpy as np

LD = np.longdouble
LOG2PI = np.log(LD(2) * LD("3.14159265358979323846264338327950288"))
RCOND = 1e-11
MISSING = 255


def tol(want):
    """The loose end of the project's parity band (README "Parity")."""
    return 1e-9 * max(1.0, abs(float(want)))


def mp_of(m):
    return next(p for p in (1, 2, 4, 8) if p >= m + 1)


def cards_for(Q):
    """Cardinalities (each <= 255) whose product is at least Q and as close as two columns get."""
    return [] if Q == 1 else [Q] if Q <= 255 else [2, (Q + 1) // 2]


def data(seed, n, cards, m, ld=None, row0=0):
    """(codes uint8 [len(cards), ld], X fp64 [m, ld]): uniform states; standard-normal noise around group means of
    order 1 with coefficients of order 1 along the columns.  Cells outside [row0, row0 + n) hold what must not be
    read: a code that is no state would raise, a NaN would show."""
    rng = np.random.default_rng(seed)
    ld = row0 + n if ld is None else ld
    codes = np.full((len(cards), ld), 254, dtype=np.uint8)
    X = np.full((m, ld), np.nan)
    w = slice(row0, row0 + n)
    for d, k in enumerate(cards):
        codes[d, w] = rng.integers(0, k, n)
    for j in range(m):
        mean = sum(np.cos(1.0 + d + j + codes[d, w].astype(float)) for d in range(len(cards)))
        X[j, w] = mean + rng.standard_normal(n) + (0.7 * X[j - 1, w] if j else 0.0)
    return codes, X


def complete(codes, X):
    ok = np.ones(codes.shape[1] if codes.size else X.shape[1], dtype=bool)
    for row in codes:
        ok &= row != MISSING
    for row in X:
        ok &= ~np.isnan(row)
    return ok


def config(codes, cards):
    q = np.zeros(codes.shape[1], dtype=np.int64)
    for row, k in zip(codes, cards):
        q = q * k + row
    return q


def moments(codes, cards, X, shift):
    """(M [Q, mp, mp] long double, A the same sums of absolute products) of the complete rows."""
    m, mp, Q = X.shape[0], mp_of(X.shape[0]), int(np.prod(cards, dtype=np.int64))
    ok = complete(codes, X)
    q = config(codes[:, ok], cards)
    Z = np.zeros((mp, int(ok.sum())), dtype=LD)
    Z[0] = 1
    for j in range(m):
        Z[1 + j] = X[j, ok].astype(LD) - LD(shift[j])
    M, A = np.zeros((Q, mp, mp), dtype=LD), np.zeros((Q, mp, mp), dtype=LD)
    for g in np.unique(q):
        Zg = Z[:, q == g]
        M[g], A[g] = Zg @ Zg.T, np.abs(Zg) @ np.abs(Zg).T
    return M, A


def density(rows):
    """(L(g; cols), columns dropped or 0 under the fallback) of rows [n_g, k]."""
    rows = np.asarray(rows, dtype=LD)
    n, k = rows.shape
    if n == 0 or k == 0:
        return LD(0), 0
    c = rows - rows.mean(axis=0)
    c[:, np.ptp(rows, axis=0) == 0] = 0  # a constant column is exactly constant
    scatter = c.T @ c
    if n == 1 or n < k:
        return -LD(n) / 2 * k * LOG2PI - np.trace(scatter) / 2, 0
    S = scatter / (n - 1)
    d = np.diag(S).copy()
    s = np.array([1 / np.sqrt(x) if x > 0 else LD(0) for x in d], dtype=LD)
    R = S * np.outer(s, s)
    logdet, r = LD(0), 0
    for j in range(k):  # Cholesky in outer-product form, no pivoting; a pivot at or below RCOND drops its column
        p = R[j, j]
        if p > RCOND:
            r += 1
            logdet += np.log(d[j] * p)
            R[j + 1:, j + 1:] -= np.outer(R[j + 1:, j], R[j + 1:, j]) / p
    return -LD(n) / 2 * (r * LOG2PI + logdet) - LD(n - 1) * r / 2, k - r


def score(codes, cards, X, var_disc):
    """(ll, n_complete, n_observed, n_dropped) of one family: codes [n_disc, n] with the variable first when it is
    discrete, X [n_cont, n] with the variable last when it is continuous."""
    ok = complete(codes, X)
    codes, rows = codes[:, ok], X[:, ok].T.astype(LD)
    n = int(ok.sum())
    ll, dropped = LD(0), 0
    if not var_disc:
        h = config(codes, cards)
        groups = np.unique(h)
        for g in groups:
            sub = rows[h == g]
            (full, df), (lead, dl) = density(sub), density(sub[:, :-1])
            ll += full - lead
            k = sub.shape[1]
            dropped += dl if (len(sub) == 1 or len(sub) < k) else df
        return ll, n, len(groups), dropped
    g_all, h_all = config(codes, cards), config(codes[1:], cards[1:])
    for key, sign in ((g_all, 1), (h_all, -1)):
        for g in np.unique(key):
            sub = rows[key == g]
            L, dr = density(sub)
            ll += sign * (L + len(sub) * np.log(LD(len(sub)) / LD(n)))
            dropped += dr
    return ll, n, len(np.unique(h_all)), dropped


def mixed_network(n, seed=0):
    """A frame of the five-node network A -> X, B -> Y, X -> Z (A, B, Z discrete; X, Y continuous) and its edges."""
    import pandas as pd

    rng = np.random.default_rng(seed)
    A, B = rng.integers(0, 2, n), rng.integers(0, 3, n)
    X = 2.0 * A - 1.0 + rng.standard_normal(n)
    Y = 1.5 * (B - 1.0) + rng.standard_normal(n)
    Z = (X + 0.5 * rng.standard_normal(n) > 0).astype(int)
    df = pd.DataFrame({"A": pd.Categorical.from_codes(A, ["a0", "a1"]), "B": pd.Categorical.from_codes(B, ["b0", "b1", "b2"]),
                       "X": X, "Y": Y, "Z": pd.Categorical.from_codes(Z, ["z0", "z1"])})
    return df, [("A", "X"), ("B", "Y"), ("X", "Z")]
