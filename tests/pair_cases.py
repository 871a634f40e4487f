"""Pairwise counts and tree learners: exact tables, the long-double restatement of the pair statistics and
edge weights, the error bounds of their comparison, and the fixtures of the tests.

``tables`` counts with np.bincount: the int64 block of every pair u < v (and stratum) under the per-pair
complete-case rule of include/pgmhip.h "pairwise counts".  ``pair_stats`` restates pgm_pair_mi and
pgm_pair_emi for one block in np.longdouble (log through numpy's long-double loop, lgamma through libm's
lgammal, tests/score_cases.py) and returns with every value the sum of |term| and the number of terms.

Bounds (u = 2^-53; U_LOG = 0.503 and U_LGAMMA = 1.538 are the recorded device figures of
tests/score_cases.py, doubled as there because real data reaches arguments the sample did not).

MI.  The kernel forms, per non-zero cell, q = fl(n / N), L = fl(fl(fl(log n + log N) - log a) - log b)
and adds fl(q L).  Write the exact value as the sum of the four sub-terms p log n, p log N, -p log a,
-p log b (p = n / N).  Each sub-term carries one log (U ulp), the ratio and the product: (U + 2) u
relative.  The three additions inside L cost at most 3 u times the cell's sub-terms in magnitude; adding
the cells in any order costs (cells - 1) u sum|t|.  All of it is below
    (n_terms - 1 + 2 U) u sum|t_i|   with n_terms = 4 cells + 3,
score_cases.bound's form (4 cells + 2 + 2 U >= cells - 1 + 3 + U + 2 for cells >= 1).  The int64 to fp64
conversions are exact below 2^53 and the clip at 0 moves the value towards the exact one.
H.  Two sub-terms per observed state (q log N, -q log a), one addition inside: n_terms = 2 states + 3.
EMI.  A term is (n / N) (log N - log a - log b + log n) exp(g), g the sum of nine lgamma values.  An
absolute error d in g is a relative error d in exp(g): d <= (2 U_LGAMMA + 8) u G with G the sum of the nine
|lgamma| (each value U ulp of itself, eight additions each below u G).  With m = (n / N) exp(g) (|log N| +
|log a| + |log b| + |log n|) >= |term|, a term's error is below m (d + (2 U_LOG + 8) u): the four logs, their
three additions, the ratio, exp (one ulp), two products.  The K terms are added in some order: (K - 1) u sum m.
NMI, AMI, TAN.  A quotient x / y with errors dx, dy is off by at most (dx + |x / y| dy) / (|y| - dy) + u
|x / y|; the mean of two entropies adds u of itself; a TAN weight sum_c p_c w_c adds sum_c p_c dw_c +
(strata + 2) u sum_c |p_c w_c|.  A value whose denominator is within its own error of 0 has no bound and is
left out; ``check_left_out`` holds a fixture to at most 1 % of such pairs.
Host.  The goldens come from scikit-learn: numpy's log (1 ulp assumed, glibc's documented bound) and
scipy's gammaln / C lgamma (score_cases.U_HOST), and scikit-learn zeroes MI terms below eps (eps per
cell added to the bound).
"""
import json
import os

import numpy as np

from tests import score_cases as S

LD = np.longdouble
U = 2.0 ** -53
U_LOG, U_LGAMMA = 0.503, S.U_DEVICE
U_HOST_LOG, U_HOST_LGAMMA = 1.0, S.U_HOST
EPS = float(np.finfo(np.float64).eps)
KINDS = ("mutual_info", "normalized_mutual_info", "adjusted_mutual_info")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MISSING = 255


# ---------------------------------------------------------------------- exact tables
def offsets(cards):
    return np.concatenate([[0], np.cumsum(cards)]).astype(np.int64)


def table(codes, cols, cards, u, v, stratum=None, c=0):
    """The exact [cards[u], cards[v]] int64 table of the pair of variables (u, v): rows with 255 in either
    column (or a stratum code other than c) left out.  Codes >= the cardinality must not occur."""
    x, y = codes[cols[u]].astype(np.int64), codes[cols[v]].astype(np.int64)
    keep = (x != MISSING) & (y != MISSING)
    if stratum is not None:
        keep &= codes[stratum] == c
    return np.bincount(x[keep] * cards[v] + y[keep], minlength=cards[u] * cards[v]).reshape(cards[u], cards[v])


def tables(codes, cols, cards, stratum=None, n_strata=1):
    """{(c, u, v): table} for every stratum c and pair u < v."""
    n = len(cols)
    return {(c, u, v): table(codes, cols, cards, u, v, stratum, c)
            for c in range(n_strata) for u in range(n) for v in range(u + 1, n)}


def blocks_of(counts, cards, Sp):
    """{(c, u, v): block} of a downloaded count tensor [n_strata, Sp, Sp]."""
    off = offsets(cards)
    counts = np.asarray(counts).reshape(-1, Sp, Sp)
    n = len(cards)
    return {(c, u, v): counts[c, off[u]:off[u] + cards[u], off[v]:off[v] + cards[v]]
            for c in range(counts.shape[0]) for u in range(n) for v in range(u + 1, n)}


# ---------------------------------------------------------------------- the long-double restatement
_LG = {}


def _lgamma_table(N):
    """lgammal(k + 1) for k = 0 .. N (every argument of the EMI is such an integer)."""
    if N not in _LG:
        _LG[N] = S.lgammal(np.arange(N + 1, dtype=np.float64) + 1.0)
    return _LG[N]


def pair_stats(t, want_emi=False):
    """dict of one int64 table: N, and per statistic (value LD, sum of |term| LD, terms) under 'mi', 'hu',
    'hv' and with want_emi 'emi' (value, bound-ready magnitudes: see emi_bound)."""
    t = np.asarray(t, dtype=np.int64)
    N = int(t.sum())
    zero = (LD(0), LD(0), 0)
    if N == 0:
        return {"N": 0, "mi": zero, "hu": zero, "hv": zero, "emi": (LD(0), LD(0), LD(0), 0), "nu": 0, "nv": 0}
    a, b = t.sum(axis=1), t.sum(axis=0)
    logN = S.logl(N)
    with np.errstate(divide="ignore"):
        la, lb = S.logl(np.maximum(a, 1)), S.logl(np.maximum(b, 1))
    nz = t > 0
    i, j = np.nonzero(nz)
    n = t[nz]
    p = n.astype(LD) / LD(N)
    sub = np.stack([p * S.logl(n), p * logN, -p * la[i], -p * lb[j]])
    mi = sub.sum(dtype=LD)
    out = {"N": N, "nu": int((a > 0).sum()), "nv": int((b > 0).sum()),
           "mi": (max(mi, LD(0)), np.abs(sub).sum(dtype=LD), 4 * int(nz.sum()) + 3)}
    for key, m, lm in (("hu", a, la), ("hv", b, lb)):
        k = m > 0
        q = m[k].astype(LD) / LD(N)
        sub = np.stack([q * logN, -q * lm[k]])
        out[key] = (sub.sum(dtype=LD), np.abs(sub).sum(dtype=LD), 2 * int(k.sum()) + 3)
    if want_emi:
        lg = _lgamma_table(N)
        total, err_g, mag, K = LD(0), LD(0), LD(0), 0
        for ii in np.nonzero(a > 0)[0]:
            for jj in np.nonzero(b > 0)[0]:
                ai, bj = int(a[ii]), int(b[jj])
                ns = np.arange(max(1, ai + bj - N), min(ai, bj) + 1)
                if ns.size == 0:
                    continue
                parts = [lg[ai], lg[bj], lg[N - ai], lg[N - bj], -lg[N] * np.ones(ns.size, dtype=LD), -lg[ns],
                         -lg[ai - ns], -lg[bj - ns], -lg[N - ai - bj + ns]]
                g = sum(parts[1:], parts[0] * np.ones(ns.size, dtype=LD))
                G = sum(np.abs(x) * np.ones(ns.size, dtype=LD) for x in parts)
                ln = S.logl(ns)
                w = (ns.astype(LD) / LD(N)) * np.exp(g)
                term = w * (logN - la[ii] - lb[jj] + ln)
                m = w * (abs(logN) + abs(la[ii]) + abs(lb[jj]) + np.abs(ln))
                total += term.sum(dtype=LD)
                err_g += (m * G).sum(dtype=LD)
                mag += m.sum(dtype=LD)
                K += ns.size
        out["emi"] = (total, err_g, mag, K)
    return out


def bound(stat, u_log=U_LOG):
    """The bound of an 'mi' / 'hu' / 'hv' entry of pair_stats."""
    return float(S.bound(stat[2], stat[1], u_log))


def emi_bound(emi, u_log=U_LOG, u_lgamma=U_LGAMMA):
    _, err_g, mag, K = emi
    return float((2 * u_lgamma + 8) * U * err_g + (max(K - 1, 0) + 2 * u_log + 8) * U * mag)


def _quotient(x, dx, y, dy):
    """(x / y, its bound) or (None, None) when y is within dy of 0."""
    if abs(y) <= 2 * dy or y == 0:
        return None, None
    q = x / y
    return q, (dx + abs(q) * dy) / (abs(y) - dy) + U * abs(q)


def weight(kind, st, device=True):
    """(weight fp64, bound) of one table's statistics under scikit-learn's special cases; (None, None) when a
    denominator is within its bound of 0.  device: the device's figures, else the host's (the goldens)."""
    ul, ug = (U_LOG, U_LGAMMA) if device else (U_HOST_LOG, U_HOST_LGAMMA)
    if st["N"] == 0:
        return 0.0, 0.0
    one_u, one_v = st["nu"] == 1, st["nv"] == 1
    mi, dmi = (0.0, 0.0) if one_u or one_v else (float(st["mi"][0]), bound(st["mi"], ul))
    if not device:
        dmi += EPS * st["mi"][2]
    if kind == "mutual_info":
        return mi, dmi
    if one_u and one_v:
        return 1.0, 0.0
    hu, hv = float(st["hu"][0]), float(st["hv"][0])
    mean = 0.5 * (hu + hv)
    dmean = 0.5 * (bound(st["hu"], ul) + bound(st["hv"], ul)) + U * mean
    if kind == "normalized_mutual_info":
        if one_u or one_v:
            return 0.0, 0.0
        if mi <= dmi:  # scikit-learn returns exactly 0 at mi == 0: no bound across that step
            return None, None
        return _quotient(mi, dmi, mean, dmean)
    if one_u or one_v:
        return 0.0, 0.0
    emi, demi = float(st["emi"][0]), emi_bound(st["emi"], ul, ug)
    num, den = mi - emi, mean - emi
    dnum, dden = dmi + demi + U * abs(num), dmean + demi + U * abs(den)
    if abs(num) <= dnum + EPS or abs(den) <= dden + EPS:  # the eps clamps of scikit-learn
        return None, None
    return _quotient(num, dnum, den, dden)


def weight_matrix(kind, codes, cols, cards, stratum=None, n_strata=1, device=True):
    """(W, B, left_out): the symmetric matrix of weights, of their bounds, and the pairs without a bound
    (NaN in both).  With a stratum: sum_c p_c w_c, p_c = N_c / sum_c N_c per pair, strata in state order."""
    n = len(cols)
    W, B, left = np.zeros((n, n)), np.zeros((n, n)), []
    want_emi = kind == "adjusted_mutual_info"
    for u in range(n):
        for v in range(u + 1, n):
            sts = [pair_stats(table(codes, cols, cards, u, v, stratum, c), want_emi) for c in range(n_strata)]
            ws = [weight(kind, st, device) for st in sts]
            if any(w[0] is None for w in ws):
                left.append((u, v))
                W[u, v] = W[v, u] = B[u, v] = B[v, u] = np.nan
                continue
            if stratum is None:
                W[u, v], B[u, v] = ws[0]
            else:
                total = sum(st["N"] for st in sts)
                ps = [st["N"] / total if total else 0.0 for st in sts]
                W[u, v] = sum(p * w[0] for p, w in zip(ps, ws))
                B[u, v] = sum(p * w[1] for p, w in zip(ps, ws)) + (n_strata + 2) * U * sum(abs(p * w[0]) for p, w in zip(ps, ws))
            W[v, u], B[v, u] = W[u, v], B[u, v]
    return W, B, left


def check_left_out(left, n_vars):
    assert len(left) <= 0.01 * n_vars * (n_vars - 1) / 2, f"{len(left)} pairs without a bound: {left[:5]}"


class HostScorer:
    """pairwise_mutual_information under the restatement (fp64 of the long-double values): the scorer the
    tree logic runs with on the CPU.  `frame` holds integer codes (255 or NaN-free), one column per variable."""

    def __init__(self, frame):
        self.frame = frame

    def pairwise_mutual_information(self, variables, given, kind):
        columns = list(self.frame.columns)
        codes, cards = encode(self.frame)
        cols = [columns.index(v) for v in variables]
        stratum = None if given is None else columns.index(given)
        W, _, left = weight_matrix(kind, codes, cols, [cards[c] for c in cols], stratum,
                                   1 if given is None else cards[stratum])
        assert not left, left
        return W


def encode(frame):
    """(codes [n_cols, n] uint8, cards) of a frame: each column's sorted distinct values become 0, 1, ..."""
    codes, cards = [], []
    for c in frame.columns:
        values, inv = np.unique(frame[c].to_numpy(), return_inverse=True)
        codes.append(inv.astype(np.uint8))
        cards.append(len(values))
    return np.stack(codes), cards


# ---------------------------------------------------------------------- fixtures
def golden():
    with open(os.path.join(GOLDEN, "pair_cases.json")) as f:
        return json.load(f)


def frames():
    """The frames of tests/golden/make_golden_pairs.py, rebuilt from the committed arrays."""
    import pandas as pd

    net5 = np.load(os.path.join(GOLDEN, "metrics_cases.npz"))["net5_codes1000"]
    alarm = np.load(os.path.join(GOLDEN, "fit_alarm.npz"))["codes"]
    f5 = pd.DataFrame(net5.T.astype(np.int64), columns=[f"v{j}" for j in range(net5.shape[0])])
    fa = pd.DataFrame(alarm.T.astype(np.int64), columns=[f"a{j:02d}" for j in range(alarm.shape[0])])
    const = f5.iloc[:200].copy()
    const["k"] = 0
    twins = f5.iloc[:200].copy()
    twins["t"] = twins["v1"]
    return {"net5": f5, "alarm": fa, "const": const, "twins": twins, "tworows": f5.iloc[:2, :3].copy()}


def dependent_codes(n_rows, cards, seed=0, missing=0.0):
    """[len(cards), n_rows] uint8 codes whose columns depend on each other, so every pair's table is
    asymmetric: column j is (x + noise_j) mod card_j of one hidden x.  `missing`: share of 255 cells."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 16, n_rows)
    codes = np.stack([((x >> (j % 5)) + (rng.random(n_rows) < 0.35) * rng.integers(0, k, n_rows) + j) % k
                      for j, k in enumerate(cards)]).astype(np.uint8)
    if missing:
        codes[rng.random(codes.shape) < missing] = MISSING
    return codes
