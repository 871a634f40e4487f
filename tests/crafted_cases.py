"""Crafted inputs for the kernels that turn counts or moments into a statistic, at the arguments a workload of 10^6
rows and more produces: host-only builders, references and bounds shared by tests/test_crafted_cpu.py and
tests/test_crafted_gpu.py.

The kernels (k_fit_score, k_fit_ci_*, k_pair_mi, k_pair_emi, k_lgs_lane / k_lgs_wave) read a device buffer the
caller hands in, so a count table or a moment matrix written by hand costs kilobytes where the rows behind it would
cost gigabytes.  References: mpmath at 50 digits (gamma_q; lgs_cases.ibeta_half) and the long-double restatements
of the other case modules (ci_cases.ci_ref, score_cases.score_ref, pair_cases.pair_stats).  u = 2^-53.

The bound of Q(a, x) (q_tol), derived as lgs_cases.ibeta_rel is.  pgm_igamc forms the prefactor exp(a ln x - x -
lgamma a) in the log domain: every term of the exponent carries a few ulps of ITSELF (log and lgamma an ulp or two,
the product and the two subtractions one each: 4 u per term), and exp turns the exponent's absolute error into a
relative one: 4 E u with E = a |ln x| + x + |lgamma a|.  The series and the continued fraction stop below u and add
O(sqrt a) terms or factors that fall off geometrically: 32 u covers them and exp's own ulp.  So
    q_rel(a, x) = (32 + 4 E) u,
relative to Q on the fraction's branch (x >= a + 1) and relative to P = 1 - Q on the series' branch, where the
function returns 1 - P (there Q > 0.08, P / Q <= 11.5), plus the smallest normal fp64 absolutely: below it a value
is denormal or 0 and has no relative precision left.  E is where the digits go at a large dof: at a = 5 10^5 and
x = a the three terms are 6.6 10^6 each and cancel to -7.
"""
import functools
import math

import numpy as np

from tests import ci_cases as C
from tests import fit_cases as F
from tests import lgs_cases as G
from tests import pair_cases as PC
from tests import score_cases as S

LD = np.longdouble
U = 2.0 ** -53
TINY = float(np.finfo(np.float64).tiny)
DPS = 50


# ---------------------------------------------------------------------------- Q(a, x) by mpmath
def gamma_q(a, x):
    """(Q(a, x), P(a, x)) as mpmath numbers good to DPS digits: the series of P below a + 1, Lentz's continued fraction
    of Q above, both in mpmath arithmetic with 20 guard digits (the prefactor's exponent cancels up to 10^7 to
    O(10)).  mpmath's own gammainc gives up ("converges too slowly") from a of some 10^4 on; it is compared with
    this function where it still answers (tests/test_crafted_cpu.py)."""
    import mpmath as mp

    with mp.workdps(DPS + 20):
        a, x = mp.mpf(a), mp.mpf(x)
        if x <= 0:
            return mp.mpf(1), mp.mpf(0)
        lead = mp.exp(a * mp.log(x) - x - mp.loggamma(a))
        eps = mp.mpf(10) ** -(DPS + 10)
        if x < a + 1:
            term = 1 / a
            total, ap = term, a
            while True:
                ap += 1
                term *= x / ap
                total += term
                if term < total * eps:
                    break
            p = lead * total
            return 1 - p, p
        tiny = mp.mpf(10) ** -10000
        b = x + 1 - a
        c, d = 1 / tiny, 1 / b
        h = d
        i = 0
        while True:
            i += 1
            an = -i * (i - a)
            b += 2
            d = an * d + b
            d = tiny if d == 0 else d
            c = b + an / c
            c = tiny if c == 0 else c
            d = 1 / d
            delta = d * c
            h *= delta
            if abs(delta - 1) < eps:
                break
        q = lead * h
        return q, 1 - q


def q_rel(a, x):
    return (32.0 + 4.0 * (a * abs(math.log(x)) + x + abs(math.lgamma(a)))) * U


def q_tol(dof, stat):
    """(p, tolerance) of pgm_chi2_sf(stat, dof) = Q(dof / 2, stat / 2): the 50-digit value rounded to fp64 and the
    module docstring's bound.  stat <= 0 is 1 exactly."""
    a, x = 0.5 * float(dof), 0.5 * float(stat)
    if x <= 0:
        return 1.0, 0.0
    q, p = gamma_q(a, x)
    return float(q), q_rel(a, x) * float(p if x < a + 1 else q) + TINY


# ---------------------------------------------------------------------------- chi-square tables
M_SMALL, M_LARGE = 10 ** 6, 10 ** 11  # the cell scale: R C stays below 2^53 at the first, 4 10^22 at the second
Z_CARDS = {1: [], 2: [2], 3: [3], 10: [10], 100: [100], 1000: [250, 4], 5000: [250, 20], 20000: [250, 80],
           65025: [255, 255], 100000: [250, 200, 2]}
DOFS = tuple(Z_CARDS)
# stat / dof at which Q(dof / 2, stat / 2) lies between the smallest normal fp64 and 1e-300 (checked by the CPU test);
# the ratio 20 underflows to 0 from dof = 100 on
TAIL_RATIOS = {1: 1400.0, 2: 700.0, 3: 470.0, 10: 145.5, 100: 17.9, 1000: 3.71, 5000: 1.945}


def ratios(dof):
    return [0.0, 0.1, 0.5, 0.9, 1.0, 1.0 + 2.0 / math.sqrt(dof), 1.5, 2.0, 5.0, 20.0]


def strata_2x2(qz, delta, m):
    """[2, 2, qz] int64: every stratum [[m + delta, m - delta], [m - delta, m + delta]].  Its marginals are 2 m, every
    E is m, and without the Yates correction it adds 4 delta^2 / m to the Pearson statistic and 1 to dof."""
    t = np.empty((2, 2, qz), dtype=np.int64)
    t[0, 0] = t[1, 1] = m + delta
    t[0, 1] = t[1, 0] = m - delta
    return t


def chi2_cases(dof, m=M_SMALL, with_tail=True):
    """[{cards, table [2, 2, qz], dof, target, ratio}]: dof strata at every ratio of the grid (and the tail point)."""
    out = []
    for target in ratios(dof) + ([TAIL_RATIOS[dof]] if with_tail and dof in TAIL_RATIOS else []):
        delta = int(round(math.sqrt(target * m) / 2))
        out.append({"cards": [2, 2] + Z_CARDS[dof], "table": strata_2x2(dof, delta, m), "dof": dof, "target": target,
                    "ratio": 4.0 * delta * delta / m})
    return out


def general_cases(m=M_SMALL, targets=(0.5, 1.0, 2.0)):
    """The general path (rx + ry > ci_cases.SMALL): one [254, 254] stratum, m + delta (-1)^(x + y) in cell (x, y).
    Every row and column sums to 254 m, every E is m, the statistic is 254^2 delta^2 / m at dof 253^2."""
    sign = 1 - 2 * ((np.arange(254)[:, None] + np.arange(254)[None, :]) % 2)
    out = []
    for target in targets:
        delta = int(round(math.sqrt(target * m * 253 ** 2 / 254 ** 2)))
        out.append({"cards": [254, 254], "table": (m + delta * sign).astype(np.int64).reshape(254, 254, 1),
                    "dof": 253 ** 2, "target": target, "ratio": 254.0 ** 2 * delta * delta / m / 253 ** 2})
    return out


def families_of(cases):
    """(families, flat int64 counts) of a list of cases: every family reads columns of its own."""
    fams, col = [], 0
    for c in cases:
        fams.append((list(range(col, col + len(c["cards"]))), list(c["cards"])))
        col += len(c["cards"])
    return fams, np.concatenate([np.ascontiguousarray(c["table"]).ravel() for c in cases])


@functools.lru_cache(maxsize=None)
def large_ci_cases():
    """Tables at m = 10^11 per cell, where R C = 4 10^22 is past 2^53.  The 2 x 2 strata of chi2_cases, a small
    table with a chunk of strata and a tail ([3, 3, 130]) and a general-path one ([9, 8, 3]) whose cells are m plus
    noise of sd sqrt(m), so that stat / dof is of order 1."""
    rng = np.random.default_rng(511)
    out = []
    for dof, targets in ((1, (0.5, 1.0, 2.0)), (3, (0.5, 1.0, 2.0)), (100, (0.5, 1.0, 2.0)), (1000, (1.0,))):
        for c in chi2_cases(dof, M_LARGE, with_tail=False):
            if c["target"] in targets:
                out.append(c)
    for cards in ([3, 3, 130], [9, 8, 3]):
        t = M_LARGE + np.rint(rng.standard_normal(cards) * math.sqrt(M_LARGE)).astype(np.int64)
        out.append({"cards": cards, "table": t, "dof": (cards[0] - 1) * (cards[1] - 1) * cards[2], "target": None,
                    "ratio": None})
    return out


@functools.lru_cache(maxsize=None)
def large_ci_reference(lam, yates):
    """[(stat, dof, p, magnitude, cells)] of large_ci_cases by ci_cases.ci_ref, computed once."""
    return [C.ci_ref(c["table"], lam, yates, len(c["cards"]) > 2) for c in large_ci_cases()]


# ---------------------------------------------------------------------------- bad codes
def bad_code_case(path, ld_kind, where, rows_per_block=4096):
    """(families, codes [n_cols, ld], n_rows, the row) with one row whose family holds MISSING in an earlier column and a code
    equal to the cardinality in a later one that no other family reads.  ld_kind "odd": the one-row kernel;
    "mult4": four rows per lane, n_rows = ld - 1, so the last rows are the one-row tail of that launch."""
    rng = np.random.default_rng(71)
    ld = rows_per_block + (11 if ld_kind == "odd" else 12)
    n_rows = ld if ld_kind == "odd" else ld - 1
    if path == "lds":
        fams, first, later = F.MIXED, 4, 5  # the last family ([4, 5], [2, 6]) alone reads the columns 4 and 5
        codes = F._random_codes(rng, 6, ld, F._col_cards(fams, 6))
    else:
        fams, first, later = [([0, 1], [17, 241]), ([0], [17])], 0, 1  # 4,097 bins: past the LDS tile
        codes = F._random_codes(rng, 2, ld, [17, 241])
    row = 0 if where == "first" else n_rows - 1
    card = {c: k for cols, cards in fams for c, k in zip(cols, cards)}
    codes[first, row] = F.MISSING
    codes[later, row] = card[later]
    assert sum(later in cols for cols, _ in fams) == 1
    return fams, codes, n_rows, row


# ---------------------------------------------------------------------------- MI and EMI
PAIR_TABLES = {
    "t10": [[5, 3], [2, 0]],
    "t50": [[30, 2, 1], [3, 9, 0], [1, 0, 4]],
    "t1000": [[900, 50], [40, 10]],
    "marginal_is_N": [[7, 5], [0, 0]],   # a_0 = N: a_0 + b_j - N = b_j, one term per cell
    "shift_is_1": [[3, 3], [2, 2]],      # a_0 + b_0 - N = 6 + 5 - 10 = 1: the start the unshifted sum has too
    "shift_is_2": [[4, 2], [2, 2]],      # a_0 + b_0 - N = 6 + 6 - 10 = 2: the first shifted start
}
SCALE_N = 1 << 20


@functools.lru_cache(maxsize=None)
def scale_tables():
    """{name: [4, 4] int64}: one multinomial draw of N = 2^20 from a fixed dependent p, and a skewed p whose first row
    and column hold three quarters of the mass each, so that a_0 + b_0 > N."""
    rng = np.random.default_rng(2 ** 20)
    base = np.array([[8, 2, 1, 1], [2, 6, 2, 1], [1, 2, 5, 3], [1, 1, 3, 9]], dtype=np.float64)
    skew = np.array([[60, 6, 5, 4], [6, 2, 1, 1], [5, 1, 2, 1], [4, 1, 1, 1]], dtype=np.float64)
    out = {name: rng.multinomial(SCALE_N, (p / p.sum()).ravel()).reshape(4, 4).astype(np.int64)
           for name, p in (("scale", base), ("scale_skewed", skew))}
    t = out["scale_skewed"]
    assert t.sum(axis=1)[0] + t.sum(axis=0)[0] > SCALE_N
    return out


@functools.lru_cache(maxsize=None)
def pair_reference(name):
    """pair_cases.pair_stats (with the EMI) of a named table, computed once."""
    t = PAIR_TABLES[name] if name in PAIR_TABLES else scale_tables()[name]
    return PC.pair_stats(np.asarray(t, dtype=np.int64), want_emi=True)


def first_terms(t, least=2):
    """{(i, j): the EMI term at n = a_i + b_j - N} (long double) of every cell whose a_i + b_j - N is at least
    `least`: the term a sum started one step late leaves out."""
    t = np.asarray(t, dtype=np.int64)
    N = int(t.sum())
    a, b = t.sum(axis=1), t.sum(axis=0)
    lg = PC._lgamma_table(N)
    out = {}
    for i in np.nonzero(a > 0)[0]:
        for j in np.nonzero(b > 0)[0]:
            ai, bj = int(a[i]), int(b[j])
            n = ai + bj - N
            if n < least or n > min(ai, bj):
                continue
            g = lg[ai] + lg[bj] + lg[N - ai] + lg[N - bj] - lg[N] - lg[n] - lg[ai - n] - lg[bj - n] - lg[N - ai - bj + n]
            out[(int(i), int(j))] = (LD(n) / LD(N)) * np.exp(g) * (S.logl(N) - S.logl(ai) - S.logl(bj) + S.logl(n))
    return out


# ---------------------------------------------------------------------------- the Pearson p-value
PEARSON_N = (3, 4, 10, 259, 10 ** 4, 10 ** 6, 10 ** 8)
PEARSON_T = (0.0, 0.01, 0.5, 1.0, 2.0, 5.0, 10.0, 30.0)


def pearson_switch(n):
    """(r just below, r just above) the point where pgm_ibeta_half changes the fraction: x = 1 - r^2 against
    (a + 1) / (a + 2.5), a = (n - 2) / 2."""
    a = 0.5 * (n - 2.0)
    y = 1.5 / (a + 2.5)
    return math.sqrt(y * (1 + 1e-3)), math.sqrt(y * (1 - 1e-3))  # the larger r has the smaller x: the first branch


@functools.lru_cache(maxsize=None)
def pearson_grid():
    """[(n, r, tag)]: r = t / sqrt(t^2 + n - 2) over PEARSON_T (one of them negated), |r| = 1, both sides of the
    switch, and n = 2, 1 (no p-value)."""
    out = []
    for n in PEARSON_N:
        for t in PEARSON_T:
            r = t / math.sqrt(t * t + n - 2.0)
            out.append((n, -r if t == 2.0 else r, f"t={t:g}"))
        out += [(n, 1.0, "r=1"), (n, -1.0, "r=-1")]
        lo, hi = pearson_switch(n)
        out += [(n, lo, "below the switch"), (n, hi, "above the switch")]
    out += [(2, 0.5, "n=2"), (1, 0.5, "n=1")]
    return out


def pearson_G(n, r):
    """The moment matrix of two centred unit columns with correlation r over n rows, d = 2: [[1, r, 0], [r, 1, 0],
    [0, 0, n]].  Every elimination step of either job shape multiplies by an exact 0 or 1."""
    return np.array([[1.0, r, 0.0], [r, 1.0, 0.0], [0.0, 0.0, float(n)]], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def pearson_reference(n, r):
    """(p, tolerance) of pgm_pearson_p(r, n): lgs_cases.ibeta_half at fl(r r) and ibeta_rel p (+ 2 u where p > 0.1),
    the rule of lgs_cases.pcorr_bound; the ends y = 0 and y = 1 are exact."""
    if n <= 2:
        return float("nan"), 0.0
    a, y = 0.5 * (n - 2.0), r * r
    if y == 0.0 or y == 1.0:
        return 1.0 - y, 0.0
    p = G.ibeta_half(a, y)
    return p, G.ibeta_rel(a, y) * p + (2 * U if p > 0.1 else 0.0)


# ---------------------------------------------------------------------------- Gaussian scores
SCORE_N = (259, 10 ** 6, 10 ** 8)
SCORE_SCALE = {259: 4.0 ** 4, 10 ** 6: 4.0 ** 10, 10 ** 8: 4.0 ** 13}  # a power of 4 next to n: every sqrt is exact


def score_G(n):
    """d = 3, the ones column orthogonal to the data: G_00 = 3 s, G_11 = 4 s, G_22 = 16 s, G_01 = s, G_02 = 2 s, G_12 = 0,
    G_33 = n.  With s a power of 4 the unit-diagonal scaling and both eliminations are exact:
    rss of column 0 = 3 s, 2.75 s and 2.5 s on no, one ([1]) and two ([1, 2]) parents."""
    s = SCORE_SCALE[n]
    g = np.zeros((4, 4), dtype=np.float64)
    g[0, 0], g[1, 1], g[2, 2], g[3, 3] = 3 * s, 4 * s, 16 * s, float(n)
    g[0, 1] = g[1, 0] = s
    g[0, 2] = g[2, 0] = 2 * s
    return g


SCORE_JOBS = [([3], [0]), ([3, 1], [0]), ([3, 1, 2], [0])]  # (K, T): the ones column and 0, 1, 2 parents


def score_reference(n, parents, kind):
    """(score, tolerance, rss) of a family of score_G(n): the closed form by mpmath, under lgs_cases' bound of the
    score at an exact rss: 4 u (|llf| + n) + 2 u penalty."""
    import mpmath as mp

    rss = (3.0, 2.75, 2.5)[parents] * SCORE_SCALE[n]
    with mp.workdps(DPS):
        llf = -mp.mpf(n) / 2 * (mp.log(2 * mp.pi * mp.mpf(rss) / n) + 1)
        pen = {"ll": mp.mpf(0), "bic": mp.mpf(parents + 2) / 2 * mp.log(n), "aic": mp.mpf(parents + 2)}[kind]
        return float(llf - pen), 4 * U * (abs(float(llf)) + n) + 2 * U * float(pen), rss


# ---------------------------------------------------------------------------- structure scores
SCORE_FAMILIES = [([0], [4]), ([1, 2], [3, 4]), ([3, 4], [254, 1]), ([5, 6], [3, 129]), ([7, 8], [3, 4]), ([9], [5])]
BIG = 1 << 40


@functools.lru_cache(maxsize=None)
def score_counts():
    """The flat int64 tables of SCORE_FAMILIES: entries 2^(40 u), u uniform, a fifth of them 0; in the 129-column
    family (a chunk and a tail of one column) column 5 holds a single non-zero bin and the columns 7 and 128 are
    empty; every bin of the fifth family is 2^40; the last family has no parents and a state without a count."""
    rng = np.random.default_rng(40)
    offsets, sizes, _ = F.layout(SCORE_FAMILIES)
    counts = np.zeros(offsets[-1] + sizes[-1], dtype=np.int64)
    for f, (_, cards) in enumerate(SCORE_FAMILIES):
        v = np.floor(2.0 ** (40.0 * rng.random(sizes[f]))).astype(np.int64)
        v[rng.random(sizes[f]) < 0.2] = 0
        t = v.reshape(cards[0], -1)
        if f == 3:
            t[:, 5] = (0, 123456789012, 0)
            t[:, 7] = 0
            t[:, 128] = 0
        if f == 4:
            t[:] = BIG
        if f == 5:
            t[:, 0] = (BIG, 0, 1, 37, BIG - 1)
        counts[offsets[f]:offsets[f] + sizes[f]] = t.ravel()
    return counts


def score_params(kind):
    """(alpha, beta) per family: "k2" (r, 1) or "bdeu" (10 / q, 10 / (q r))."""
    alpha, beta = [], []
    for _, cards in SCORE_FAMILIES:
        r, q = int(cards[0]), int(np.prod(cards[1:], dtype=np.int64))
        alpha.append(float(r) if kind == "k2" else 10.0 / q)
        beta.append(1.0 if kind == "k2" else 10.0 / (q * r))
    return np.array(alpha), np.array(beta)


def score_tables():
    offsets, sizes, _ = F.layout(SCORE_FAMILIES)
    counts = score_counts()
    return [counts[offsets[f]:offsets[f] + sizes[f]].reshape(cards[0], -1) for f, (_, cards) in enumerate(SCORE_FAMILIES)]


def score_arguments():
    """(lgamma arguments, log arguments): the distinct fp64 values the score kernel evaluates on score_counts under
    LL, K2 and BDeu, formed as the kernel forms them (count + beta, column sum + alpha)."""
    lg, lo = [], []
    for f, t in enumerate(score_tables()):
        nj = t.sum(axis=0)
        lo += [t[t > 0].astype(np.float64), nj[nj > 0].astype(np.float64)]
        for kind in ("k2", "bdeu"):
            alpha, beta = score_params(kind)
            lg += [t.astype(np.float64).ravel() + beta[f], nj.astype(np.float64) + alpha[f]]
    return np.unique(np.concatenate(lg)), np.unique(np.concatenate(lo))


def write_ulp_arguments(path):
    """The argument list of tools/lgamma_ulp.hip: lines "lgamma <hex float>" and "log <hex float>"."""
    lg, lo = score_arguments()
    with open(path, "w") as f:
        for name, xs in (("lgamma", lg), ("log", lo)):
            for x in xs:
                f.write(f"{name} {float(x).hex()}\n")
    return len(lg), len(lo)
