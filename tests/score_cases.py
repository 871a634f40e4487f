"""Structure scores: the numpy restatement of the score kernel and of the host constants, the error bound
of their comparison, and the case lists of the tests.

A family's table is the CPD's ``[r, q]`` int64 counts (tests/fit_cases.py).  N_jk is the count of state
k in column j, N_j their sum over k.  The restatement forms every argument in fp64 exactly as the kernel
and the reference do (``N_jk + beta``, ``N_j + alpha``, the integers themselves), evaluates lgamma with
libm's ``lgammal`` through ctypes and log with numpy's long-double loop (``logl``), and adds the terms
in ``np.longdouble``.  ctypes hands ``lgammal``'s value back rounded to fp64: half an fp64 ulp per term,
which the doubled U of the bound covers (U >= 1/2).

  score_ref     per family: (sum of the column terms, sum of |term|, number of terms, observed columns)
  local_ref     the same with a score's host constants added (K2, BDeu, BDs, LL, BIC, AIC)
  bound         (n - 1 + 2 U) 2^-53 sum|t_i|: n - 1 for the summation in any order (as the fit tests), U
                the largest ulp error of the evaluated lgamma / log, doubled because real data reaches
                arguments the sample does not.  A term is one lgamma or log value (times an integer
                count or column number); an LL bin N (log N_jk - log N_j) is two terms; every further
                rounding of a host constant (a product, a division) counts as one more term.
"""
import ctypes
import ctypes.util
import json
import math
import os

import numpy as np

from tests import fit_cases as F

LD = np.longdouble
BD, LL, SKIP_EMPTY = 0, 1, 2
CHUNK = 128  # PGM_SCORE_CHUNK (include/pgmhip.h): CPD columns per workgroup of the score kernel

# Largest error, in fp64 ulps of the exact value, of the device's lgamma / log against lgammal / logl
# over the arguments the cases produce (tools/lgamma_ulp.hip on an MI355X; DESIGN.md "Structure scores").
U_DEVICE = 1.538  # lgamma(4357 + 10/1260); log: 0.503
# The same over the distinct arguments of the large-count cases of tests/crafted_cases.py (counts up to 2^40;
# crafted_cases.write_ulp_arguments, tools/lgamma_ulp.hip --args on an MI355X, 2026-10-21).
U_DEVICE_LARGE = 1.355  # lgamma(9), of 1,182 arguments; log: 0.498 at 586, of 561
# The same for scipy.special.gammaln / numpy.log on the host that recorded the goldens, measured by
# host_ulp() below (+ 1/2 for ctypes' rounding of the long-double value).
U_HOST = 905.5

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.lgammal.restype = ctypes.c_longdouble
_libm.lgammal.argtypes = [ctypes.c_longdouble]


def lgammal(x):
    """lgammal of an fp64 array (evaluated once per distinct argument)."""
    x = np.asarray(x, dtype=np.float64)
    u, inv = np.unique(x.ravel(), return_inverse=True)
    v = np.array([_libm.lgammal(float(a)) for a in u], dtype=LD)
    return v[inv].reshape(x.shape)


def logl(x):
    return np.log(np.asarray(x, dtype=np.float64).astype(LD))


def family_terms(table, mode, alpha=None, beta=None):
    """(sum, sum of |term|, number of terms, observed columns) of one [r, q] int64 table."""
    table = np.asarray(table, dtype=np.int64)
    nj = table.sum(axis=0)
    observed = int((nj > 0).sum())
    if mode & LL:
        keep = table > 0
        n = table.astype(np.float64).astype(LD)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.where(keep, n * logl(np.where(keep, table, 1)), LD(0))
            b = np.where(keep, n * logl(np.where(nj > 0, nj, 1))[None, :], LD(0))
        total = (a - b).sum(dtype=LD)
        return total, (np.abs(a) + np.abs(b)).sum(dtype=LD), 2 * int(keep.sum()), observed
    cols = nj > 0 if mode & SKIP_EMPTY else np.ones(nj.shape, dtype=bool)
    bins = lgammal(table[:, cols].astype(np.float64) + np.float64(beta))
    cond = lgammal(nj[cols].astype(np.float64) + np.float64(alpha))
    total = bins.sum(dtype=LD) - cond.sum(dtype=LD)
    return total, np.abs(bins).sum(dtype=LD) + np.abs(cond).sum(dtype=LD), int(bins.size + cond.size), observed


def score_ref(counts, families, mode, alpha=None, beta=None):
    """Per family of a flat count buffer: arrays (sum LD, magnitude LD, terms int64, observed int64)."""
    offsets, sizes, _ = F.layout(families)
    out = [family_terms(np.asarray(counts[offsets[f]:offsets[f] + sizes[f]]).reshape(int(cards[0]), -1), mode,
                        None if alpha is None else alpha[f], None if beta is None else beta[f])
           for f, (cols, cards) in enumerate(families)]
    return (np.array([o[0] for o in out], dtype=LD), np.array([o[1] for o in out], dtype=LD),
            np.array([o[2] for o in out], dtype=np.int64), np.array([o[3] for o in out], dtype=np.int64))


def bound(n_terms, magnitude, U):
    return (np.maximum(np.asarray(n_terms) - 1, 0) + 2.0 * U) * 2.0 ** -53 * np.asarray(magnitude, dtype=np.float64)


def _lg(x):
    return LD(_libm.lgammal(float(x)))


def local_ref(name, table, ess=10, sample_size=None, has_parents=None):
    """(score LD, magnitude, terms) of one family under the named score: family_terms plus the host
    constants of pgmpy_amd/estimators/StructureScore.py.  has_parents (default: q > 1) matters to BDeu
    and BDs: for a family with parents the reference's count table has no row for a state without a
    count, so lgamma(0 + beta) is left out once per such state and observed column."""
    table = np.asarray(table, dtype=np.int64)
    r, q = table.shape
    has_parents = q > 1 if has_parents is None else has_parents
    dropped = int((table.sum(axis=1) == 0).sum()) * int((table.sum(axis=0) > 0).sum()) if has_parents else 0
    consts = []  # (value, roundings)
    if name == "k2":
        s, mag, n, _ = family_terms(table, BD | SKIP_EMPTY, float(r), 1.0)
        consts = [(q * _lg(r), 2)]
    elif name == "bdeu":
        a, b = ess / q, ess / (q * r)
        s, mag, n, _ = family_terms(table, BD, a, b)
        consts = [(q * _lg(a), 2), (-(q * r) * _lg(b), 2), (-dropped * _lg(b), 2)]
    elif name == "bds":
        q_obs = int((table.sum(axis=0) > 0).sum())
        a, b = ess / q_obs, ess / (q * r)
        s, mag, n, _ = family_terms(table, BD | SKIP_EMPTY, a, b)
        empty = q - q_obs
        consts = [(empty * r * _lg(b), 2), (-empty * _lg(a), 2), (q_obs * _lg(a), 2), (-(q * r) * _lg(b), 2),
                  (-dropped * _lg(b), 2)]
    else:
        s, mag, n, _ = family_terms(table, LL)
        if name == "bic-d":
            consts = [(-LD(0.5) * LD(math.log(sample_size)) * q * (r - 1), 4)]
        elif name == "aic-d":
            consts = [(-LD(q * (r - 1)), 1)]
    for value, roundings in consts:
        s, mag, n = s + value, mag + abs(value), n + roundings
    return s, mag, n


# 10 / d are the alphas and betas the cases' families produce at equivalent sample size 10 (the list of
# tools/lgamma_ulp.hip)
ULP_DENOMS = (1, 2, 3, 4, 6, 8, 9, 12, 16, 18, 24, 27, 36, 54, 72, 81, 108, 162, 254, 381, 384, 1260, 4096, 4097, 12288)


def host_ulp(max_count=4100):
    """Largest error of scipy's gammaln and numpy's log, in fp64 ulps of the long-double value, over the
    integers 1 .. max_count and integer + 10 / d (what U_HOST records; the goldens' largest count is
    2,000).  The largest errors sit next to lgamma's zeros at 1 and 2, where the value is small."""
    from scipy.special import gammaln

    n = np.arange(0, max_count + 1, dtype=np.float64)
    worst = 0.0
    for d in ULP_DENOMS:
        x = n + np.float64(10.0 / d)
        x = x[x > 0]
        exact = lgammal(x)
        err = np.abs(gammaln(x).astype(LD) - exact)
        ulp = np.spacing(np.abs(exact.astype(np.float64)))
        ok = exact != 0
        worst = max(worst, float((err[ok] / ulp[ok]).max()))
    x = n[1:]
    exact = logl(x)
    ok = exact != 0
    err = np.abs(np.log(x).astype(LD) - exact)
    worst = max(worst, float((err[ok] / np.spacing(np.abs(exact.astype(np.float64)))[ok]).max()))
    return worst


# ---------------------------------------------------------------------------- kernel cases
def kernel_params(families):
    """(alpha, beta) per family for the BD modes: even families BDeu-like (10 / q, 10 / (q r)), odd
    families K2-like (r, 1): non-integer and integer arguments."""
    alpha, beta = [], []
    for f, (cols, cards) in enumerate(families):
        r, q = int(cards[0]), int(np.prod(cards[1:], dtype=np.int64))
        alpha.append(10.0 / q if f % 2 == 0 else float(r))
        beta.append(10.0 / (q * r) if f % 2 == 0 else 1.0)
    return np.array(alpha), np.array(beta)


def kernel_cases():
    """[{name, families, codes [n_cols, n_rows] uint8}] (seeded; built once per call): the smallest
    shapes at which the score kernel can go wrong."""
    rng = np.random.default_rng(2025)
    cases = []

    def add(name, families, n_rows, missing=0.0, codes=None):
        n_cols = 1 + max(c for cols, _ in families for c in cols)
        if codes is None:
            codes = F._random_codes(rng, n_cols, n_rows, F._col_cards(families, n_cols), missing)
        cases.append({"name": name, "families": families, "codes": codes})

    for n in (1, 65, 4097):
        add(f"mixed_{n}", F.MIXED, n, missing=0.1)
    add("no_parents", [([0], [3])], 300)
    add("r_1", [([0, 1], [1, 4]), ([1], [4])], 300, missing=0.1)
    add("r_254_parent_1", [([0, 1], [254, 1])], 3000, missing=0.1)
    # columns one less than, equal to and one more than a chunk; three chunks and a tail of 36
    assert CHUNK == 128, "the families below are factorised for a 128-column chunk"
    add("chunk_edges", [([0, 1], [3, 127]), ([0, 2, 3], [3, 8, 16]), ([0, 4, 5], [3, 3, 43]), ([0, 6, 7], [3, 20, 21])],
        5000, missing=0.02)
    add("above_tile", [([0, 1], [17, 241])], 6000, missing=0.02)
    cards = [3] + [2] * 12 + [1] * (F.MAX_DIMS - 13)
    add("max_parents_global", [(list(range(F.MAX_DIMS)), cards), ([5], [2])], 1500, missing=0.01)
    add("one_bin", F.MIXED, 700, codes=np.full((6, 700), 1, dtype=np.uint8))
    add("all_missing", F.MIXED, 200, codes=np.full((6, 200), F.MISSING, dtype=np.uint8))
    add("rows_100000", [([0, 1, 2], [3, 2, 2]), ([1], [2]), ([2, 0], [2, 3])], 100000)
    # 1,400 two-column families over 38 columns of cardinality 2 .. 5: many count groups
    col_card = [2 + c % 4 for c in range(38)]
    pairs = [(a, b) for a in range(38) for b in range(38) if a != b][:1400]
    add("families_1400", [([a, b], [col_card[a], col_card[b]]) for a, b in pairs], 500, missing=0.05)
    return cases


# ---------------------------------------------------------------------------- golden cases (tests/golden)
NAMES = ("k2", "bdeu", "bds", "bic-d", "aic-d", "ll-d")


def load_golden():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "score_cases.json")) as f:
        return json.load(f)


def case_frame(golden, key):
    """The input DataFrame of case a, b, c, d (the fit case's frame without `_weight`) or s."""
    import pandas as pd

    case = golden[key]
    if "frame" in case:
        return pd.DataFrame({c: np.asarray(v, dtype=object) for c, v in case["frame"].items()})
    fit, _ = F.load_golden()
    df = F.golden_frame(fit[case["fit_case"]])
    return df[[c for c in df.columns if c != "_weight"]]


def case_tables(golden, key):
    """{(variable, parents tuple): [r, q] int64 table} for every recorded family of a case, from
    host-encoded codes through fit_cases.count_ref, and the frame's row count."""
    from pgmpy_amd.inference.batch import encode_states

    df = case_frame(golden, key)
    variables = list(df.columns)
    states = F.collected_states(df, golden[key]["state_names"])
    codes = encode_states({v: states[v] for v in variables}, df, variables)
    fams, keys = [], []
    for rec in golden[key]["local"]:
        scope = [rec["variable"]] + list(rec["parents"])
        fams.append(([variables.index(v) for v in scope], [len(states[v]) for v in scope]))
        keys.append((rec["variable"], tuple(rec["parents"])))
    counts = F.count_ref(codes, fams)
    offsets, sizes, _ = F.layout(fams)
    return {k: counts[offsets[f]:offsets[f] + sizes[f]].reshape(fams[f][1][0], -1) for f, k in enumerate(keys)}, len(df)


class HostScorer:
    """The scorer interface of estimators.HillClimbSearch.hill_climb on the host: local scores by the
    restatement over host-encoded codes (rounded to fp64), the structure prior of the named score."""

    def __init__(self, name, df, state_names=None, ess=10):
        from pgmpy_amd.inference.batch import encode_states

        self.name, self.ess, self.n = name, ess, len(df)
        self.variables = list(df.columns)
        self.states = F.collected_states(df, state_names)
        self.codes = encode_states({v: self.states[v] for v in self.variables}, df, self.variables)
        self.calls = []  # the families of every local_scores call

    def local_scores(self, families):
        families = [(v, list(ps)) for v, ps in families]
        self.calls.append([(v, tuple(ps)) for v, ps in families])
        fams = [([self.variables.index(u) for u in [v] + ps], [len(self.states[u]) for u in [v] + ps])
                for v, ps in families]
        counts = F.count_ref(self.codes, fams)
        offsets, sizes, _ = F.layout(fams)
        return [float(local_ref(self.name, counts[offsets[f]:offsets[f] + sizes[f]].reshape(fams[f][1][0], -1),
                                self.ess, self.n, len(fams[f][0]) > 1)[0]) for f in range(len(fams))]

    def structure_prior_ratio(self, operation):
        if self.name == "bds":
            return {"+": -math.log(2.0), "-": math.log(2.0)}.get(operation, 0)
        return 0

    def structure_prior(self, model):
        if self.name != "bds":
            return 0
        nodes = float(len(model.nodes()))
        return -(float(len(model.edges())) + nodes * (nodes - 1) / 2.0) * math.log(2.0)
