"""Conditional-independence tests restated on the host, for the tests of pgm_fit_citest, CITests and PC.

A numpy / long-double restatement of include/pgmhip.h "conditional-independence tests": per stratum the
dropped empty rows and columns, dof_z, E = R C / n, the Yates correction at dof_z = 1, the power-divergence
term per cell; per test the sums and Q(dof / 2, stat / 2) in long double.  Beside each statistic it
returns the magnitude the error bound is taken from.

The bound.  A cell's term is a few fp64 operations on O, E = R C / n (two roundings) and O / E (one more).
A relative error eps in E moves (O - E)^2 / E by about 2 |O - E| eps, O ln(O / E) by O eps, E ln(E / O) by
E (|ln| + 1) eps and O (O / E)^lambda by |lambda| times itself; so a cell's magnitude is taken as
|term| + O + E (all times the stratum's factor), which covers each of these, and a statistic of n cells
is held to  (n - 1 + 2 U) 2^-53 sum(magnitude)  as the structure scores are (tests/score_cases.py):
n - 1 for the additions in any order, U for the roundings inside a cell.  U = 16: two roundings of E, one
of the ratio, one of log / pow (device log 0.503 ulp, pow under 2), the Yates shift, the product, each
counted with the sensitivity factor <= 2 above, rounded up to a power of two.  The reference (scipy, fp64)
and the device differ from the long-double value by that much each, so the restatement is compared with
either under the same bound.  The bound on the p-value is the change of Q over stat +- that bound plus
Q_REL of the value.  Q_REL is 10 x the error tools/ci_selftest.cpp measures on the recorded grid, which ends at
dof 5,000 (DESIGN.md records it); it is NOT the function's error at any dof: the prefactor's exponent a ln x -
x - lgamma(a) cancels, so the error grows with the dof (2.6e-10 at dof 10^6).  The cases of this module stay
at a dof of a few thousand, where the statistic's slack dominates; tests/crafted_cases.py q_tol is the bound of Q itself
at any dof, and tests/test_crafted_gpu.py holds the device to it.
"""
import ctypes
import ctypes.util
import json
import math
import os

import numpy as np

from tests import fit_cases as F

LD = np.longdouble
CHUNK = 128  # PGM_CI_CHUNK (include/pgmhip.h): strata per workgroup of the CI kernel
SMALL = 16   # kCiSmall (pgmpy_amd/csrc/pgm_fit.h): rx + ry of the one-work-item-per-stratum path
YATES = 1
U = 16.0
# the largest relative error of pgm_igamc against scipy.stats.chi2.sf that tools/ci_selftest.cpp measured over
# the grid of tests/golden/ci_cases.npz is 1.742e-12 at k = 5000; the tests allow 10 x that, under the ceiling 1e-9
Q_MEASURED = 1.742e-12
Q_REL = min(10 * Q_MEASURED, 1e-9)
LAMBDAS = {"pearson": 1.0, "log-likelihood": 0.0, "freeman-tukey": -0.5, "mod-log-likelihood": -1.0, "neyman": -2.0,
           "cressie-read": 2.0 / 3.0}

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.lgammal.restype = ctypes.c_longdouble
_libm.lgammal.argtypes = [ctypes.c_longdouble]


# ---------------------------------------------------------------------------- Q(a, x) in long double
def igamc(a, x):
    """The regularised upper incomplete gamma function in long double (series below a + 1, Lentz's
    continued fraction above); lgamma through libm's lgammal (ctypes rounds its value to fp64)."""
    a, x = LD(a), LD(x)
    if np.isnan(x) or np.isnan(a) or not a > 0:
        return LD("nan")
    if x <= 0:  # a statistic rounded below 0 counts as 0, as scipy's chi2.sf
        return LD(1)
    if np.isinf(x):
        return LD(0)
    with np.errstate(under="ignore"):
        lead = np.exp(a * np.log(x) - x - LD(_libm.lgammal(float(a))))
        eps = LD(2.0) ** -66
        if x < a + 1:
            term = 1 / a
            total, ap = term, a
            for _ in range(1000000):
                ap += 1
                term *= x / ap
                total += term
                if term < total * eps:
                    break
            return 1 - lead * total
        tiny = LD(np.finfo(LD).tiny) * 2 ** 64
        b = x + 1 - a
        c, d = 1 / tiny, 1 / b
        h = d
        for i in range(1, 1000000):
            an = -LD(i) * (LD(i) - a)
            b += 2
            d = an * d + b
            d = tiny if abs(d) < tiny else d
            c = b + an / c
            c = tiny if abs(c) < tiny else c
            d = 1 / d
            delta = d * c
            h *= delta
            if abs(delta - 1) < eps:
                break
        return lead * h


def chi2_sf(stat, dof):
    return igamc(LD(dof) / 2, LD(stat) / 2)


# ---------------------------------------------------------------------------- the restatement
def _term(o, e, lam):
    """One cell's term before the stratum's factor; scipy's conventions for O = 0."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if lam == 1.0:
            return (o - e) * (o - e) / e
        if lam == 0.0:
            return o * np.log(o / e) if o > 0 else LD(0)
        if lam == -1.0:
            return e * np.log(e / o) if o > 0 else LD("inf")
        if o == 0:
            return LD("nan") if lam < 0 else LD(0) * (LD(0) - 1)  # 0 * inf, as scipy
        return o * ((o / e) ** LD(lam) - 1)


def _factor(lam):
    return LD(1) if lam == 1.0 else LD(2) if lam in (0.0, -1.0) else 2 / (LD(lam) * (LD(lam) + 1))


def stratum_ref(table, lam, yates=True):
    """(stat, dof, magnitude, cells) of one [rx, ry] int64 table."""
    table = np.asarray(table, dtype=np.int64)
    table = table[table.sum(axis=1) > 0][:, table.sum(axis=0) > 0] if table.sum() > 0 else table[:0, :0]
    if table.size == 0:
        return LD(0), 0, LD(0), 0
    dof = (table.shape[0] - 1) * (table.shape[1] - 1)
    if dof == 0:
        return LD(0), 0, LD(0), 0
    R, C, n = table.sum(axis=1), table.sum(axis=0), LD(int(table.sum()))
    factor = _factor(lam)
    stat, mag = LD(0), LD(0)
    for x in range(table.shape[0]):
        for y in range(table.shape[1]):
            e = LD(int(R[x])) * LD(int(C[y])) / n
            o = LD(int(table[x, y]))
            if yates and dof == 1:
                o = o + np.sign(e - o) * min(LD(0.5), abs(e - o))
            t = _term(o, e, lam)
            stat += factor * t
            if np.isfinite(t):
                mag += abs(factor) * (abs(t) + o + e)
    return stat, dof, mag, table.size


def ci_ref(table, lam, yates=True, has_z=None):
    """(stat LD, dof, pvalue LD, magnitude LD, cells) of one [rx, ry, qz] int64 table."""
    table = np.asarray(table, dtype=np.int64)
    has_z = table.shape[2] > 1 if has_z is None else has_z
    stat, dof, mag, cells = LD(0), 0, LD(0), 0
    for z in range(table.shape[2]):
        s, d, m, c = stratum_ref(table[:, :, z], lam, yates)
        stat, dof, mag, cells = stat + s, dof + d, mag + m, cells + c
    if dof == 0:
        p = LD("nan") if has_z else LD(1)
    else:
        p = chi2_sf(stat, dof)
    return stat, dof, p, mag, cells


def bound(cells, magnitude):
    return float((max(cells - 1, 0) + 2.0 * U) * 2.0 ** -53 * float(magnitude))


def p_bound(stat, dof, p, stat_bound):
    """How far a p-value may lie from the restatement's: the change of Q over stat +- stat_bound, plus
    Q_REL of the value, plus the smallest normal fp64 (below it a value is denormal or flushed to 0 and has
    no relative precision left)."""
    if dof == 0 or not np.isfinite(float(stat)):
        return 0.0
    lo, hi = chi2_sf(max(LD(stat) - LD(stat_bound), LD(0)), dof), chi2_sf(LD(stat) + LD(stat_bound), dof)
    return float(abs(lo - hi)) + Q_REL * float(p) + float(np.finfo(np.float64).tiny)


def same(got, want, tol):
    """NaN equals NaN, inf equals inf, otherwise |got - want| <= tol."""
    got, want = float(got), float(want)
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got)
    if math.isinf(want) or math.isinf(got):
        return got == want
    return abs(got - want) <= tol


def tables_of(codes, families):
    """The [rx, ry, qz] table of every family (X, Y, Z...) over host codes [n_cols, n_rows]."""
    counts = F.count_ref(codes, families)
    offsets, sizes, _ = F.layout(families)
    return [counts[offsets[f]:offsets[f] + sizes[f]].reshape(int(c[0]), int(c[1]), -1) for f, (_, c) in enumerate(families)]


# ---------------------------------------------------------------------------- frames and a host tester
def _pack_case(case, prefix, arrays):
    """A case's frame as state names + uint8 codes (255: missing), its tests as triples + [n, 6, 3] results."""
    case = dict(case)
    frame, tests = case.pop("frame"), case.pop("tests")
    states = {c: sorted({x for x in v if x is not None}) for c, v in frame.items()}
    arrays[prefix + "codes"] = np.array([[255 if x is None else states[c].index(x) for x in v]
                                         for c, v in frame.items()], dtype=np.uint8)
    arrays[prefix + "results"] = np.array([[t["results"][name] for name in LAMBDAS] for t in tests], dtype=np.float64)
    return dict(case, states=states, triples=[[t["X"], t["Y"], t["Z"]] for t in tests])


def _unpack_case(case, prefix, arrays):
    case = dict(case)
    states, triples = case.pop("states"), case.pop("triples")
    codes, results = arrays[prefix + "codes"], arrays[prefix + "results"]
    case["frame"] = {c: [None if k == 255 else states[c][k] for k in codes[i]] for i, c in enumerate(states)}
    case["tests"] = [{"X": X, "Y": Y, "Z": Z, "results": {name: [float(r[0]), float(r[1]), int(r[2])]
                                                        for name, r in zip(LAMBDAS, results[i])}}
                     for i, (X, Y, Z) in enumerate(triples)]
    return case


def pack_golden(out):
    """(meta for ci_cases.json, arrays for ci_cases.npz) of the generator's record: the frames, every
    recorded float and the alarm separating-set sizes go to the arrays (exact float64), names and graphs
    stay readable in the json."""
    arrays = {"sf_grid": np.array(out["sf_grid"], dtype=np.float64)}
    meta = {"s": _pack_case(out["s"], "s_", arrays),
            "edge": {k: _pack_case(c, f"edge_{k}_", arrays) for k, c in out["edge"].items()}, "pdags": out["pdags"]}
    nodes = sorted({v for pair, _ in out["alarm"]["separating_set_sizes"] for v in pair})
    meta["alarm"] = {"nodes": nodes}
    for key, rec in (("stable", out["alarm"]), ("parallel", out["alarm"]["parallel"])):
        meta["alarm"][key] = {"edges": rec["edges"]}
        arrays[f"alarm_{key}_sizes"] = np.array([[nodes.index(a), nodes.index(b), n]
                                                 for (a, b), n in rec["separating_set_sizes"]], dtype=np.int16)
    return meta, arrays


def load_golden():
    """The generator's record, put together again from ci_cases.json and ci_cases.npz."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "ci_cases.json")) as f:
        meta = json.load(f)
    arrays = np.load(os.path.join(here, "ci_cases.npz"))
    nodes = meta["alarm"]["nodes"]
    alarm = {key: {"edges": meta["alarm"][key]["edges"],
                   "separating_set_sizes": sorted([sorted((nodes[a], nodes[b])), int(n)]
                                                  for a, b, n in arrays[f"alarm_{key}_sizes"])}
             for key in ("stable", "parallel")}
    return {"s": _unpack_case(meta["s"], "s_", arrays),
            "edge": {k: _unpack_case(c, f"edge_{k}_", arrays) for k, c in meta["edge"].items()},
            "alarm": dict(alarm["stable"], parallel=alarm["parallel"]), "pdags": meta["pdags"],
            "sf_grid": [[int(k), float(x), float(sf)] for k, x, sf in arrays["sf_grid"]]}


def frame_of(case):
    """The recorded frame: {column: values}, null -> NaN (object columns)."""
    import pandas as pd

    return pd.DataFrame({c: np.asarray([np.nan if x is None else x for x in v], dtype=object)
                         for c, v in case["frame"].items()})


def alarm_frame():
    """The 1,000 alarm rows of fit_alarm.npz under the model's state names, nodes sorted."""
    import pandas as pd

    from pgmpy_amd.utils import get_example_model

    m = get_example_model("alarm")
    nodes = sorted(m.nodes())
    _, alarm = F.load_golden()
    codes = np.asarray(alarm["codes"])
    states = {v: list(m.states[v]) for v in nodes}
    return pd.DataFrame({v: np.asarray(states[v], dtype=object)[codes[i]] for i, v in enumerate(nodes)}), states


class HostTester:
    """The tester interface of estimators.PC.pc_skeleton on the host: the restatement over host-encoded
    codes.  `calls` records the triples of every batch."""

    def __init__(self, df, lam=1.0, state_names=None):
        from pgmpy_amd.inference.batch import encode_states

        self.lam = lam
        self.variables = list(df.columns)
        self.states = F.collected_states(df, state_names)
        self.codes = encode_states({v: self.states[v] for v in self.variables}, df, self.variables)
        self.calls = []

    def family(self, X, Y, Z):
        scope = [X, Y] + list(Z)
        return [self.variables.index(v) for v in scope], [len(self.states[v]) for v in scope]

    def tests(self, triples, lam=None):
        lam = self.lam if lam is None else lam
        fams = [self.family(X, Y, Z) for X, Y, Z in triples]
        return [ci_ref(t, lam, True, len(Z) > 0) for t, (_, _, Z) in zip(tables_of(self.codes, fams), triples)]

    def independent(self, triples, significance_level, lam=None):
        triples = [(X, Y, list(Z)) for X, Y, Z in triples]
        self.calls.append(triples)
        return [bool(float(r[2]) >= significance_level) for r in self.tests(triples, lam)]


# ---------------------------------------------------------------------------- the kernel-level case table
def kernel_cases():
    """[{name, families, codes [n_cols, n_rows] uint8}] (seeded; built once per call): the smallest
    shapes at which the CI kernels can go wrong.  A family is (X, Y, Z...)."""
    rng = np.random.default_rng(2026)
    cases = []

    def add(name, families, n_rows, missing=0.0, codes=None):
        n_cols = 1 + max(c for cols, _ in families for c in cols)
        if codes is None:
            codes = F._random_codes(rng, n_cols, n_rows, F._col_cards(families, n_cols), missing)
        cases.append({"name": name, "families": families, "codes": codes})

    assert CHUNK == 128 and SMALL == 16, "the families below are chosen for a 128-stratum chunk and rx + ry <= 16"
    # one Z of cardinality 1, 2, one less than, equal to and one more than a chunk; three chunks and a tail
    add("qz_edges", [([0, 1], [3, 2]), ([0, 1, 2], [3, 2, 1]), ([0, 1, 3], [3, 2, 2]), ([0, 1, 4], [3, 2, 127]),
                     ([0, 1, 5], [3, 2, 128]), ([0, 1, 6], [3, 2, 129]), ([1, 0, 7], [2, 3, 255])], 2000, missing=0.02)
    add("two_z", [([0, 1, 2, 3], [3, 3, 4, 5]), ([1, 0, 3, 2], [3, 3, 5, 4]), ([0, 1, 2, 3], [3, 3, 4, 5])], 1500)
    add("rx_ry_1", [([0, 1], [1, 4]), ([1, 0], [4, 1]), ([0, 1, 2], [1, 4, 3]), ([1, 0, 2], [4, 1, 3]), ([0, 3], [1, 1])], 300)
    # past the small-table path: the general path with one, three and 130 strata; rx + ry = 16 and 17
    add("general", [([0, 1, 2], [40, 40, 3]), ([0, 1], [40, 40]), ([3, 4, 5], [9, 8, 130]), ([3, 6], [9, 7]),
                    ([3, 4], [9, 8]), ([7, 8, 2], [254, 3, 3])], 2000, missing=0.02)
    # strata without rows, with one non-empty row (dof_z = 0) and 2 x 2 strata (dof_z = 1, Yates)
    codes = F._random_codes(rng, 4, 600, [3, 3, 6, 2], 0.0)
    codes[2][codes[2] == 4] = 3              # stratum 4 never occurs
    codes[0][codes[2] == 1] = 2              # stratum 1: one row of the table
    codes[0][(codes[2] == 2) & (codes[0] == 2)] = 0
    codes[1][(codes[2] == 2) & (codes[1] == 2)] = 1   # stratum 2: 2 x 2
    add("strata", [([0, 1, 2], [3, 3, 6]), ([3, 1, 2], [2, 3, 6]), ([3, 0, 2], [2, 3, 6]), ([0, 3], [3, 2])],
        600, codes=codes)
    codes = F._random_codes(rng, 3, 400, [2, 2, 3], 0.0)
    add("two_by_two", [([0, 1], [2, 2]), ([0, 1, 2], [2, 2, 3]), ([1, 0], [2, 2])], 400, codes=codes)
    # zero cells: the pair (0, 2) and (2, 0) of X, Y never occurs
    codes = F._random_codes(rng, 3, 500, [3, 3, 2], 0.0)
    codes[1][(codes[0] == 0) & (codes[1] == 2)] = 1
    codes[1][(codes[0] == 2) & (codes[1] == 0)] = 1
    add("zero_cells", [([0, 1], [3, 3]), ([0, 1, 2], [3, 3, 2])], 500, codes=codes)
    add("all_missing", [([0, 1], [3, 2]), ([0, 1, 2], [3, 2, 4])], 100, codes=np.full((3, 100), F.MISSING, dtype=np.uint8))
    # 1,400 packed tests over 38 columns: many workgroups of the packed kernel and a tail
    col_card = [2 + c % 4 for c in range(38)]
    pairs = [(a, b) for a in range(38) for b in range(38) if a != b][:1400]
    add("pairs_1400", [([a, b], [col_card[a], col_card[b]]) for a, b in pairs], 500, missing=0.05)
    return cases


def mixed_batch(cases):
    """One case that holds the families of all the others (columns shifted so that every family keeps its
    own data; rows padded with MISSING to the longest) and, per family, where it came from."""
    n_rows = max(c["codes"].shape[1] for c in cases)
    blocks, families, origin, base = [], [], [], 0
    for ci, c in enumerate(cases):
        if c["name"] == "pairs_1400":
            continue
        pad = np.full((c["codes"].shape[0], n_rows), F.MISSING, dtype=np.uint8)
        pad[:, :c["codes"].shape[1]] = c["codes"]
        blocks.append(pad)
        for fi, (cols, cards) in enumerate(c["families"]):
            families.append(([base + col for col in cols], list(cards)))
            origin.append((ci, fi))
        base += c["codes"].shape[0]
    return {"name": "mixed", "families": families, "codes": np.concatenate(blocks)}, origin
