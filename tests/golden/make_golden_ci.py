#!/usr/bin/env python3
"""Generate the CI-test and PC fixtures by running the REFERENCE CITests, PC and PDAG, and scipy.

    PYTHONHASHSEED=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ci.py

Same set-up as make_golden.py (its _setup(): the reference and the offline shims on sys.path).  Writes
recorded inputs and results only, as tests/ci_cases.py's pack_golden splits them: names, triples and graphs
to ci_cases.json, the frames (uint8 codes) and every recorded number (float64) to ci_cases.npz:

  s        a seeded 2,000-row frame over seven variables (cardinalities 2-3) with the known structure
           A -> C <- B, C -> D and E -> G <- F (two components: every
           dependence is strong or absent, so few p-values of a PC run fall near alpha):
           "tests": for every pair (column order) and every Z of size 0-2 the reference's (chi, p, dof)
                    under the six named lambdas
           "pc":    per test in chi_square, g_sq the reference's build_skeleton(variant="stable",
                    significance_level=0.01): edges, separating sets, and the directed / undirected edges
                    of estimate(return_type="pdag"); "checks" records what the generator verified (it
                    stops otherwise): no p-value of the run lies in [alpha / 2, 2 alpha]; "orig", "stable"
                    and "parallel" give the same skeleton and separating sets; the reference loop with
                    neighbours walked in column order gives the same skeleton, separating sets and PDAG
  edge     small frames: a stratum with one non-empty row (dof_z = 0), total dof 0 (Z a copy of X: (0, nan,
           0); a constant Y without Z: p = 1), 2 x 2 strata (Yates), a zero cell (lambda = -1: inf, p = 0;
           lambda = -2, -1/2: scipy's nan), a Z configuration that never occurs, NaN where the semantics
           coincide (in Z columns, or in tests without Z)
  alarm    over the 1,000 rows of fit_alarm.npz: the reference's "stable" chi_square skeleton edges and the
           size of each separating set; under "parallel" the same of its "parallel" variant (the only one
           that tests a level against frozen neighbour sets)
  pdags    small PDAGs as edge lists with the reference's apply_meeks_rules (with and without R4) and
           to_dag() edges
  sf_grid  scipy.stats.chi2.sf(x, k) for k in 1, 2, 3, 10, 100, 1000, 5000, x from 1e-3 k to 20 k, and tail
           points down to p = 1e-300

--time-pc: wall time of one reference PC.estimate(variant="stable") on the alarm rows (the comparison row
of tools/ci_bench.py's table; writes no fixture).

"""
import itertools
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as G  # noqa: E402

LAMBDAS = {"pearson": 1.0, "log-likelihood": 0.0, "freeman-tukey": -0.5, "mod-log-likelihood": -1.0, "neyman": -2.0,
           "cressie-read": 2.0 / 3.0}
ALPHA = 0.01
S_SEED = 4


def _lab(x, prefix, k):
    return np.asarray([f"{prefix}{i}" for i in range(k)], dtype=object)[x]


def _noisy(rng, x, k, rate):
    x = x.copy()
    flip = rng.random(len(x)) < rate
    x[flip] = rng.integers(0, k, flip.sum())
    return x


def frame_s(seed=S_SEED):
    import pandas as pd

    rng = np.random.default_rng(seed)
    n = 2000
    a = rng.choice(3, n, p=[0.4, 0.35, 0.25])
    b = rng.choice(2, n, p=[0.55, 0.45])
    c = _noisy(rng, (a + 2 * b) % 3, 3, 0.1)
    d = _noisy(rng, (c + 1) % 3, 3, 0.15)
    e = rng.choice(2, n, p=[0.5, 0.5])
    f = rng.choice(2, n, p=[0.6, 0.4])
    g = _noisy(rng, e + f, 3, 0.1)
    return pd.DataFrame({"A": _lab(a, "a", 3), "B": _lab(b, "b", 2), "C": _lab(c, "c", 3), "D": _lab(d, "d", 3),
                         "E": _lab(e, "e", 2), "F": _lab(f, "f", 2), "G": _lab(g, "g", 3)})


def _result(X, Y, Z, df):
    import warnings

    from pgmpy.estimators.CITests import power_divergence

    out = {}
    for name in LAMBDAS:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            chi, p, dof = power_divergence(X, Y, list(Z), df, boolean=False, lambda_=name)
        out[name] = [float(chi), float(p), int(dof)]
    return out


def all_tests(df, max_z=2):
    cols = list(df.columns)
    out = []
    for X, Y in itertools.combinations(cols, 2):
        rest = [c for c in cols if c not in (X, Y)]
        for k in range(max_z + 1):
            for Z in itertools.combinations(rest, k):
                out.append({"X": X, "Y": Y, "Z": list(Z), "results": _result(X, Y, Z, df)})
    return out


def _skeleton_record(skel, sepsets):
    return {"edges": sorted(sorted(e) for e in skel.edges()),
            "separating_sets": sorted([sorted(k), sorted(v)] for k, v in sepsets.items())}


def _pdag_record(pdag):
    return {"nodes": sorted(pdag.nodes()), "directed": sorted(list(e) for e in pdag.directed_edges),
            "undirected": sorted(sorted(e) for e in pdag.undirected_edges)}


def _column_order_sepsets(columns):
    """The reference's candidate enumeration with neighbours walked in column order instead of set order."""
    from itertools import chain, combinations

    order = {c: i for i, c in enumerate(columns)}

    def potential(u, v, temporal_ordering, graph, lim_neighbors):
        nu = sorted((w for w in graph.neighbors(u) if w != v), key=order.__getitem__)
        nv = sorted((w for w in graph.neighbors(v) if w != u), key=order.__getitem__)
        return chain(combinations(nu, lim_neighbors), combinations(nv, lim_neighbors))

    return staticmethod(potential)


def pc_on_s(df):
    from pgmpy.estimators import PC
    from pgmpy.estimators import CITests as RC
    from pgmpy.estimators.BaseConstraintEstimator import BaseConstraintEstimator as Base

    out = {}
    for name in ("chi_square", "g_sq"):
        fn = getattr(RC, name)
        pvalues = []

        def recording(X, Y, Z, data, boolean=True, **kw):
            chi, p, dof = fn(X, Y, Z, data, boolean=False)
            pvalues.append(float(p))
            return p >= kw["significance_level"]

        runs = {}
        for variant in ("orig", "stable", "parallel"):
            skel, sep = PC(df).build_skeleton(variant=variant, ci_test=name, significance_level=ALPHA, n_jobs=1,
                                              show_progress=False)
            runs[variant] = _skeleton_record(skel, sep)
        skel, sep = PC(df).build_skeleton(variant="stable", ci_test=recording, significance_level=ALPHA,
                                          show_progress=False)
        assert _skeleton_record(skel, sep) == runs["stable"]
        close = [p for p in pvalues if ALPHA / 2 <= p <= 2 * ALPHA]
        if close:
            raise SystemExit(f"{name}: p-values {close} lie within [alpha / 2, 2 alpha]: pick another seed")
        if not (runs["orig"] == runs["stable"] == runs["parallel"]):
            raise SystemExit(f"{name}: the variants disagree: pick another seed")
        pdag = PC(df).estimate(variant="stable", ci_test=name, return_type="pdag", significance_level=ALPHA,
                               show_progress=False)
        saved = Base.__dict__["_get_potential_sepsets"]  # the staticmethod object itself
        Base._get_potential_sepsets = _column_order_sepsets(list(df.columns))
        try:
            skel2, sep2 = PC(df).build_skeleton(variant="stable", ci_test=name, significance_level=ALPHA,
                                                show_progress=False)
            pdag2 = PC(df).estimate(variant="stable", ci_test=name, return_type="pdag", significance_level=ALPHA,
                                    show_progress=False)
        finally:
            Base._get_potential_sepsets = saved
        if _skeleton_record(skel2, sep2) != runs["stable"] or _pdag_record(pdag2) != _pdag_record(pdag):
            raise SystemExit(f"{name}: the column-order loop gives another result: pick another seed")
        out[name] = dict(runs["stable"], pdag=_pdag_record(pdag), tests_run=len(pvalues),
                         checks={"no_pvalue_in": [ALPHA / 2, 2 * ALPHA], "variants_agree": True,
                                 "column_order_agrees": True,
                                 "closest_pvalue_ratio": float(min(max(p / ALPHA, ALPHA / p) for p in pvalues if p > 0))})
    return out


# ---------------------------------------------------------------------------- edge frames
def edge_frames():
    import pandas as pd

    rng = np.random.default_rng(11)
    out = {}

    def record(key, df, triples, note):
        frame = {c: [None if (isinstance(x, float) and np.isnan(x)) else x for x in df[c].tolist()] for c in df.columns}
        out[key] = {"note": note, "frame": frame,
                    "tests": [{"X": X, "Y": Y, "Z": list(Z), "results": _result(X, Y, Z, df)} for X, Y, Z in triples]}

    n = 300
    z = rng.integers(0, 3, n)
    x = rng.integers(0, 3, n)
    y = _noisy(rng, x, 3, 0.5)
    x1 = x.copy()
    x1[z == 0] = 1  # stratum z0: one non-empty row
    df = pd.DataFrame({"X": _lab(x1, "x", 3), "Y": _lab(y, "y", 3), "Z": _lab(z, "z", 3)})
    record("dof0_stratum", df, [("X", "Y", ["Z"]), ("Y", "X", ["Z"])], "X is constant where Z = z0")

    df = pd.DataFrame({"X": _lab(x, "x", 3), "Y": _lab(y, "y", 3), "X2": _lab(x, "x", 3), "K": _lab(np.zeros(n, dtype=int), "k", 1)})
    record("total_dof0", df, [("X", "Y", ["X2"]), ("X", "K", []), ("K", "Y", []), ("X", "K", ["Y"])],
           "X2 is a copy of X; K is constant")

    b1, b3 = rng.integers(0, 2, n), rng.integers(0, 2, n)
    b2 = _noisy(rng, b1, 2, 0.6)
    df = pd.DataFrame({"P": _lab(b1, "p", 2), "Q": _lab(b2, "q", 2), "R": _lab(b3, "r", 2), "T": _lab(z, "t", 3)})
    record("two_by_two", df, [("P", "Q", []), ("P", "Q", ["R"]), ("P", "Q", ["R", "T"]), ("Q", "R", ["P"]), ("P", "T", ["Q"])],
           "2 x 2 strata: the Yates correction")

    y0 = y.copy()
    y0[(x == 0) & (y0 == 2)] = 1  # the cell (x0, y2) is empty
    df = pd.DataFrame({"X": _lab(x, "x", 3), "Y": _lab(y0, "y", 3), "Z": _lab(z, "z", 3)})
    record("zero_cell", df, [("X", "Y", []), ("X", "Y", ["Z"]), ("Y", "X", [])], "the cell (x0, y2) never occurs")

    z2 = rng.integers(0, 2, n)
    z1 = z.copy()
    z1[(z1 == 2) & (z2 == 1)] = 0  # the configuration (z2, w1) never occurs
    df = pd.DataFrame({"X": _lab(x, "x", 3), "Y": _lab(y, "y", 3), "Z": _lab(z1, "z", 3), "W": _lab(z2, "w", 2)})
    record("missing_config", df, [("X", "Y", ["Z", "W"]), ("X", "Y", ["W", "Z"])], "(z2, w1) never occurs")

    df = pd.DataFrame({"X": _lab(x, "x", 3), "Y": _lab(y, "y", 3), "Z": _lab(z, "z", 3), "W": _lab(z2, "w", 2)})
    df.loc[rng.random(n) < 0.15, "Z"] = np.nan
    df.loc[rng.random(n) < 0.15, "W"] = np.nan
    record("nan_in_z", df, [("X", "Y", ["Z"]), ("X", "Y", ["Z", "W"]), ("X", "Y", [])], "NaN in the Z columns only")
    df = pd.DataFrame({"X": _lab(x, "x", 3), "Y": _lab(y, "y", 3)})
    df.loc[rng.random(n) < 0.15, "X"] = np.nan
    df.loc[rng.random(n) < 0.15, "Y"] = np.nan
    record("nan_no_z", df, [("X", "Y", [])], "NaN in X and Y, tested without Z")
    return out


# ---------------------------------------------------------------------------- alarm
def alarm_frame():
    import pandas as pd

    ref = G._model("alarm")
    nodes = sorted(ref.nodes())
    codes = np.load(os.path.join(HERE, "fit_alarm.npz"))["codes"]
    states = {v: list(ref.get_cpds(v).state_names[v]) for v in nodes}
    return pd.DataFrame({v: np.asarray(states[v], dtype=object)[codes[i]] for i, v in enumerate(nodes)})


def alarm():
    from pgmpy.estimators import PC

    df = alarm_frame()
    out = {}
    for variant in ("stable", "parallel"):
        skel, sep = PC(df).build_skeleton(variant=variant, ci_test="chi_square", significance_level=ALPHA, n_jobs=1,
                                          show_progress=False)
        out[variant] = {"edges": sorted(sorted(e) for e in skel.edges()),
                        "separating_set_sizes": sorted([sorted(k), len(v)] for k, v in sep.items())}
    # the reference's "stable" branch is its "orig" branch (BaseConstraintEstimator.py:200-245: both remove an
    # edge as soon as it is separated); only "parallel" tests a level against frozen neighbour sets
    return dict(out["stable"], parallel=out["parallel"])


def time_reference_pc():
    from pgmpy.estimators import PC

    df = alarm_frame()
    t0 = time.perf_counter()
    pdag = PC(df).estimate(variant="stable", ci_test="chi_square", significance_level=ALPHA, show_progress=False)
    print(json.dumps({"reference_pc_stable_s": time.perf_counter() - t0, "rows": len(df), "edges": len(pdag.edges())}))


# ---------------------------------------------------------------------------- PDAGs
PDAGS = [
    {"directed": [["A", "B"]], "undirected": [["B", "C"]]},                                        # R1
    {"directed": [["A", "B"], ["B", "C"]], "undirected": [["A", "C"]]},                            # R2
    {"directed": [["B", "D"], ["C", "D"]], "undirected": [["A", "B"], ["A", "C"], ["A", "D"]]},    # R3
    {"directed": [["D", "C"], ["C", "B"]], "undirected": [["A", "B"], ["A", "C"], ["A", "D"]]},    # R4
    {"directed": [], "undirected": [["A", "B"], ["B", "C"], ["C", "D"]]},                          # a chain: nothing
    {"directed": [["A", "C"], ["B", "C"]], "undirected": [["C", "D"], ["D", "E"]]},                # R1 twice
    {"directed": [["A", "B"]], "undirected": [["B", "C"], ["A", "C"]]},                            # shielded: nothing
    {"directed": [["A", "B"], ["C", "B"]], "undirected": [["C", "D"], ["D", "A"]]},                # the docstring's
    {"directed": [["A", "C"], ["B", "C"]], "undirected": [["C", "D"], ["C", "E"], ["D", "E"]]},
    {"directed": [["A", "B"], ["B", "C"]], "undirected": [["A", "C"], ["C", "D"], ["A", "D"]]},
    {"directed": [], "undirected": [["A", "B"], ["B", "C"], ["C", "A"], ["C", "D"]]},
    {"directed": [["A", "D"], ["B", "D"], ["D", "E"]], "undirected": [["E", "F"], ["F", "G"], ["A", "G"]]},
    {"directed": [], "undirected": [["A", "B"], ["B", "C"], ["C", "D"], ["D", "A"]]},              # a 4-cycle: no extension
]


def _colliders(arcs):
    """The unshielded colliders a -> c <- b of a list of arcs (adjacency: among these arcs and, for a PDAG's
    directed part, close enough: the fixtures' colliders are unshielded in the whole graph)."""
    arcs = {tuple(e) for e in arcs}
    adjacent = arcs | {(v, u) for u, v in arcs}
    return {(min(a, b), c, max(a, b)) for a, c in arcs for b, c2 in arcs if c2 == c and a != b and (a, b) not in adjacent}


def pdags():
    import logging

    from pgmpy.base import PDAG

    class Warned(logging.Handler):
        def __init__(self):
            super().__init__(logging.WARNING)
            self.hit = False

        def emit(self, record):
            self.hit = self.hit or "no faithful extension" in record.getMessage()

    logger = logging.getLogger("pgmpy")
    level = logger.level
    logger.setLevel(logging.WARNING)
    out = []
    for case in PDAGS:
        def make():
            return PDAG(directed_ebunch=[tuple(e) for e in case["directed"]],
                        undirected_ebunch=[tuple(e) for e in case["undirected"]])

        warned = Warned()
        logger.addHandler(warned)
        to_dag = sorted(list(e) for e in make().to_dag().edges())
        logger.removeHandler(warned)
        # no_extension: the reference warned that the PDAG has no consistent extension (its logger prints
        # the message once per process) or its DAG has other colliders than the PDAG: it oriented the
        # remaining edges as they came (set order), so only the skeleton of that result is comparable
        out.append(dict(case, meek=_pdag_record(make().apply_meeks_rules(apply_r4=False)),
                        meek_r4=_pdag_record(make().apply_meeks_rules(apply_r4=True)), to_dag=to_dag,
                        no_extension=bool(warned.hit or _colliders(to_dag) != _colliders(case["directed"]))))
    logger.setLevel(level)
    return out


# ---------------------------------------------------------------------------- chi2.sf
def sf_grid():
    from scipy import stats

    out = []
    for k in (1, 2, 3, 10, 100, 1000, 5000):
        xs = list(np.geomspace(1e-3 * k, 20.0 * k, 120))
        xs += [float(stats.chi2.isf(p, k)) for p in (1e-20, 1e-50, 1e-100, 1e-150, 1e-200, 1e-250, 1e-290, 1e-299)]
        xs += [float(k), float(k) + 2.0, max(float(k) - 2.0, 0.5)]  # either side of the series / fraction switch
        for x in xs:
            out.append([k, float(x), float(stats.chi2.sf(x, k))])
    return out


def main():
    G._setup()
    if "--time-pc" in sys.argv:
        return time_reference_pc()
    df = frame_s()
    out = {"s": {"frame": {c: df[c].tolist() for c in df.columns}, "seed": S_SEED, "alpha": ALPHA,
                 "tests": all_tests(df), "pc": pc_on_s(df)},
           "edge": edge_frames(), "alarm": alarm(), "pdags": pdags(), "sf_grid": sf_grid()}
    from tests import ci_cases as C

    meta, arrays = C.pack_golden(out)
    G._dump("ci_cases.json", meta)
    np.savez_compressed(os.path.join(HERE, "ci_cases.npz"), **arrays)


if __name__ == "__main__":
    main()
