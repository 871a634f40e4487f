#!/usr/bin/env python3
"""Generate tests/golden/lgs_cases.json + lgs_cases.npz by running the REFERENCE's pearsonr and its PC with
ci_test="pearsonr" on small dyadic frames.

    PYTHONHASHSEED=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lgs.py

Frames are drawn from known linear-Gaussian DAGs with strong effects (|beta| >= 0.75 on unit noise) and rounded to
multiples of 2^-10, so that every value is a short dyadic number:
  chain4     a -> b -> c -> d
  collider5  a -> c <- b, c -> d, c -> e <- b
  fork6      r -> s, r -> t, s -> u <- t, u -> v, w alone
Per frame: the reference's pearsonr(..., boolean=False) for a list of (X, Y, Z) triples, and PC(...).estimate with
ci_test="pearsonr" for the variants "orig" and "stable": skeleton, separating sets and PDAG.  A second run of each
estimate with a recording wrapper around the reference's own pearsonr collects the p-value of every decision; the
maker REFUSES a frame (and tries its next seed) when a decision's p-value lies within a factor MARGIN = 10 of the
significance level, when the two runs disagree, when the "stable" skeleton is not the generating DAG's, or when
"orig" (whose result depends on the reference's hash order) and "stable" differ in skeleton or PDAG.  The smallest
margin met is recorded.  statsmodels is a mock where the goldens are made, so the reference's Gaussian scores
cannot be recorded (tests/lgs_cases.py pins their closed form instead).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402

N_ROWS = 500
ALPHA, MARGIN = 0.01, 10.0
DAGS = {
    "chain4": {"nodes": ["a", "b", "c", "d"], "edges": [("a", "b", 1.0), ("b", "c", -0.75), ("c", "d", 1.25)]},
    "collider5": {"nodes": ["a", "b", "c", "d", "e"],
                  "edges": [("a", "c", 1.0), ("b", "c", -1.0), ("c", "d", 0.75), ("c", "e", 1.0), ("b", "e", 1.5)]},
    "fork6": {"nodes": ["r", "s", "t", "u", "v", "w"],
              "edges": [("r", "s", 1.0), ("r", "t", 1.25), ("s", "u", 1.0), ("t", "u", 1.0), ("u", "v", -0.75)]},
}


def draw(spec, seed):
    import pandas as pd

    rng = np.random.default_rng(seed)
    cols = {}
    for v in spec["nodes"]:  # the nodes are listed in a topological order
        x = rng.standard_normal(N_ROWS) + 0.5 * (len(cols) % 3 - 1)
        for a, b, w in spec["edges"]:
            if b == v:
                x = x + w * cols[a]
        cols[v] = x
    return pd.DataFrame({v: np.round(cols[v] * 1024) / 1024 for v in spec["nodes"]})


def triples(nodes):
    out = [(nodes[0], nodes[1], []), (nodes[0], nodes[-1], []), (nodes[0], nodes[2], [nodes[1]]),
           (nodes[1], nodes[3], [nodes[2]]), (nodes[0], nodes[3], [nodes[1], nodes[2]]),
           (nodes[-1], nodes[0], list(nodes[1:-1]))]
    return out


def pc_record(df, variant, log):
    from pgmpy.estimators import PC
    from pgmpy.estimators import CITests as RC

    def recording(X, Y, Z, data, boolean=True, **kw):
        coef, p = RC.pearsonr(X, Y, Z, data, boolean=False)
        log.append(float(p))
        return p >= kw["significance_level"]

    def run(ci_test):
        skel, seps = PC(df).estimate(variant=variant, ci_test=ci_test, return_type="skeleton", significance_level=ALPHA,
                                     n_jobs=1, show_progress=False)
        pdag = PC(df).estimate(variant=variant, ci_test=ci_test, return_type="pdag", significance_level=ALPHA, n_jobs=1,
                               show_progress=False)
        return {"skeleton": sorted(sorted(e) for e in skel.edges()),
                "separating_sets": sorted([sorted(k), sorted(v)] for k, v in seps.items()),
                "directed": sorted(list(e) for e in pdag.directed_edges),
                "undirected": sorted(sorted(e) for e in pdag.undirected_edges)}

    named = run("pearsonr")
    if run(recording) != named:
        return None
    return named


def main():
    make_golden._setup()
    from pgmpy.estimators import CITests as RC

    out = {"what": "the reference's pearsonr and PC(ci_test='pearsonr') on dyadic frames; see make_golden_lgs.py",
           "n_rows": N_ROWS, "significance_level": ALPHA, "margin_required": MARGIN, "frames": {}, "pearsonr": {}, "pc": {}}
    arrays, smallest = {}, np.inf
    for name, spec in DAGS.items():
        skeleton = sorted(sorted((a, b)) for a, b, _ in spec["edges"])
        for seed in range(100, 140):
            df = draw(spec, seed)
            log, pcs = [], {}
            for variant in ("orig", "stable"):
                pcs[variant] = pc_record(df, variant, log)
            if any(v is None for v in pcs.values()) or pcs["stable"]["skeleton"] != skeleton:
                continue
            # "orig" removes edges as it goes, in the reference in hash order: only a frame on which that order does
            # not matter can be compared with a walk in column order
            if any(pcs["orig"][k] != pcs["stable"][k] for k in ("skeleton", "directed", "undirected")):
                continue
            margin = min(max(p / ALPHA, ALPHA / max(p, 1e-300)) for p in log)
            if margin < MARGIN:
                print(f"{name} seed {seed}: margin {margin:.3g}, refused")
                continue
            break
        else:
            raise SystemExit(f"{name}: no seed gives the margin")
        print(f"{name}: seed {seed}, {len(log)} decisions, margin {margin:.3g}")
        smallest = min(smallest, margin)
        arrays[f"{name}_frame"] = df.to_numpy(dtype=np.float64)
        out["frames"][name] = {"columns": list(df.columns), "seed": seed, "edges": [[a, b] for a, b, _ in spec["edges"]],
                               "decisions": len(log), "margin": margin}
        out["pc"][name] = pcs
        out["pearsonr"][name] = []
        for X, Y, Z in triples(spec["nodes"]):
            coef, p = RC.pearsonr(X, Y, Z, df, boolean=False)
            out["pearsonr"][name].append({"X": X, "Y": Y, "Z": Z, "coef": float(coef), "p": float(p)})
    out["smallest_margin"] = smallest
    make_golden._dump("lgs_cases.json", out)
    path = os.path.join(HERE, "lgs_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main()
