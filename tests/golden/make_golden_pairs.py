#!/usr/bin/env python3
"""Generate tests/golden/pair_cases.json by running the REFERENCE's TreeSearch (with scikit-learn's scores).

    PYTHONHASHSEED=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pairs.py

Frames (integer state codes as the cell values, so the tests rebuild them from the committed arrays):
  net5     metrics_cases.npz net5_codes1000, columns v0 .. v4, class v4
  alarm    the 1,000 alarm rows of fit_alarm.npz, columns a00 .. a36, class a05 (three states)
  const    the first 200 rows of net5 plus a constant column k
  twins    the first 200 rows of net5 plus a copy t of v1
  tworows  the first 2 rows of net5's v0 .. v2
For each frame and each of the three named weightings: the matrix of _get_weights; for mutual_info also
_get_conditional_weights; and, for net5 and alarm (all weightings) and const (mutual_info), the edge sets of
estimate("chow-liu") with a given root and with the root auto-picked, and of estimate("tan").

An edge set is only as stable as the gaps between the weights it was chosen by, so each one is recorded
with its tree margin (the smallest gap between a non-tree edge and the lightest tree edge on the cycle it
closes) and, where the root was auto-picked, its root gap (largest minus second largest column sum); a
case whose margin is below MIN_MARGIN is refused.  The twins and tworows frames are full of exact ties:
only their weight matrices are recorded.
"""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

MIN_MARGIN = 1e-6
KINDS = ("mutual_info", "normalized_mutual_info", "adjusted_mutual_info")


def frames():
    import pandas as pd

    net5 = np.load(os.path.join(HERE, "metrics_cases.npz"))["net5_codes1000"]
    alarm = np.load(os.path.join(HERE, "fit_alarm.npz"))["codes"]
    f5 = pd.DataFrame(net5.T.astype(np.int64), columns=[f"v{j}" for j in range(net5.shape[0])])
    fa = pd.DataFrame(alarm.T.astype(np.int64), columns=[f"a{j:02d}" for j in range(alarm.shape[0])])
    const = f5.iloc[:200].copy()
    const["k"] = 0
    twins = f5.iloc[:200].copy()
    twins["t"] = twins["v1"]
    return {"net5": (f5, "v4", "v0", True), "alarm": (fa, "a05", "a00", True), "const": (const, "v4", "v0", True),
            "twins": (twins, None, None, False), "tworows": (f5.iloc[:2, :3].copy(), None, None, False)}


def tree_margin(weights, columns, edges):
    """The smallest gap between a non-tree pair's weight and the lightest tree edge on its cycle."""
    import networkx as nx

    T = nx.Graph()
    T.add_nodes_from(columns)
    idx = {c: i for i, c in enumerate(columns)}
    for u, v in edges:
        T.add_edge(u, v, weight=weights[idx[u], idx[v]])
    margin = float("inf")
    for u, v in itertools.combinations(columns, 2):
        if T.has_edge(u, v) or not nx.has_path(T, u, v):
            continue
        path = nx.shortest_path(T, u, v)
        lightest = min(T[a][b]["weight"] for a, b in zip(path, path[1:]))
        margin = min(margin, lightest - weights[idx[u], idx[v]])
    return margin


def root_gap(weights):
    s = np.sort(weights.sum(axis=0))
    return float(s[-1] - s[-2])


def main():
    make_golden._setup()
    from pgmpy.estimators import TreeSearch

    out = {"what": "weights and edge sets of the reference's TreeSearch (scikit-learn scores); see make_golden_pairs.py",
           "min_margin": MIN_MARGIN, "cases": {}}
    for name, (df, class_node, root, with_edges) in frames().items():
        columns = list(df.columns)
        case = {"columns": columns, "class_node": class_node, "root": root, "weights": {}, "estimates": {}}
        for kind in KINDS:
            w = TreeSearch._get_weights(df, kind, n_jobs=1, show_progress=False)
            case["weights"][kind] = w.tolist()
            if not with_edges or (name == "const" and kind != "mutual_info"):
                continue
            est = {}
            given = TreeSearch(df, root_node=root, n_jobs=1).estimate("chow-liu", edge_weights_fn=kind, show_progress=False)
            auto_search = TreeSearch(df, n_jobs=1)
            auto = auto_search.estimate("chow-liu", edge_weights_fn=kind, show_progress=False)
            est["chow-liu"] = {"edges": sorted(map(list, given.edges())), "nodes": sorted(given.nodes()),
                               "margin": tree_margin(w, columns, given.edges())}
            est["chow-liu-auto"] = {"edges": sorted(map(list, auto.edges())), "nodes": sorted(auto.nodes()),
                                    "root": auto_search.root_node, "margin": tree_margin(w, columns, auto.edges()),
                                    "root_gap": root_gap(w)}
            cw = TreeSearch._get_conditional_weights(df, class_node, kind, n_jobs=1, show_progress=False)
            tan = TreeSearch(df, root_node=root, n_jobs=1).estimate("tan", class_node=class_node, edge_weights_fn=kind,
                                                                   show_progress=False)
            k = columns.index(class_node)
            reduced = columns[:k] + columns[k + 1:]
            cwr = np.delete(np.delete(cw, k, axis=0), k, axis=1)
            tree_edges = [e for e in tan.edges() if e[0] != class_node]
            est["tan"] = {"edges": sorted(map(list, tan.edges())), "nodes": sorted(tan.nodes()),
                          "margin": tree_margin(cwr, reduced, tree_edges)}
            if kind == "mutual_info":
                case["conditional_weights"] = cw.tolist()
            for what, e in est.items():
                print(f"{name} {kind} {what}: margin {e['margin']:.3g}" + (f" root gap {e['root_gap']:.3g}" if "root_gap" in e else ""))
                if e["margin"] < MIN_MARGIN:
                    raise SystemExit(f"{name} {kind} {what}: tree margin {e['margin']:.3g} < {MIN_MARGIN}: rounding could flip an edge")
            case["estimates"][kind] = est
        if not with_edges:
            pass
        out["cases"][name] = case
    make_golden._dump("pair_cases.json", out)


if __name__ == "__main__":
    main()
