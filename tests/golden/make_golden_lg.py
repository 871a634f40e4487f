#!/usr/bin/env python3
"""Generate tests/golden/lg_cases.json + lg_cases.npz by running the REFERENCE's LinearGaussianBayesianNetwork
(scikit-learn regressions, scipy logpdf, numpy draws).

    PYTHONHASHSEED=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lg.py

Models with dyadic parameters (beta in {+-0.25, +-0.5, +-1, 2} and small integers for the reference's own
docstring model, std in {0.5, 1, 2, 3, 4}, depth <= 3), so that the reference's rounding of to_joint_gaussian to
8 decimals changes nothing: the maker ASSERTS that the rounded result equals the unrounded formula exactly and
refuses the case otherwise.
  chain3     x1 -> x2 -> x3, the reference's docstring model
  collider5  a -> c <- b, c -> d, c -> e <- b
  dense6     two roots, two nodes on both, two nodes on (nearly) all four
Per model: node and topological orders, to_joint_gaussian, a frame simulated by the reference (N_ROWS rows, in
the npz), its log_likelihood with kappa(cov) for the host bound, predict for two missing-sets on 8 rows, fit with
both std_estimators, and per family kappa of the correlation-scaled centred parent Gram matrix and S_vv / rss
(cases with kappa > 1e4 or S_vv / rss > 1e3 are refused).
Further: shifted (chain3's frame + 1e8 on x2), twins (x2 on x1 and a copy of x1: the reference's min-norm
coefficients), tworows (n = 2), onerow (a root on one row: NaN std), the str() of three CPDs, and
get_random(n_nodes = 5, seed = 7): its graph and CPD values (the reference draws the graph WITHOUT the seed, so this
entry alone differs from run to run; the test rebuilds the recorded graph and compares the seeded CPDs).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402

N_ROWS = 1000
MAX_KAPPA, MAX_SVV_RSS = 1e4, 1e3

MODELS = {
    "chain3": {"nodes": ["x1", "x2", "x3"], "edges": [["x1", "x2"], ["x2", "x3"]],
               "cpds": [("x1", [1], 4, []), ("x2", [-5, 0.5], 4, ["x1"]), ("x3", [4, -1], 3, ["x2"])],
               "missing": [["x3"], ["x1", "x3"]], "seed": 11},
    "collider5": {"nodes": ["a", "b", "c", "d", "e"], "edges": [["a", "c"], ["b", "c"], ["c", "d"], ["c", "e"], ["b", "e"]],
                  "cpds": [("a", [0.5], 1, []), ("b", [-1], 2, []), ("c", [0.25, 0.5, -0.25], 0.5, ["a", "b"]),
                           ("d", [2, 1], 1, ["c"]), ("e", [-0.5, -1, 0.5], 3, ["c", "b"])],
                  "missing": [["c"], ["a", "d", "e"]], "seed": 12},
    "dense6": {"nodes": ["u5", "u0", "u3", "u1", "u4", "u2"],
               "edges": [["u0", "u2"], ["u1", "u2"], ["u0", "u3"], ["u1", "u3"], ["u0", "u4"], ["u1", "u4"], ["u2", "u4"],
                         ["u3", "u4"], ["u0", "u5"], ["u2", "u5"], ["u3", "u5"]],
               "cpds": [("u0", [1], 2, []), ("u1", [-0.5], 1, []), ("u2", [0.25, 0.5, -1], 0.5, ["u0", "u1"]),
                        ("u3", [-1, -0.25, 2], 4, ["u0", "u1"]), ("u4", [0.5, 1, -0.5, 0.25, -0.25], 1, ["u0", "u1", "u2", "u3"]),
                        ("u5", [2, -1, 0.5, 0.25], 3, ["u0", "u2", "u3"])],
               "missing": [["u4"], ["u0", "u5"]], "seed": 13},
}


def ref_model(spec):
    from pgmpy.factors.continuous import LinearGaussianCPD
    from pgmpy.models import LinearGaussianBayesianNetwork

    m = LinearGaussianBayesianNetwork()
    m.add_nodes_from(spec["nodes"])
    m.add_edges_from([tuple(e) for e in spec["edges"]])
    for v, beta, std, ev in spec.get("cpds", []):
        m.add_cpds(LinearGaussianCPD(v, beta, std, list(ev)))
    return m


def unrounded_joint(m):
    import networkx as nx

    order = list(nx.topological_sort(m))
    pos = {v: i for i, v in enumerate(order)}
    n = len(order)
    mean, B, om = np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
    for v in order:
        c = m.get_cpds(v)
        mean[pos[v]] = (c.beta * np.array([1.0] + [mean[pos[u]] for u in c.evidence])).sum()
        for i, u in enumerate(c.evidence):
            B[pos[u], pos[v]] = c.beta[i + 1]
        om[pos[v], pos[v]] = c.std ** 2
    inv = np.linalg.inv(np.eye(n) - B)
    return order, mean, inv.T @ om @ inv


def cpd_list(m):
    return [{"variable": c.variable, "beta": [float(b) for b in c.beta], "std": float(c.std), "evidence": list(c.evidence)}
            for c in m.cpds]


def fit_record(spec, df, name, refuse=True):
    """The reference's fit with both std estimators, and each family's condition figures."""
    from tests import lg_cases as LC

    out = {}
    for est in ("unbiased", "mle"):
        m = ref_model({"nodes": spec["nodes"], "edges": spec["edges"]})
        m.fit(df, std_estimator=est)
        out[est] = cpd_list(m)
    cols = list(df.columns)
    X = np.ascontiguousarray(df.to_numpy(dtype=np.float64).T)
    idx = list(range(len(cols)))
    shift = LC.colmean(X, idx)
    G, _ = LC.gram_ld(X, idx, shift)
    cond = {}
    for c in out["unbiased"]:
        parents = [cols.index(u) for u in c["evidence"]]
        with np.errstate(all="ignore"):
            kappa, ratio = LC.family_condition(G, shift, cols.index(c["variable"]), parents)
        cond[c["variable"]] = {"kappa": kappa, "svv_over_rss": ratio}
        print(f"{name} {c['variable']}: kappa {kappa:.3g} S_vv/rss {ratio:.3g}")
        if refuse and (not kappa <= MAX_KAPPA or not ratio <= MAX_SVV_RSS):
            raise SystemExit(f"{name} {c['variable']}: kappa {kappa:.3g} / S_vv/rss {ratio:.3g} above the limits")
    out["condition"] = cond
    return out


def main():
    make_golden._setup()
    from pgmpy.factors.continuous import LinearGaussianCPD
    from pgmpy.models import LinearGaussianBayesianNetwork

    out = {"what": "the reference's LinearGaussianBayesianNetwork on dyadic models; see make_golden_lg.py", "n_rows": N_ROWS,
           "models": {}, "frames": {}}
    arrays = {}
    for name, spec in MODELS.items():
        m = ref_model(spec)
        mean_r, cov_r = m.to_joint_gaussian()
        order, mean, cov = unrounded_joint(m)
        if not (np.array_equal(mean_r, mean) and np.array_equal(cov_r, cov)):
            raise SystemExit(f"{name}: the reference's rounding changes to_joint_gaussian")
        df = m.simulate(n_samples=N_ROWS, seed=spec["seed"])
        arrays[f"{name}_frame"] = df.to_numpy(dtype=np.float64)
        out["frames"][name] = list(df.columns)
        case = {"nodes": list(m.nodes()), "edges": spec["edges"], "order": order, "cpds": cpd_list(m), "mean": mean.tolist(),
                "cov": cov.tolist(), "kappa_cov": float(np.linalg.cond(cov)), "log_likelihood": float(m.log_likelihood(df)),
                "predict": [], "fit": fit_record(spec, df, name)}
        for missing in spec["missing"]:
            part = df.iloc[:8].drop(columns=missing)
            mv, mu, cc = m.predict(part)
            case["predict"].append({"missing": missing, "variables": list(mv), "mu": np.asarray(mu).tolist(),
                                    "cov": np.asarray(cc).tolist()})
        # simulate(do) / simulate(evidence): the distribution the samples must have, from the reference's own formulas
        do_var, ev_var = spec["missing"][0][0], order[0]
        md = m.copy()
        # the intervened model written out by hand (the node leaves, its children's intercepts take beta * value),
        # and the reference's joint of it
        cut = {"nodes": [v for v in spec["nodes"] if v != do_var], "edges": [e for e in spec["edges"] if do_var not in e], "cpds": []}
        for v, beta, std, evid in spec["cpds"]:
            if v == do_var:
                continue
            beta, evid = list(beta), list(evid)
            if do_var in evid:
                k = evid.index(do_var)
                beta[0] += beta.pop(k + 1) * 1.5
                evid.pop(k)
            cut["cpds"].append((v, beta, std, evid))
        mc = ref_model(cut)
        import networkx as nx

        cm, cc = mc.to_joint_gaussian()
        sim = m.simulate(n_samples=4, do={do_var: 1.5}, seed=1)
        case["do"] = {"do": {do_var: 1.5}, "variables": list(nx.topological_sort(mc)), "mean": cm.tolist(), "cov": cc.tolist(),
                      "columns": list(sim.columns)}
        ev = {ev_var: 0.75}
        import pandas as pd

        mv, mu, cc = md.predict(pd.DataFrame([ev]))
        case["evidence"] = {"evidence": ev, "variables": list(mv), "mean": np.asarray(mu)[0].tolist(), "cov": np.asarray(cc).tolist(),
                            "columns": list(m.simulate(n_samples=4, evidence=ev, seed=1).columns)}
        out["models"][name] = case

    chain = MODELS["chain3"]
    df = pd.DataFrame(arrays["chain3_frame"], columns=out["frames"]["chain3"])
    shifted = df.copy()
    shifted["x2"] = shifted["x2"] + 1e8
    out["shifted"] = fit_record(chain, shifted, "shifted")
    twins = df[["x1", "x2"]].copy()
    twins["x1b"] = twins["x1"]
    tw_spec = {"nodes": ["x1", "x1b", "x2"], "edges": [["x1", "x2"], ["x1b", "x2"]]}
    out["twins"] = {"spec": tw_spec, "fit": fit_record(tw_spec, twins, "twins", refuse=False)}
    out["tworows"] = fit_record(chain, df.iloc[:2].copy(), "tworows", refuse=False)
    one_spec = {"nodes": ["x1"], "edges": []}
    out["onerow"] = {"spec": one_spec, "fit": fit_record(one_spec, df.iloc[:1][["x1"]].copy(), "onerow", refuse=False)}

    m = ref_model(chain)
    fitted = ref_model({"nodes": chain["nodes"], "edges": chain["edges"]}).fit(df)
    out["strings"] = [{"cpd": c, "str": str(LinearGaussianCPD(c["variable"], c["beta"], c["std"], c["evidence"]))}
                      for c in cpd_list(m)[:2] + cpd_list(fitted)[2:]]
    r = LinearGaussianBayesianNetwork.get_random(n_nodes=5, seed=7)
    out["get_random"] = {"seed": 7, "nodes": list(r.nodes()), "edges": [list(e) for e in r.edges()], "cpds": cpd_list(r)}
    c = LinearGaussianCPD.get_random("Income", ["Age", "Experience"], loc=2.0, scale=0.5, seed=5)
    out["cpd_get_random"] = {"variable": "Income", "evidence": ["Age", "Experience"], "loc": 2.0, "scale": 0.5, "seed": 5,
                             "beta": [float(b) for b in c.beta], "std": float(c.std)}
    make_golden._dump("lg_cases.json", out)
    path = os.path.join(HERE, "lg_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main()
