#!/usr/bin/env python3
"""Generate the metrics fixtures by running the REFERENCE (pgmpy/metrics/metrics.py, bn_inference.py).

    PYTHONHASHSEED=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py [--time]

Same set-up as make_golden_fit.py (make_golden._setup(): the reference and the offline shims on sys.path).
Writes data only:

  metrics_cases.json  the 5-node network "net5" (edges, state names, CPD values [card, parent
                      configurations] with the parents in the CPD's order), its score and
                      log_likelihood_score on 200 rows; on 1,000 rows, for the true DAG and for the DAG
                      with two edges removed: correlation_score (summary and F1, chi_square at 0.05),
                      fisher_c (p-value and RMSEA, chi_square) and SHD against the true DAG; alarm's score and
                      log_likelihood_score on the 1,000 rows of fit_alarm.npz; is_dconnected for every
                      pair given nothing, C and E; scipy's chi2.sf at 2 k degrees of freedom, k = 1, 7, 500, 5000
  metrics_cases.npz   net5_codes200 / net5_codes1000 (uint8 [5, n], nodes sorted, codes into the state
                      names of the json), net5_logp200 and alarm_logp (BayesianModelProbability.log_probability)

The generator stops with an error when a pairwise p-value lies within a factor of 2 of the significance
level (a rounding difference could flip a label) or when a state of a variable is unobserved in the 1,000
rows (a known deviation of the CI tests).  --time prints the reference's wall time for log_probability
on the 1,000 alarm rows and writes nothing.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as G  # noqa: E402

EDGES = [("A", "C"), ("B", "C"), ("C", "D"), ("A", "E"), ("D", "E")]
REMOVED = [("A", "E"), ("C", "D")]  # the second DAG lacks these two edges
CARDS = {"A": 2, "B": 3, "C": 2, "D": 3, "E": 2}
SIGNIFICANCE = 0.05


def net5():
    from pgmpy.factors.discrete import TabularCPD
    from pgmpy.models import DiscreteBayesianNetwork

    rng = np.random.default_rng(21)
    m = DiscreteBayesianNetwork(EDGES)
    states = {v: [f"{v.lower()}{s}" for s in range(k)] for v, k in CARDS.items()}
    for v in sorted(CARDS):
        parents = sorted(m.get_parents(v))
        # far from uniform, so that dependent pairs are detected with p-values far below the level
        t = rng.dirichlet(np.full(CARDS[v], 0.6), size=int(np.prod([CARDS[p] for p in parents], dtype=int))).T
        t = np.maximum(t, 0.02)
        t = t / t.sum(axis=0, keepdims=True)
        m.add_cpds(TabularCPD(v, CARDS[v], t, evidence=parents or None, evidence_card=[CARDS[p] for p in parents] or None,
                              state_names={u: states[u] for u in [v] + parents}))
    m.check_model()
    return m, states


def codes_of(df, states):
    nodes = sorted(states)
    return np.stack([np.array([states[v].index(s) for s in df[v]], dtype=np.uint8) for v in nodes])


def alarm_case():
    import pandas as pd

    ref = G._model("alarm")
    nodes = sorted(ref.nodes())
    codes = np.load(os.path.join(HERE, "fit_alarm.npz"))["codes"]
    states = {v: list(ref.get_cpds(v).state_names[v]) for v in nodes}
    df = pd.DataFrame({v: np.asarray(states[v], dtype=object)[codes[i]] for i, v in enumerate(nodes)})
    return ref, df


def main():
    G._setup()
    from pgmpy.estimators.CITests import chi_square
    from pgmpy.metrics import SHD, BayesianModelProbability, correlation_score, fisher_c, log_likelihood_score
    from pgmpy.models import DiscreteBayesianNetwork
    from pgmpy.sampling import BayesianModelSampling

    ref, adf = alarm_case()
    if "--time" in sys.argv:
        bmp = BayesianModelProbability(ref)
        t0 = time.perf_counter()
        bmp.log_probability(adf)
        print(f"reference log_probability, alarm, 1,000 rows: {time.perf_counter() - t0:.3f} s")
        return

    m, states = net5()
    nodes = sorted(states)
    sampler = BayesianModelSampling(m)
    d200 = sampler.forward_sample(size=200, seed=5, show_progress=False)[nodes]
    d1000 = sampler.forward_sample(size=1000, seed=13, show_progress=False)[nodes]  # passes the checks below (6 does not)
    for v in nodes:
        if set(d1000[v]) != set(states[v]) or set(d200[v]) != set(states[v]):
            raise SystemExit(f"a state of {v} is unobserved in the sampled rows: choose another seed")
    from itertools import combinations

    for u, v in combinations(nodes, 2):
        p = chi_square(X=u, Y=v, Z=[], data=d1000, boolean=False)[1]
        if SIGNIFICANCE / 2 <= p <= SIGNIFICANCE * 2:
            raise SystemExit(f"the p-value of ({u}, {v}) is {p}: within a factor of 2 of {SIGNIFICANCE}; choose another seed")

    bmp = BayesianModelProbability(m)
    out = {"nodes": nodes, "edges": EDGES, "removed": REMOVED, "states": states, "significance_level": SIGNIFICANCE,
           "cpds": {v: {"variables": list(m.get_cpds(v).variables),
                        "values": np.asarray(m.get_cpds(v).get_values(), dtype=np.float64).tolist()} for v in nodes},
           "score200": float(bmp.score(d200)), "loglik200": float(log_likelihood_score(m, d200)),
           "score200_array": float(bmp.score(d200[nodes[::-1]].values, ordering=nodes[::-1]))}
    arrays = {"net5_codes200": codes_of(d200, states), "net5_codes1000": codes_of(d1000, states),
              "net5_logp200": np.asarray(bmp.log_probability(d200), dtype=np.float64)}

    pruned = DiscreteBayesianNetwork([e for e in EDGES if e not in REMOVED])
    pruned.add_nodes_from(nodes)
    out["dags"] = {}
    for name, dag in (("true", m), ("pruned", pruned)):
        summary = correlation_score(dag, d1000, test="chi_square", significance_level=SIGNIFICANCE, return_summary=True)
        p, rmsea = fisher_c(dag, d1000, ci_test=chi_square, compute_rmsea=True, show_progress=False)
        out["dags"][name] = {
            "edges": [list(e) for e in dag.edges()],
            "f1": float(correlation_score(dag, d1000, test="chi_square", significance_level=SIGNIFICANCE)),
            "summary": {"var1": summary["var1"].tolist(), "var2": summary["var2"].tolist(),
                        "stat_test": [bool(x) for x in summary["stat_test"]],
                        "d_connected": [bool(x) for x in summary["d_connected"]]},
            "fisher_p": float(p), "fisher_rmsea": float(rmsea), "shd_to_true": int(SHD(m, dag)),
            "dconnected": [[u, v, z, bool(dag.is_dconnected(u, v, observed=z))]
                           for u, v in combinations(nodes, 2) for z in ([], ["C"], ["E"]) if u not in z and v not in z],
        }
    reversed_dag = DiscreteBayesianNetwork([("C", "A"), ("B", "C"), ("C", "D"), ("A", "E"), ("E", "D")])
    out["shd_reversed"] = {"edges": [list(e) for e in reversed_dag.edges()], "shd": int(SHD(m, reversed_dag))}

    # the survival function fisher_c ends in, at the even degree of freedom 2 k (scipy's chi2.sf, not 1 - cdf)
    from scipy import stats

    out["chi2_sf"] = [{"k": k, "C": float(f * k), "sf": float(stats.chi2.sf(f * k, 2 * k))}
                      for k in (1, 7, 500, 5000) for f in (0.5, 1.0, 2.0, 2.2, 3.0)]

    abmp = BayesianModelProbability(ref)
    arrays["alarm_logp"] = np.asarray(abmp.log_probability(adf), dtype=np.float64)
    out["alarm_score"] = float(abmp.score(adf))
    out["alarm_loglik"] = float(log_likelihood_score(ref, adf))

    G._dump("metrics_cases.json", out)
    path = os.path.join(HERE, "metrics_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main()
