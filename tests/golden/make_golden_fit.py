#!/usr/bin/env python3
"""Generate the parameter-learning fixtures by running the REFERENCE estimators.

    PYTHONHASHSEED=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fit.py

Same set-up as make_golden.py (its _setup(): the reference and the offline shims on sys.path).  Writes

  fit_cases.json   cases (a)-(d): input frames, state names, and for every estimator call the reference's
                   state_counts tables (values, index, columns) and CPDs (variables, cardinalities, state
                   names, values); fit_update's CPDs for case (a)
  fit_alarm.npz    case (e): 1,000 forward-sampled alarm rows as uint8 codes [37, 1000] (nodes sorted,
                   pgmpy_amd.utils.sampling.forward_sample_codes, seed 11) and, for MLE and BDeu on all
                   rows and MLE on each half, the count tables and CPD values of all 37 families laid
                   end to end in sorted-node order (each [node_card, prod(parent_card)], parents sorted)

NaN cells are stored as null; every float is written with repr precision (json round-trips float64).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as G  # noqa: E402


def _py(x):
    """A JSON-able scalar: numpy scalars unwrapped, NaN -> None."""
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return None if np.isnan(x) else float(x)
    return x


def _frame(df):
    return {str(c): [_py(v) for v in df[c].tolist()] for c in df.columns}


def _cpd(cpd):
    return {"variables": list(cpd.variables), "cardinality": [int(c) for c in cpd.cardinality],
            "state_names": {v: [_py(s) for s in cpd.state_names[v]] for v in cpd.variables},
            "values": np.asarray(cpd.get_values(), dtype=np.float64).tolist()}


def _counts(sc):
    cols = [list(c) if isinstance(c, tuple) else [c] for c in sc.columns.tolist()]
    return {"values": np.asarray(sc, dtype=np.float64).tolist(), "index": [_py(s) for s in sc.index.tolist()],
            "index_name": sc.index.name, "columns": [[_py(x) for x in c] for c in cols],
            "column_names": list(sc.columns.names)}


def _estimate(model_edges, nodes, df, estimator, state_names=None, weighted=False, **kwargs):
    """The reference's CPDs (get_parameters and estimate_cpd must agree) and state_counts per node."""
    from pgmpy.estimators import BayesianEstimator, MaximumLikelihoodEstimator
    from pgmpy.models import DiscreteBayesianNetwork

    m = DiscreteBayesianNetwork(model_edges)
    m.add_nodes_from(nodes)
    cls = {"mle": MaximumLikelihoodEstimator, "bayes": BayesianEstimator}[estimator]
    est = cls(m, df, **({"state_names": state_names} if state_names is not None else {}))
    cpds = est.get_parameters(weighted=weighted, **kwargs)
    out = {"cpds": {c.variable: _cpd(c) for c in cpds}, "node_order": [c.variable for c in cpds], "counts": {}}
    for n in nodes:
        out["counts"][n] = _counts(est.state_counts(n, weighted=weighted))
        per = {k: (v[n] if isinstance(v, dict) else v) for k, v in kwargs.items()}
        one = est.estimate_cpd(n, weighted=weighted, **per)
        assert np.array_equal(np.asarray(one.get_values()), np.asarray(out["cpds"][n]["values"]), equal_nan=True)
    return out


def case_a():
    import pandas as pd
    from pgmpy.estimators import BayesianEstimator
    from pgmpy.models import DiscreteBayesianNetwork

    df = pd.DataFrame(data={"A": [0, 0, 1], "B": [0, 1, 0], "C": [1, 1, 0]})
    edges, nodes = [("A", "C"), ("B", "C")], ["A", "B", "C"]
    out = {"frame": _frame(df), "edges": edges, "nodes": nodes,
           "mle": _estimate(edges, nodes, df, "mle"),
           "bdeu5": _estimate(edges, nodes, df, "bayes", prior_type="BDeu", equivalent_sample_size=5)}
    m = DiscreteBayesianNetwork(edges)
    m.fit(df, estimator=BayesianEstimator, prior_type="BDeu", equivalent_sample_size=5)
    m.fit_update(df, n_prev_samples=10)
    out["fit_update10"] = {c.variable: _cpd(c) for c in m.get_cpds()}
    c = np.asarray(out["mle"]["cpds"]["C"]["values"])
    assert np.array_equal(c, [[0, 0, 1, .5], [1, 1, 0, .5]])
    assert np.allclose(out["bdeu5"]["cpds"]["C"]["values"][0], [.2778, .2778, .7222, .5], atol=5e-5)
    assert np.allclose(out["fit_update10"]["C"]["values"][0], [.2525, .2525, .7475, .5], atol=5e-5)
    # reindex=False on the family with an unseen parent configuration
    from pgmpy.estimators import ParameterEstimator

    out["counts_C_noreindex"] = _counts(ParameterEstimator(DiscreteBayesianNetwork(edges), df)
                                        .state_counts("C", reindex=False))
    return out


def frame_b():
    """200 rows, string and float states, about 20 % NaN per column."""
    import pandas as pd

    rng = np.random.default_rng(5)
    n = 200
    x = rng.choice(np.array(["lo", "mid", "hi"], dtype=object), n)
    y = rng.choice(np.array([0.5, 1.5], dtype=np.float64), n)
    z = np.where((x == "hi") ^ (y > 1), "on", "off").astype(object)
    flip = rng.random(n) < 0.2
    z[flip] = np.where(z[flip] == "on", "off", "on")
    w = rng.choice(np.array([10.0, 20.0, 30.0]), n)
    df = pd.DataFrame({"X": x, "Y": y, "Z": z, "W": w})
    for c in df.columns:
        df.loc[rng.random(n) < 0.2, c] = np.nan
    return df


def case_b_c():
    df = frame_b()
    edges, nodes = [("X", "Z"), ("Y", "Z"), ("Z", "W")], ["X", "Y", "Z", "W"]
    # a state never seen in X and in W
    state_names = {"X": ["hi", "lo", "mid", "none"], "Y": [0.5, 1.5], "Z": ["off", "on"], "W": [10.0, 20.0, 30.0, 40.0]}
    b = {"frame": _frame(df), "edges": edges, "nodes": nodes, "state_names": state_names,
         "mle": _estimate(edges, nodes, df, "mle", state_names=state_names),
         "mle_collected": _estimate(edges, nodes, df, "mle"),
         "bdeu5": _estimate(edges, nodes, df, "bayes", state_names=state_names, prior_type="BDeu",
                            equivalent_sample_size=5)}
    rng = np.random.default_rng(6)
    shapes = {"X": (4, 1), "Y": (2, 1), "Z": (2, 8), "W": (4, 2)}
    arrays = {v: rng.integers(0, 5, size=s).astype(np.float64) + rng.choice([0.0, 0.25], size=s) for v, s in shapes.items()}
    c = {"k2": _estimate(edges, nodes, df, "bayes", state_names=state_names, prior_type="K2"),
         "dirichlet_scalar": _estimate(edges, nodes, df, "bayes", state_names=state_names, prior_type="dirichlet",
                                       pseudo_counts=3),
         "dirichlet_arrays": _estimate(edges, nodes, df, "bayes", state_names=state_names, prior_type="dirichlet",
                                       pseudo_counts=arrays),
         "bdeu_per_node": _estimate(edges, nodes, df, "bayes", state_names=state_names, prior_type="BDeu",
                                    equivalent_sample_size={"X": 1, "Y": 2.5, "Z": 10, "W": 4}),
         "pseudo_arrays": {v: a.tolist() for v, a in arrays.items()}}
    return b, c


def case_d():
    import pandas as pd

    rng = np.random.default_rng(8)
    n = 100
    a = rng.integers(0, 3, n)
    b = rng.integers(0, 2, n)
    c = (a + b + rng.integers(0, 2, n)) % 3
    df = pd.DataFrame({"A": a, "B": b, "C": c, "_weight": rng.random(n) * 4 + 0.25})
    edges, nodes = [("A", "C"), ("B", "C")], ["A", "B", "C"]
    return {"frame": _frame(df), "edges": edges, "nodes": nodes,
            "mle_weighted": _estimate(edges, nodes, df, "mle", weighted=True)}


def case_e():
    import pandas as pd
    from pgmpy.estimators import BayesianEstimator, MaximumLikelihoodEstimator

    from pgmpy_amd.utils import get_example_model
    from pgmpy_amd.utils.sampling import forward_sample_codes

    mine = get_example_model("alarm")
    codes, nodes = forward_sample_codes(mine, 1000, seed=11)
    ref = G._model("alarm")
    states = {v: list(ref.get_cpds(v).state_names[v]) for v in nodes}
    assert all([str(s) for s in states[v]] == [str(s) for s in mine.states[v]] for v in nodes)
    df = pd.DataFrame({v: np.asarray(states[v], dtype=object)[codes[i]] for i, v in enumerate(nodes)})
    out = {"codes": codes}
    for name, rows, cls, kw in (("mle", slice(None), MaximumLikelihoodEstimator, {}),
                                ("bdeu5", slice(None), BayesianEstimator, {"prior_type": "BDeu", "equivalent_sample_size": 5}),
                                ("mle_first", slice(0, 500), MaximumLikelihoodEstimator, {}),
                                ("mle_second", slice(500, 1000), MaximumLikelihoodEstimator, {})):
        from pgmpy.models import DiscreteBayesianNetwork

        m = DiscreteBayesianNetwork(ref.edges())
        m.add_nodes_from(ref.nodes())
        est = cls(m, df.iloc[rows].reset_index(drop=True), state_names=states)
        cpds = {c.variable: c for c in est.get_parameters(**kw)}
        vals, cnts = [], []
        for v in nodes:
            assert list(cpds[v].variables[1:]) == sorted(ref.get_parents(v))
            vals.append(np.asarray(cpds[v].get_values(), dtype=np.float64).ravel())
            cnts.append(np.asarray(est.state_counts(v), dtype=np.float64).ravel())
        out[f"{name}_values"] = np.concatenate(vals)
        out[f"{name}_counts"] = np.concatenate(cnts).astype(np.int64)
    path = os.path.join(HERE, "fit_alarm.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} B)")


def main():
    G._setup()
    b, c = case_b_c()
    G._dump("fit_cases.json", {"a": case_a(), "b": b, "c": c, "d": case_d()})
    case_e()


if __name__ == "__main__":
    main()
