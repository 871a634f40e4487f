#!/usr/bin/env python3
"""Generate the ApproxInference fixtures by running the REFERENCE (pgmpy/inference/ApproxInference.py).

    PYTHONHASHSEED=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_approx.py

Same set-up as make_golden_metrics.py (make_golden._setup(): the reference and the offline shims on
sys.path).  The network is the 5-node "net5" of metrics_cases.json and the frame its first 500 recorded
rows (metrics_cases.npz net5_codes1000), so nothing is sampled here.  Writes data only:

  approx_cases.json  n_rows; for the reference's get_distribution on that frame with the model's state
                     names: the joint over JOINT (variables, cardinalities, values in C order) and the
                     per-variable distributions of every node; map_query(samples=frame) over JOINT and
                     over MAP2; and the joint over SUBSET_VARS with the state names SUBSET (a state left
                     out, the others reordered)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as G  # noqa: E402

N_ROWS = 500
JOINT = ["C", "A", "E"]
MAP2 = ["D", "B"]
SUBSET_VARS = ["D", "A"]
SUBSET = {"D": ["d2", "d0"], "A": ["a1", "a0"]}


def main():
    G._setup()
    import pandas as pd
    from pgmpy.factors.discrete import TabularCPD
    from pgmpy.inference import ApproxInference
    from pgmpy.models import DiscreteBayesianNetwork

    with open(os.path.join(HERE, "metrics_cases.json")) as f:
        meta = json.load(f)
    states = meta["states"]
    m = DiscreteBayesianNetwork([tuple(e) for e in meta["edges"]])
    for v in meta["nodes"]:
        variables = meta["cpds"][v]["variables"]
        m.add_cpds(TabularCPD(v, len(states[v]), meta["cpds"][v]["values"], evidence=variables[1:] or None,
                              evidence_card=[len(states[u]) for u in variables[1:]] or None,
                              state_names={u: states[u] for u in variables}))
    m.check_model()
    codes = np.load(os.path.join(HERE, "metrics_cases.npz"))["net5_codes1000"][:, :N_ROWS]
    nodes = sorted(states)
    frame = pd.DataFrame({v: [states[v][k] for k in codes[i]] for i, v in enumerate(nodes)})
    infer = ApproxInference(m)

    def dump(f):
        return {"variables": list(f.variables), "cardinality": [int(k) for k in f.cardinality],
                "values": np.asarray(f.values, dtype=np.float64).ravel().tolist(),
                "state_names": {v: list(f.state_names[v]) for v in f.variables}}

    out = {
        "n_rows": N_ROWS,
        "joint": dump(infer.get_distribution(frame, JOINT, state_names=states, joint=True)),
        "marginals": {v: dump(f) for v, f in infer.get_distribution(frame, nodes, state_names=states, joint=False).items()},
        "map_joint": infer.map_query(JOINT, samples=frame, state_names=states),
        "map2_variables": MAP2,
        "map2": infer.map_query(MAP2, samples=frame, state_names=states),
        "subset": dump(infer.get_distribution(frame, SUBSET_VARS, state_names=SUBSET, joint=True)),
    }
    G._dump("approx_cases.json", out)


if __name__ == "__main__":
    main()
