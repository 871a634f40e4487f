#!/usr/bin/env python3
"""Generate tests/golden/dbn_viterbi.json by running the REFERENCE's VariableElimination.map_query on the networks of
tests/golden/dbn_cases.json ("doc" and "two_iface") unrolled to T = 3 as a DiscreteBayesianNetwork.

    PYTHONHASHSEED=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_viterbi.py

Recorded (inputs and results only), per network and evidence pattern of tests/viterbi_cases.golden_patterns:
  evidence         [[name, t], state] pairs;
  map              the reference's most probable assignment of every unobserved node, [[name, t], state] pairs;
  log_probability  log P(that assignment, the evidence), from the CPD tables in long double;
  gap              the relative distance of the second most probable completion (brute force).
"impossible" holds inputs only: a network with a deterministic X (zeros in its tables, recorded under "networks") and an
evidence pattern of probability 0 on it, for the tests of the impossible case (the reference has no rule for it).
The maker STOPS unless the reference's assignment is the brute-force argmax of the unrolled joint and the optimum is
separated from the second by more than 1e-6, so neither a fault of the reference nor a coin toss is ever pinned.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402

from tests import dbn_cases as C  # noqa: E402
from tests import viterbi_cases as V  # noqa: E402

SEPARATED, T = 1e-6, 3


def unrolled(spec, n_slices):
    """The reference's DiscreteBayesianNetwork of the first n_slices slices; node `{name}_{t}`."""
    from pgmpy.factors.discrete import TabularCPD
    from pgmpy.models import DiscreteBayesianNetwork

    names, card, n = spec["names"], spec["card"], len(spec["card"])

    def node(t, c):
        return f"{names[c % n]}_{t - 1 if (t and c < n) else t}"

    bn, cpds = DiscreteBayesianNetwork(), []
    for t in range(n_slices):
        for v, (cols, tab) in enumerate(spec["fam1"] if t else spec["fam0"]):
            var = [node(t, c) for c in cols]
            bn.add_node(var[0])
            cpds.append(TabularCPD(var[0], card[v], tab.reshape(card[v], -1), evidence=var[1:] or None,
                                   evidence_card=[card[c % n] for c in cols[1:]] or None))
    for cpd in cpds:
        bn.add_edges_from([(p, cpd.variable) for p in cpd.variables[1:]])
    bn.add_cpds(*cpds)
    bn.check_model()
    return bn


def main():
    make_golden._setup()
    from pgmpy.inference import VariableElimination

    golden = C.load_golden()
    out = {"T": T, "queries": []}
    for net in ("doc", "two_iface"):
        spec = C.golden_spec(golden, net)
        ve = VariableElimination(unrolled(spec, T + 1))
        for pat, ev in V.golden_patterns(spec).items():
            variables = [f"{name}_{t}" for t in range(T + 1) for name in spec["names"] if (name, t) not in ev]
            got = ve.map_query(variables=variables, evidence={f"{name}_{t}": s for (name, t), s in ev.items()},
                               show_progress=False)
            arr = C.evidence_array(spec, ev, T)
            want_path, want_l, gap = V.enumerate_map(spec, arr)
            ref = {(name, t): int(got[f"{name}_{t}"]) for t in range(T + 1) for name in spec["names"] if (name, t) not in ev}
            brute = {(spec["names"][v], t): int(want_path[t, v]) for t in range(T + 1) for v in range(len(spec["card"]))
                     if arr[t, v] == C.MISSING}
            if ref != brute:
                raise SystemExit(f"{net}/{pat}: the reference's map_query is not the brute-force argmax")
            if not gap > SEPARATED:
                raise SystemExit(f"{net}/{pat}: the optimum is separated by {gap:.3g} only")
            out["queries"].append({"network": net, "pattern": pat, "T": T,
                                   "evidence": [[list(k), int(s)] for k, s in ev.items()],
                                   "map": [[list(k), s] for k, s in ref.items()],
                                   "log_probability": float(V.path_logprob(spec, arr, want_path)), "gap": gap})
            assert abs(out["queries"][-1]["log_probability"] - float(want_l)) <= 1e-12
    # an evidence pattern of probability 0 under "doc" does not exist (no zeros in its tables): the impossible row of
    # the frame test contradicts itself through a recorded network with a deterministic X
    det = C.make_spec(seed=80, deterministic=("X",), **C.DOC)
    x_of_z = np.argmax(det["fam0"][0][1], axis=0)
    out["impossible"] = {"network": "deterministic", "T": 2, "evidence": [[["Z", 0], 0], [["X", 0], int(1 - x_of_z[0])], [["Y", 1], 1]]}
    out["networks"] = {"deterministic": {"names": det["names"], "card": det["card"], "intra": [list(e) for e in det["intra"]],
                                         "inter": [list(e) for e in det["inter"]],
                                         "fam0": [{"cols": list(map(int, c)), "table": t.tolist()} for c, t in det["fam0"]],
                                         "fam1": [{"cols": list(map(int, c)), "table": t.tolist()} for c, t in det["fam1"]]}}
    path = os.path.join(HERE, "dbn_viterbi.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"{len(out['queries'])} map queries agree with brute force; wrote {path} ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main()
