#!/usr/bin/env python3
"""Generate tests/golden/dbn_cases.json + dbn_cases.npz by running the REFERENCE's DynamicBayesianNetwork and
DBNInference on the small networks of tests/dbn_cases.py.

    PYTHONHASHSEED=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dbn.py [--time]

Recorded (inputs and results only):
  networks   the CPD tables of "doc" (the docstring network Z -> X -> Y, Z_0 -> Z_1) and "two_iface"
             (Z_0 -> X_0, W_0 -> X_0, X_0 -> Y_0, Z_0 -> Z_1, W_0 -> W_1, Z_0 -> W_1, all binary);
  queries    per network and evidence pattern (none; on the non-interface node Y with gaps; on slice 0, interface
             nodes included) forward_inference and backward_inference of every node at t = 0 .. 3, and d, the
             deviation of the fp64 restatement from the long-double one on that sequence;
  interface_evidence   the two sequences on which the reference's backward pass is wrong (an interface node
             observed at t >= 1, an earlier slice queried): its value and the enumerated one;
  graph      graph-logic expectations: the edges after add_edge, interface nodes, get_constant_bn's edges, the CPDs
             initialize_initial_state adds, check_model's errors;
  fit        the reference's CPDs for a 4-node network on a 1,000 x 5 slice frame (dbn_cases.npz: the frame).
The maker STOPS unless the reference agrees with enumeration of the unrolled network to 1e-12 on every recorded
query, so a fault of the reference is never pinned; on the interface_evidence sequences it stops unless the
reference is MORE than 1e-2 away (that is what those two records are for).
--time also records the reference's wall time of one query on one sequence of the benchmark's HMM model at T = 20.
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402

from tests import dbn_cases as C  # noqa: E402

AGREE, WRONG = 1e-12, 1e-2
# (pattern, t) where the reference's BACKWARD pass is wrong on both networks although the evidence sits on slice 0
# alone: every interface node observed at slice 0 and slice 1 queried with no later evidence.  Its forward pass is
# right there and is recorded; the backward values go to "reference_faults" beside the enumerated ones, and the
# maker stops if the reference ever agrees there (the record would then be stale).
KNOWN_WRONG = {("slice0", 1)}


def ref_model(spec, only_needed=False):
    """The reference's model of a spec.  only_needed: slice-1 CPDs only where the node has a parent in the slice
    before (initialize_initial_state adds the others)."""
    from pgmpy.factors.discrete import TabularCPD
    from pgmpy.models import DynamicBayesianNetwork as DBN

    names, card, n = spec["names"], spec["card"], len(spec["card"])
    m = DBN()
    m.add_nodes_from(names)
    m.add_edges_from([((p, 0), (c, 0)) for p, c in spec["intra"]] + [((p, 0), (c, 1)) for p, c in spec["inter"]])
    for h, fams in enumerate((spec["fam0"], spec["fam1"])):
        for v, (cols, tab) in enumerate(fams):
            if h and only_needed and not any(c < n for c in cols[1:]):
                continue
            var = [(names[c % n], (c // n) if h else 0) for c in cols]
            m.add_cpds(TabularCPD(var[0], card[v], tab.reshape(card[v], -1), evidence=var[1:] or None,
                                  evidence_card=[card[c % n] for c in cols[1:]] or None))
    m.initialize_initial_state()
    return m


def spec_json(spec):
    return {"names": spec["names"], "card": spec["card"], "intra": [list(e) for e in spec["intra"]],
            "inter": [list(e) for e in spec["inter"]],
            "fam0": [{"cols": list(map(int, c)), "table": t.tolist()} for c, t in spec["fam0"]],
            "fam1": [{"cols": list(map(int, c)), "table": t.tolist()} for c, t in spec["fam1"]]}


def evidence_patterns(spec):
    iface = sorted({p for p, _ in spec["inter"]})
    return {
        "none": {},
        "leaf_gaps": {("Y", 0): 0, ("Y", 2): 1, ("Y", 3): 1},
        "leaf_all": {("Y", t): t % 2 for t in range(4)},
        "slice0": {**{(v, 0): 1 for v in iface}, ("Y", 0): 0},
        "slice0_and_leaf": {(iface[0], 0): 0, ("Y", 1): 1, ("Y", 3): 0},
    }


def gen_queries(out):
    from pgmpy.inference import DBNInference

    faults = out["reference_faults"] = []
    for net, spec in C.golden_networks().items():
        out["networks"][net] = spec_json(spec)
        m = ref_model(spec)
        off, _ = C.offsets(spec)
        for pat, ev in evidence_patterns(spec).items():
            for t in range(4):
                # the reference refuses a variable that is also evidence
                variables = [(name, t) for name in spec["names"] if (name, t) not in ev]
                inf = DBNInference(m)
                fwd = inf.forward_inference(variables, ev)
                bwd = DBNInference(m).backward_inference(variables, ev)
                T = max([t] + [s for _, s in ev])
                arr = C.evidence_array(spec, ev, T)
                ef, es, _ = C.enumerate_unrolled(spec, arr)
                rec = {"network": net, "pattern": pat, "evidence": [[list(k), int(s)] for k, s in ev.items()],
                       "variables": [list(v) for v in variables], "forward": [], "backward": []}
                for var in variables:
                    v = spec["names"].index(var[0])
                    sl = slice(off[v], off[v] + spec["card"][v])
                    for key, got, want in (("forward", fwd, ef), ("backward", bwd, es)):
                        val = np.asarray(got[var].values, dtype=np.float64)
                        err = float(np.abs(val - want[t, sl]).max())
                        if key == "backward" and (pat, t) in KNOWN_WRONG:
                            faults.append({"network": net, "pattern": pat, "variable": list(var), "reference": val.tolist(),
                                           "enumerated": want[t, sl].astype(np.float64).tolist(), "gap": err})
                            continue
                        if not err <= AGREE:
                            raise SystemExit(f"{net}/{pat}/{var}/{key}: the reference is {err:.3g} from enumeration")
                        rec[key].append(val.tolist())
                if (pat, t) in KNOWN_WRONG:
                    rec["backward"] = None
                    if not max(f["gap"] for f in faults if f["network"] == net and f["pattern"] == pat) > WRONG:
                        raise SystemExit(f"{net}/{pat}/t={t}: the reference's backward pass agrees with enumeration now")
                dm, dl = C.deviation(spec, [], arr)
                rec["d"] = [dm, dl]
                out["queries"].append(rec)
    print(f"{len(out['queries'])} queries agree with enumeration to {AGREE}")


def gen_interface_evidence(out):
    from pgmpy.inference import DBNInference

    for case in C.interface_evidence_cases():
        spec, var = case["spec"], case["query"]
        got = np.asarray(DBNInference(ref_model(spec)).query([var], case["evidence"])[var].values, dtype=np.float64)
        T = max(t for _, t in list(case["evidence"]) + [var])
        _, es, _ = C.enumerate_unrolled(spec, C.evidence_array(spec, case["evidence"], T), smooth_only=True)
        off, _ = C.offsets(spec)
        v = spec["names"].index(var[0])
        want = es[var[1], off[v]:off[v] + spec["card"][v]].astype(np.float64)
        gap = float(np.abs(got - want).max())
        if not gap > WRONG:
            raise SystemExit(f"interface evidence {case['name']}: the reference is only {gap:.3g} from enumeration")
        out["interface_evidence"][case["name"]] = {"reference": got.tolist(), "enumerated": want.tolist(), "gap": gap}
        print(f"interface evidence {case['name']}: the reference is {gap:.3g} from enumeration")


def gen_graph(out):
    from pgmpy.factors.discrete import TabularCPD
    from pgmpy.models import DynamicBayesianNetwork as DBN

    def nodes(xs):
        return sorted([list(x) for x in xs])

    def edges(es):
        return sorted([[list(u), list(v)] for u, v in es])

    g = {}
    m = DBN()
    m.add_edges_from([(("Z", 0), ("X", 0)), (("X", 0), ("Y", 0)), (("Z", 0), ("Z", 1))])
    g["edges"] = edges(m.edges())
    g["intra0"], g["intra3"], g["inter"] = edges(m.get_intra_edges()), edges(m.get_intra_edges(3)), edges(m.get_inter_edges())
    g["interface0"], g["interface1"] = nodes(m.get_interface_nodes(0)), nodes(m.get_interface_nodes(1))
    g["slice2"] = nodes(m.get_slice_nodes(2))
    g["constant_bn_edges"] = sorted([list(e) for e in m.get_constant_bn().edges()])
    g["moral_edges"] = sorted(sorted([list(u), list(v)]) for u, v in m.moralize().edges())
    g["markov_blanket_Z1"] = nodes(set(m.get_markov_blanket(("Z", 1))))
    errors = {}
    for name, bad in (("backward", lambda: m.add_edge(("X", 1), ("Z", 0))), ("far", lambda: m.add_edge(("X", 0), ("Z", 2))),
                      ("self", lambda: m.add_edge(("X", 0), ("X", 0))), ("loop", lambda: m.add_edge(("Y", 0), ("Z", 0))),
                      ("shape", lambda: m.add_edge("X", "Z"))):
        try:
            bad()
            raise SystemExit(f"the reference accepted the {name} edge")
        except (ValueError, NotImplementedError) as e:
            errors[name] = [type(e).__name__, str(e)]
    spec = C.doc_spec()
    cpds = [TabularCPD(("Z", 0), 2, [[0.5], [0.5]]),
            TabularCPD(("X", 0), 2, [[0.6, 0.9], [0.4, 0.1]], evidence=[("Z", 0)], evidence_card=[2]),
            TabularCPD(("Y", 0), 2, [[0.2, 0.3], [0.8, 0.7]], evidence=[("X", 0)], evidence_card=[2]),
            TabularCPD(("Z", 1), 2, [[0.4, 0.7], [0.6, 0.3]], evidence=[("Z", 0)], evidence_card=[2])]
    m.add_cpds(*cpds)
    m.initialize_initial_state()
    g["initialized"] = sorted(([list(v) for v in c.variables], np.asarray(c.get_values()).tolist()) for c in m.get_cpds())
    del spec
    for name, cpd in (("parents", TabularCPD(("X", 0), 2, [[0.5], [0.5]])),
                      ("sum", TabularCPD(("X", 0), 2, [[0.6, 0.9], [0.3, 0.1]], evidence=[("Z", 0)], evidence_card=[2]))):
        m2 = DBN([(("Z", 0), ("X", 0)), (("Z", 0), ("Z", 1))])
        m2.add_cpds(cpd)
        try:
            m2.check_model()
            raise SystemExit(f"the reference's check_model accepted the {name} CPD")
        except ValueError as e:
            errors["check_" + name] = [type(e).__name__, str(e)]
    g["errors"] = errors
    out["graph"] = g


FIT_EDGES = [(("A", 0), ("B", 0)), (("A", 0), ("C", 0)), (("B", 0), ("D", 0)), (("C", 0), ("D", 0)),
             (("A", 0), ("A", 1)), (("B", 0), ("B", 1)), (("C", 0), ("C", 1)), (("D", 0), ("D", 1))]


def gen_fit(out, arrays):
    import pandas as pd
    from pgmpy.models import DynamicBayesianNetwork as DBN

    rng = np.random.default_rng(7)
    # not uniform noise: A persists, B and C follow A, D follows B xor C, each with a flip probability
    cols, data = [], {}
    for t in range(5):
        a = data[("A", t - 1)] ^ (rng.random(1000) < 0.2) if t else rng.random(1000) < 0.4
        b = a ^ (rng.random(1000) < 0.3)
        c = a ^ (rng.random(1000) < 0.25)
        d = (b ^ c) ^ (rng.random(1000) < 0.1)
        for name, x in zip("ABCD", (a, b, c, d)):
            data[(name, t)] = x.astype(bool)
            cols.append((name, t))
    frame = np.stack([data[c] for c in cols], axis=1).astype(np.uint8)
    m = DBN(FIT_EDGES)
    m.fit(pd.DataFrame(frame, columns=cols))
    arrays["fit_data"] = frame
    out["fit"] = {"columns": [list(c) for c in cols], "edges": [[list(u), list(v)] for u, v in FIT_EDGES],
                  "cpds": [{"variables": [list(v) for v in c.variables], "values": np.asarray(c.get_values()).tolist()}
                           for c in m.cpds]}


def gen_time(out):
    from pgmpy.inference import DBNInference

    spec = C.hmm_spec()
    m = ref_model(spec)
    ev = {(name, t): int(C.sample(spec, 20, 1, 3)[0, t, v]) for t in range(21)
          for v, name in enumerate(spec["names"]) if name != "H"}
    t0 = time.perf_counter()
    DBNInference(m).query([("H", t) for t in range(21)], ev)
    out["timing"] = {"model": "hmm: 1 hidden node of 8 states, 8 observed children", "T": 20, "queries": 1,
                     "reference_seconds": time.perf_counter() - t0}
    print("reference query, one sequence, T = 20:", out["timing"]["reference_seconds"], "s")


def main():
    make_golden._setup()
    out = {"networks": {}, "queries": [], "interface_evidence": {}}
    arrays = {}
    gen_queries(out)
    gen_interface_evidence(out)
    gen_graph(out)
    gen_fit(out, arrays)
    if "--time" in sys.argv:
        gen_time(out)
    path = os.path.join(HERE, "dbn_cases.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    np.savez_compressed(os.path.join(HERE, "dbn_cases.npz"), **arrays)
    print("wrote", path, os.path.getsize(path), "B;", os.path.getsize(os.path.join(HERE, "dbn_cases.npz")), "B")


if __name__ == "__main__":
    main()
