#!/usr/bin/env python3
"""Generate the expectation-maximisation fixtures by running the REFERENCE ExpectationMaximization.

    PYTHONHASHSEED=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_em.py [--time]

Same set-up as make_golden_fit.py.  Writes recorded inputs and results only:

  em_cases.json   per case the network (observed nodes, latents, cardinalities, sorted parents), the nodes EM
                  re-estimates, the call's arguments, the stopping iteration n, and the reference's CPDs
                  (flat, [node, sorted parents]) after max_iter = 1, 3, 10 and at convergence; case (e): the
                  values of TabularCPD.get_random / get_uniform; case (f): the rows and latents the
                  constructor keeps
  em_cases.npz    the uint8 frames [n_observed, n_rows] (observed node i of the case is row i, the states are
                  0 .. card - 1), the initial CPD values and the pseudo-counts in the plan's flat layout

(a) A->H<-C, H->D<-C, H->E<-G with latents H:3 and G:2, 300 rows, explicit init_cpds;  (b) the same with
apply_smoothing=True, prior_type="BDeu";  (c) a hidden class Z:3 with four observed children, 500 rows,
init_cpds="uniform";  (d) case (a) with init_cpds="random", seed=7.

The stopping iteration n: the reference runs with max_iter = n - 2, n - 1 and n give the allclose quantity
max(|old - new| - 1e-5 |new|) of iterations n - 1 and n.  The generator stops with an error unless n < 100 and
that quantity is a factor of 2 away from atol at both (>= 2 atol at n - 1, <= atol / 2 at n), so that a rounding
difference cannot move n; the run with max_iter = 100 must return what max_iter = n returned.  EM on the network
of (a) converges linearly at a rate close to 1 (the quantity is still above 1e-3 after 100 iterations for every
data seed tried), so (a), (b) and (d) never stop: they record n = 100 = max_iter, and the same factor of 2 is
asked on the one side that exists (>= 2 atol at iteration 100).  The generator also prints d per case (the
largest difference between tests/em_cases.em_ref in plain fp64 and the reference), which goes into
tests/em_cases.GOLDEN_D.

--time: instead, the wall time of ONE reference iteration on the 1,000 alarm rows of fit_alarm.npz with the
two latents of tools/em_bench.py (the comparison row of DESIGN.md).
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import em_cases as C  # noqa: E402
import make_golden as G  # noqa: E402

EDGES_A = [("A", "H"), ("C", "H"), ("H", "D"), ("C", "D"), ("H", "E"), ("G", "E")]
CARD_A = {"A": 2, "C": 3, "D": 2, "E": 3, "H": 3, "G": 2}
EDGES_C = [("Z", f"X{i}") for i in range(4)]
CARD_C = {"Z": 3, "X0": 2, "X1": 3, "X2": 2, "X3": 4}
ITERS = (1, 3, 10)
MAX_ITER = 100  # get_parameters' default


def _network(edges, latents):
    nodes = []
    for u, v in edges:
        nodes += [x for x in (u, v) if x not in nodes]
    parents = {n: sorted(u for u, v in edges if v == n) for n in nodes}
    return nodes, parents, [n for n in nodes if n not in latents]


def _random_cpds(nodes, parents, card, rng, sharp):
    """Flat [node, sorted parents] values per node; `sharp` > 1 moves the columns away from uniform."""
    out = {}
    for n in nodes:
        v = rng.random((card[n], int(np.prod([card[p] for p in parents[n]], dtype=int)))) ** sharp + 0.02
        out[n] = v / v.sum(axis=0)
    return out


def _sample(nodes, parents, card, cpds, n_rows, rng):
    """Ancestral samples {node: int codes}; `nodes` is in a topological order of the edges used here."""
    order, done = [], set()
    while len(order) < len(nodes):
        for n in nodes:
            if n not in done and all(p in done for p in parents[n]):
                order.append(n), done.add(n)
    data = {}
    for n in order:
        col = np.zeros(n_rows, dtype=np.int64)
        for p in parents[n]:
            col = col * card[p] + data[p]
        cdf = np.cumsum(cpds[n], axis=0)
        u = rng.random(n_rows)
        data[n] = np.minimum((u[None, :] >= cdf[:, col]).sum(axis=0), card[n] - 1)
    return data


def _frame(data, observed):
    import pandas as pd

    return pd.DataFrame({v: data[v] for v in observed})


def _ref_cpd(variable, parents, card, flat):
    from pgmpy.factors.discrete import TabularCPD

    sn = {v: list(range(card[v])) for v in [variable] + parents}
    if not parents:
        return TabularCPD(variable, card[variable], flat.reshape(card[variable], 1), state_names=sn)
    return TabularCPD(variable, card[variable], flat.reshape(card[variable], -1), evidence=parents,
                      evidence_card=[card[p] for p in parents], state_names=sn)


def _run(edges, latents, card, df, max_iter, **kw):
    """The reference's CPDs after at most max_iter iterations: {node: flat [node, sorted parents]}."""
    from pgmpy.estimators import ExpectationMaximization
    from pgmpy.models import DiscreteBayesianNetwork

    m = DiscreteBayesianNetwork(edges, latents=set(latents))
    est = ExpectationMaximization(m, df)
    cpds = est.get_parameters(latent_card={v: card[v] for v in latents}, max_iter=max_iter, show_progress=False, **kw)
    out = {}
    for c in cpds:
        assert list(c.variables[1:]) == sorted(c.variables[1:]), c.variables
        assert [int(k) for k in c.cardinality] == [card[v] for v in c.variables]
        out[c.variable] = np.asarray(c.get_values(), dtype=np.float64).ravel()
    return out


def _em_case(name, edges, latents, card, frame, df, em_nodes, init, atol=1e-8, pseudo=None, bayes=False, **kw):
    nodes, parents, observed = _network(edges, latents)
    flat = lambda r: np.concatenate([r[v] for v in em_nodes])  # noqa: E731
    init_flat = np.concatenate([init[v].ravel() for v in em_nodes])
    col_of = {v: j for j, v in enumerate(observed + list(latents))}
    families = [([col_of[v] for v in [x] + parents[x]], [card[v] for v in [x] + parents[x]]) for x in em_nodes]
    codes = np.stack([df[v].to_numpy().astype(np.uint8) for v in observed])
    # where the restatement stops tells which reference runs are needed; the margin is the reference's own
    _, _, n = C.em_ref(families, [col_of[v] for v in latents], init_flat, codes, MAX_ITER, atol=atol, pseudo=pseudo,
                       bayes=bayes, dtype=np.float64)
    runs = {0: {v: init[v].ravel() for v in em_nodes}}
    for k in sorted(set(ITERS) | {max(n - 2, 1), max(n - 1, 1), n, MAX_ITER}):
        runs[k] = _run(edges, latents, card, df, k, atol=atol, **kw)
    excess = {k: C.allclose_excess(flat(runs[k - 1]), flat(runs[k])) for k in (n - 1, n) if k >= 1}
    if excess[n] > atol:  # max_iter reached: nothing stops the reference, and a rounding difference must not
        if n != MAX_ITER or excess[n] < 2 * atol:
            raise SystemExit(f"case {name}: excess {excess[n]:.3e} at iteration {n}: change the data")
    else:
        if n >= MAX_ITER:
            raise SystemExit(f"case {name}: converged only at iteration {n}: change the data")
        for k, e in excess.items():
            if not (e >= 2 * atol if k < n else e <= atol / 2):
                raise SystemExit(f"case {name}: excess {e:.3e} at iteration {k} is within a factor 2 of atol: change the data")
        assert all(np.array_equal(runs[MAX_ITER][v], runs[n][v]) for v in runs[n]), "the reference did not stop at n"
    results = {str(k): runs[k] for k in ITERS}
    results["converged"] = runs[MAX_ITER]
    # d: the restatement in plain fp64 against the reference
    d = 0.0
    for key, r in results.items():
        k = n if key == "converged" else min(int(key), n)
        mine, _, _ = C.em_ref(families, [col_of[v] for v in latents], init_flat, codes, k, pseudo=pseudo, bayes=bayes,
                              dtype=np.float64)
        d = max(d, float(np.max(np.abs(mine - flat(r)))))
        fixed = [v for v in r if v not in em_nodes]  # estimated once: the same in every run
        assert all(np.array_equal(r[v], runs[MAX_ITER][v]) for v in fixed)
    print(f"case {name}: n = {n}, excess = { {k: float(f'{e:.3e}') for k, e in excess.items()} }, d = {d:.3e}")
    meta = {"frame": frame, "edges": edges, "nodes": nodes, "observed": observed, "latents": list(latents),
            "cardinality": card, "parents": parents, "em_nodes": em_nodes, "atol": atol, "n_iter": n, "d": d,
            "kwargs": {k: v for k, v in kw.items() if k != "init_cpds" or isinstance(v, str)},
            "results": {key: {v: a.tolist() for v, a in r.items()} for key, r in results.items()}}
    return meta, init_flat


def cases_abd(meta, arrays):
    latents = ["H", "G"]
    nodes, parents, observed = _network(EDGES_A, latents)
    rng = np.random.default_rng(3)
    truth = _random_cpds(nodes, parents, CARD_A, rng, sharp=3.0)
    df = _frame(_sample(nodes, parents, CARD_A, truth, 300, rng), observed)
    arrays["abd_codes"] = np.stack([df[v].to_numpy().astype(np.uint8) for v in observed])
    em_nodes = [n for n in nodes if n in ("H", "G", "D", "E")]
    init = _random_cpds(nodes, parents, CARD_A, np.random.default_rng(4), sharp=1.0)
    init_cpds = {v: _ref_cpd(v, parents[v], CARD_A, init[v]) for v in em_nodes}
    meta["a"], arrays["a_init"] = _em_case("a", EDGES_A, latents, CARD_A, "abd", df, em_nodes, init, init_cpds=init_cpds)
    # (b): BDeu, equivalent_sample_size 5 (BayesianEstimator's default): 5 / bins per entry
    pseudo = np.concatenate([np.full(init[v].size, 5.0 / init[v].size) for v in em_nodes])
    meta["b"], arrays["b_init"] = _em_case("b", EDGES_A, latents, CARD_A, "abd", df, em_nodes, init, pseudo=pseudo, bayes=True,
                                           init_cpds=init_cpds, apply_smoothing=True, prior_type="BDeu")
    arrays["b_pseudo"] = pseudo
    # (d): every node starts from TabularCPD.get_random(seed=7), in the model's own parent order
    from pgmpy.factors.discrete import TabularCPD
    from pgmpy.models import DiscreteBayesianNetwork

    m = DiscreteBayesianNetwork(EDGES_A)
    rand = {}
    for v in nodes:
        ps = m.get_parents(v)
        c = TabularCPD.get_random(variable=v, evidence=ps, cardinality={x: CARD_A[x] for x in [v] + ps}, seed=7)
        vals = np.asarray(c.values, dtype=np.float64)
        rand[v] = np.ascontiguousarray(vals.transpose([0] + [1 + ps.index(p) for p in parents[v]])).reshape(CARD_A[v], -1)
    meta["d"], arrays["d_init"] = _em_case("d", EDGES_A, latents, CARD_A, "abd", df, nodes, rand, init_cpds="random", seed=7)


def case_c(meta, arrays):
    latents = ["Z"]
    nodes, parents, observed = _network(EDGES_C, latents)
    rng = np.random.default_rng(5)
    truth = _random_cpds(nodes, parents, CARD_C, rng, sharp=3.0)
    df = _frame(_sample(nodes, parents, CARD_C, truth, 500, rng), observed)
    arrays["c_codes"] = np.stack([df[v].to_numpy().astype(np.uint8) for v in observed])
    init = {v: np.full((CARD_C[v], int(np.prod([CARD_C[p] for p in parents[v]], dtype=int))), 1.0 / CARD_C[v]) for v in nodes}
    meta["c"], arrays["c_init"] = _em_case("c", EDGES_C, latents, CARD_C, "c", df, nodes, init, init_cpds="uniform")


def case_e(meta):
    from pgmpy.factors.discrete import TabularCPD

    out = []
    for seed in (0, 7):
        for evidence, card in ((None, {"A": 3}), (["B", "C"], {"A": 3, "B": 2, "C": 4})):
            for kind in ("random", "uniform"):
                fn = TabularCPD.get_random if kind == "random" else TabularCPD.get_uniform
                c = fn(variable="A", evidence=evidence, cardinality=card, seed=seed)
                out.append({"kind": kind, "seed": seed, "evidence": evidence, "cardinality": card,
                            "variables": list(c.variables), "values": np.asarray(c.get_values()).tolist()})
    c = TabularCPD.get_random(variable="A", evidence=["B"], seed=0)  # cardinality None: 2 each
    out.append({"kind": "random", "seed": 0, "evidence": ["B"], "cardinality": None, "variables": list(c.variables),
                "values": np.asarray(c.get_values()).tolist()})
    meta["e"] = out


def case_f(meta):
    import pandas as pd
    from pgmpy.estimators import ExpectationMaximization
    from pgmpy.models import DiscreteBayesianNetwork

    rng = np.random.default_rng(9)
    n = 40
    frame = {"A": rng.integers(0, 2, n).astype(float), "B": rng.integers(0, 3, n).astype(float),
             "C": rng.integers(0, 2, n).astype(float), "H": np.full(n, np.nan)}
    for col, row in (("A", 3), ("B", 17), ("C", 31)):
        frame[col][row] = np.nan
    df = pd.DataFrame(frame)
    edges = [("H", "A"), ("H", "B"), ("B", "C"), ("G", "C")]
    m = DiscreteBayesianNetwork(edges, latents={"G"})  # G is declared latent, H is not
    est = ExpectationMaximization(m, df)
    # The reference warns that it treats H as latent, but its `latents` property hands out a copy, so the update
    # is lost (and get_parameters then fails on H): "latents" is what it keeps, "all_nan" what it warned about.
    meta["f"] = {"frame": {c: [None if np.isnan(x) else x for x in df[c]] for c in df.columns}, "edges": edges,
                 "declared_latents": ["G"], "kept_rows": [int(i) for i in est.data.index],
                 "columns": list(est.data.columns), "latents": sorted(est.model.latents),
                 "all_nan": sorted(set(df.columns) - set(est.data.columns)),
                 "state_names": {v: [float(s) for s in est.state_names[v]] for v in est.data.columns}}


BENCH_LATENTS = {"VENTLUNG": 4, "CATECHOL": 2}  # tools/em_bench.py's


def time_reference():
    import pandas as pd
    from pgmpy.estimators import ExpectationMaximization
    from pgmpy.models import DiscreteBayesianNetwork

    ref = G._model("alarm")
    nodes = sorted(ref.nodes())
    codes = np.load(os.path.join(HERE, "fit_alarm.npz"))["codes"]
    states = {v: list(ref.get_cpds(v).state_names[v]) for v in nodes}
    df = pd.DataFrame({v: np.asarray(states[v], dtype=object)[codes[i]] for i, v in enumerate(nodes)
                       if v not in BENCH_LATENTS})
    m = DiscreteBayesianNetwork(ref.edges(), latents=set(BENCH_LATENTS))
    est = ExpectationMaximization(m, df)
    t0 = time.perf_counter()
    est.get_parameters(latent_card=dict(BENCH_LATENTS), max_iter=1, seed=0, show_progress=False)
    print(f"reference EM, alarm, latents {sorted(BENCH_LATENTS)}, {len(df)} rows, 1 iteration: "
          f"{time.perf_counter() - t0:.2f} s wall")


def main():
    G._setup()
    if "--time" in sys.argv:
        return time_reference()
    meta, arrays = {}, {}
    cases_abd(meta, arrays)
    case_c(meta, arrays)
    case_e(meta)
    case_f(meta)
    G._dump("em_cases.json", meta)
    path = os.path.join(HERE, "em_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main()
