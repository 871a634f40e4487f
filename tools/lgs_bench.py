#!/usr/bin/env python3
"""Time Gaussian structure learning on a resident value matrix: the Gram, the batched partial correlations and
family scores on it, PC and a BICGauss hill climb, each batch next to the only alternative the parent of this
change had: download the Gram matrix and solve every job on the host with numpy / models._lg.ols.

    python tools/lgs_bench.py [--rows 1000000] [--d 37 128] [--steps 10] [--warmup 3] [--host-jobs 20000]
                              [--out profiles/lgs_bench.json]

Per d a random linear-Gaussian DAG (at most three parents per node, zero intercepts, unit noise) is sampled into
device memory (LinearGaussianBayesianNetwork.simulate_values) and stays there.  Recorded:

  gram_ms          pgm_lg_colsum + pgm_lg_gram over all the rows (HIP events)
  level1           every test X _|_ Y | {Z} (d (d - 1) / 2 pairs x d - 2 columns; 23,310 at d = 37):
                     kernel_ms   the pgm_lgs_pcorr launch on a handle made before (HIP events)
                     batch_s     the batch end to end: the handle from host job lists, the launch, the download
                                 (wall clock, three runs); handle_s is its share spent making the handle
                     host_s      the host loop over the first --host-jobs jobs from the downloaded matrix, and
                                 host_s_per_job; host_full_s_estimate = per job x all jobs (an estimate, marked so)
  families1        the d (d - 1) single-parent families of a first hill-climb step, the same four figures
                   (pgm_lgs_score, kind bic; the host side is models._lg.ols per family)
  pc_stable_s      at d = 37: PC(tester=GaussCITester.from_values(...)).estimate("stable"), two runs (the second warm)
  hill_climb_s     at d = 37: hill_climb(variables, BICGauss.from_values(...)), two runs
A path that finds no device fails.  Prints one JSON line per d; --out also writes them to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.fit_bench import event_ms  # noqa: E402


def random_model(d, seed):
    from pgmpy_amd.factors.continuous import LinearGaussianCPD
    from pgmpy_amd.models import LinearGaussianBayesianNetwork

    rng = np.random.default_rng(seed)
    names = [f"x{i}" for i in range(d)]
    m = LinearGaussianBayesianNetwork()
    m.add_nodes_from(names)
    for i, v in enumerate(names):
        parents = sorted(rng.choice(i, size=min(i, int(rng.integers(0, 4))), replace=False).tolist()) if i else []
        m.add_edges_from([(names[p], v) for p in parents])
        beta = [0.0] + [float(rng.choice([-1.0, -0.75, 0.75, 1.0])) for _ in parents]
        m.add_cpds(LinearGaussianCPD(v, beta, 1.0, [names[p] for p in parents]))
    return m, names


def host_pcorr(G, shift, jobs):
    """The parent's only route: every job solved with numpy from the downloaded matrix (no intercept, raw moments)."""
    from scipy.special import betainc

    d = G.shape[0] - 1
    n = G[d, d]
    c = np.append(shift, 0.0)
    M = G + np.outer(c, G[:, d]) + np.outer(G[:, d], c) + n * np.outer(c, c)
    coef = np.empty(len(jobs))
    for i, (K, T) in enumerate(jobs):
        Mkk, Mkt, Mtt = M[np.ix_(K, K)], M[np.ix_(K, T)], M[np.ix_(T, T)]
        R = Mtt - Mkt.T @ np.linalg.solve(Mkk, Mkt) if len(K) else Mtt
        cxx, cyy, cxy = R[0, 0] - R[0, 2] ** 2 / n, R[1, 1] - R[1, 2] ** 2 / n, R[0, 1] - R[0, 2] * R[1, 2] / n
        coef[i] = cxy / np.sqrt(cxx * cyy)
    coef = np.clip(coef, -1, 1)
    return coef, betainc((n - 2) / 2, 0.5, 1 - coef ** 2)


def host_scores(G, shift, fams):
    from pgmpy_amd.models import _lg

    n, mean, S = _lg.moments(G, shift)
    out = np.empty(len(fams))
    nn = float(n)
    for i, (v, parents) in enumerate(fams):
        _, std = _lg.ols(n, mean, S, v, parents, "mle")
        out[i] = -0.5 * nn * (np.log(2 * np.pi * std * std) + 1) - 0.5 * (len(parents) + 2) * np.log(nn)
    return out


def batch_figures(data, jobs, call, host, host_jobs, args):
    import torch

    from pgmpy_amd.models import _lg

    G, shift = data.gram()
    handle = _lg.SchurJobs(data.d, jobs)
    kernel_ms = event_ms(lambda: call(handle, G, shift), args.steps, args.warmup)
    walls, pys = [], []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = _lg.SchurJobs(data.d, jobs)
        t1 = time.perf_counter()
        a, b, _ = call(h, G, shift)
        torch.stack([a, b]).cpu()
        walls.append(time.perf_counter() - t0)
        pys.append(t1 - t0)
    t0 = time.perf_counter()
    Gh, sh = G.cpu().numpy(), shift.cpu().numpy()
    host(Gh, sh, host_jobs)
    host_s = time.perf_counter() - t0
    return {"jobs": len(jobs), "launches": int(handle.info.n_buckets), "kernel_ms_median": kernel_ms[0], "kernel_ms_min": kernel_ms[1],
            "batch_s": walls, "handle_s": pys, "host_jobs_timed": len(host_jobs), "host_s": host_s,
            "host_s_per_job": host_s / max(len(host_jobs), 1),
            "host_full_s_estimate": host_s / max(len(host_jobs), 1) * len(jobs)}


def run(d, args):
    import torch

    from pgmpy_amd.estimators import PC, BICGauss, GaussCITester
    from pgmpy_amd.estimators.HillClimbSearch import hill_climb

    model, names = random_model(d, args.seed)
    X = model.simulate_values(args.rows, seed=args.seed)
    tester = GaussCITester.from_values(X, names)
    tester.gram()
    gram_ms = event_ms(lambda: tester._plan.moments_device(X, args.rows, 0), args.steps, args.warmup)
    tests = [([z], [x, y, d]) for x in range(d) for y in range(x + 1, d) for z in range(d) if z not in (x, y)]
    fams = [([d, u], [v]) for v in range(d) for u in range(d) if u != v]
    res = {"d": d, "rows": args.rows, "edges": model.number_of_edges(), "gram_ms_median": gram_ms[0], "gram_ms_min": gram_ms[1],
           "level1": batch_figures(tester, tests, lambda h, G, s: h.pcorr(G, s), host_pcorr, tests[:args.host_jobs], args),
           "families1": batch_figures(tester, fams, lambda h, G, s: h.score(G, s, "bic"),
                                      lambda G, s, jobs: host_scores(G, s, [(T[0], K[1:]) for K, T in jobs]),
                                      fams[:args.host_jobs], args)}
    if d <= args.search_max_d:
        pc_s, hc_s = [], []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pdag = PC(None, tester=GaussCITester.from_values(X, names)).estimate(variant="stable", significance_level=0.01)
            torch.cuda.synchronize()
            pc_s.append(time.perf_counter() - t0)
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dag, steps, _ = hill_climb(names, BICGauss.from_values(X, names))
            torch.cuda.synchronize()
            hc_s.append(time.perf_counter() - t0)
        res.update({"pc_stable_s": pc_s, "pc_edges": len(pdag.directed_edges) + len(pdag.undirected_edges),
                    "hill_climb_s": hc_s, "hill_climb_steps": steps, "hill_climb_edges": dag.number_of_edges()})
    res.update({"steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
                "date": time.strftime("%Y-%m-%d"), "kind": "measured"})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, nargs="+", default=[37, 128])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-jobs", type=int, default=20000)
    ap.add_argument("--search-max-d", type=int, default=37)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native

    assert torch.cuda.is_available(), "lgs_bench needs a HIP device"
    _native.lib()
    lines = []
    for d in args.d:
        res = run(d, args)
        print(json.dumps(res), flush=True)
        lines.append(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f)


if __name__ == "__main__":
    main()
