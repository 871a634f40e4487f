#!/usr/bin/env python3
"""Time the exact structure search (csrc/pgmxs.hip: the subset-lattice dynamic programme behind ExhaustiveSearch).

    python tools/xs_bench.py [--sizes 16 20 24] [--max-indegree 3] [--rows 10000] [--steps 5] [--warmup 2]
                             [--out profiles/xs_bench.json]

Synthetic: every family of at most `max_indegree` parents over n nodes with N(0, 1) scores, one pgm_xs_run per step:
the host checks, the staging of the families, the fill, scatter, zeta, sink and read-back launches and the download
of the record, on a host clock around the call (it ends in a stream synchronise).  The tables are allocated by the
first, untimed run.  Beside it the device time of each phase of the same runs (pgm_xs_phase_ms: HIP events around the
fill and scatter, the zeta launches, the sink launches; the rest of a run is host work).  At the first size the numpy restatement of the recurrence (tests/xs_cases.py recurrence) runs on
the same families in the same process, and the device result must equal it.  Then the edge posteriors of the same
families on the same handle (pgm_xs_posterior), on the same clocks: the whole call, and its four phases (fill and
scatter; the alpha passes; F and B; gamma, its superset sums and the edge sums); every mass must be 1 and F[V] = B[V]
to 1e-9, and at the first size the matrix must agree with tests/xsp_cases.py recurrence in float64.  Real: BIC on the first 16 columns of rows
forward-sampled from alarm, ExhaustiveSearch.estimate(max_indegree) split into family scoring (local_scores) and the
programme; HillClimbSearch's score on the same data beside it.  `warmup` untimed runs, the median and minimum of `steps`.
Not measured: single launches within a phase (a kernel trace would give them), hardware counters, the tilings other
than the default.  A run that finds no device fails.  Prints one JSON line; --out also writes it.
"""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def clock_ms(fn, steps, warmup):
    """(median, min) ms of fn(), which synchronises, on the host clock."""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--max-indegree", type=int, default=3)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pandas as pd
    import torch

    from pgmpy_amd import _native
    from pgmpy_amd.estimators import BIC, ExhaustiveSearch, HillClimbSearch
    from pgmpy_amd.estimators._xs import XsPlan
    from pgmpy_amd.estimators.ExhaustiveSearch import enumerate_families
    from pgmpy_amd.utils import get_example_model
    from pgmpy_amd.utils.sampling import forward_sample_codes
    from tests.xs_cases import recurrence
    from tests.xsp_cases import recurrence as posterior_recurrence

    assert torch.cuda.is_available(), "xs_bench needs a HIP device"
    _native.lib()
    synthetic = []
    for k, n in enumerate(args.sizes):
        fams = enumerate_families(n, args.max_indegree)
        nodes = np.array([v for v, _ in fams], dtype=np.int32)
        masks = np.array([m for _, m in fams], dtype=np.uint32)
        scores = np.random.default_rng(n).standard_normal(len(fams))
        plan = XsPlan(n)
        info = plan.info()
        phases = []

        def step():
            plan.run(nodes, masks, scores)
            phases.append(plan.phase_ms())

        med, lo = clock_ms(step, args.steps, args.warmup)
        phase = {f"{k}_ms_median": float(np.median([p[k] for p in phases[args.warmup:]])) for k in phases[0]}
        # at every size: the parents are given families, every parent stands after its child in the sink order, and
        # the families' scores sum to R[V] within the rounding of n adds
        got, given, later = plan.run(nodes, masks, scores), dict(zip(zip(nodes.tolist(), masks.tolist()), scores)), 0
        for v in reversed(got["order"]):
            assert got["parents"][v] & ~later == 0, "the sink order does not fit the parents"
            later |= 1 << v
        terms = [given[(v, got["parents"][v])] for v in range(n)]
        assert abs(sum(terms) - got["score"]) <= n * 2.0 ** -52 * sum(abs(t) for t in terms), "R[V] is not the families' sum"
        cells = n << (n - 1)
        row = {"n": n, "families": len(fams), "table_cells": cells, "table_bytes": 12 * cells + 12 * (1 << n),
               "zeta_launches": int(info.zeta_launches), "sink_launches": int(info.sink_launches),
               "run_ms_median": med, "run_ms_min": lo, "cells_per_s": cells / (med * 1e-3), **phase}
        if k == 0:
            t0 = time.perf_counter()
            want = recurrence(n, nodes, masks, scores)
            row["numpy_restatement_ms"] = (time.perf_counter() - t0) * 1e3
            assert got["score"] == want["score"] and got["parents"] == want["parents"], "device and restatement differ"
        # the edge posteriors of the same families on the same handle (pgm_xs_posterior), timed the same way
        phases = []

        def post_step():
            plan.posterior(nodes, masks, scores)
            phases.append(plan.phase_ms())

        med, lo = clock_ms(post_step, args.steps, args.warmup)
        post = plan.posterior(nodes, masks, scores)
        z = abs(post["log_z"][0])
        assert not post["infeasible"] and np.abs(post["mass"] - 1).max() < 1e-9 and abs(post["log_z"][0] - post["log_z"][1]) < 1e-9 * z
        row["posterior"] = {"run_ms_median": med, "run_ms_min": lo, "log_z": float(post["log_z"][0]),
                            "lse2_evaluations": (n - 1) * cells + n * (1 << n),
                            **{f"{k}_ms_median": float(np.median([p[k] for p in phases[args.warmup:]])) for k in phases[0]}}
        if k == 0:
            t0 = time.perf_counter()
            want = posterior_recurrence(n, (nodes, masks, scores))
            row["posterior"]["numpy_restatement_ms"] = (time.perf_counter() - t0) * 1e3
            assert np.abs(post["edge_post"] - want["edge_post"]).max() < 1e-9, "device and restatement differ"
        synthetic.append(row)
        del plan

    codes, names = forward_sample_codes(get_example_model("alarm"), args.rows, seed=1)
    data = pd.DataFrame({v: np.asarray(codes[i]) for i, v in enumerate(names[:16])})
    scorer = BIC(data)
    search = ExhaustiveSearch(data, scoring_method=scorer, use_cache=False)
    search.estimate(max_indegree=args.max_indegree)  # warm
    nodes16 = search._nodes()
    fams = enumerate_families(16, args.max_indegree)
    score_ms = clock_ms(lambda: search._scores(nodes16, fams), args.steps, 0)
    total_ms = clock_ms(lambda: search.estimate(max_indegree=args.max_indegree), args.steps, 0)
    hill = HillClimbSearch(data).estimate(scoring_method=scorer, max_indegree=args.max_indegree, show_progress=False)
    real = {"model": "alarm", "columns": 16, "rows": args.rows, "score": "BIC", "max_indegree": args.max_indegree,
            "families": search.n_families, "family_scoring_ms_median": score_ms[0], "family_scoring_ms_min": score_ms[1],
            "estimate_ms_median": total_ms[0], "estimate_ms_min": total_ms[1],
            "programme_and_host_ms_median": total_ms[0] - score_ms[0], "best_score": search.best_score,
            "hill_climb_score": float(scorer.score(hill))}
    out = {"workload": "exact_structure_search", "synthetic": synthetic, "real": real, "steps": args.steps,
           "warmup": args.warmup,
           "not_measured": ["single launches within a phase", "hardware counters", "tilings other than the default"],
           "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "tool": "tools/xs_bench.py",
           "kind": "measured"}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump([out], f)
            f.write("\n")


if __name__ == "__main__":
    main()
