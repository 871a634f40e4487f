#!/usr/bin/env python3
"""Time MirrorDescentEstimator's one launch (csrc/pgmmd.hip k_md) beside the numpy restatement of tests/md_cases.py.

    python tools/md_bench.py [--card 8] [--iters 100] [--rows 1 256] [--reps 120] [--windows 5] [--warmup 3]
                             [--out profiles/md_bench.json]

The workload is the star ab - bc, bc - cd, bc - ce with every variable at `card` states, every clique a marginal,
n = 1000, `iters` iterations of the line search, for each batch size of `rows` (different target rows, the first
shared).  A window is a host clock around `reps` launches that ends in a device synchronise (about a second at the
defaults); `warmup` untimed launches first; the median, minimum and maximum over `windows`.  The restatement runs
the first row in float64 on the host (wall clock) and the device's mu of that row is compared with it.  A run that
finds no device fails.  Prints one JSON line; --out also writes it.
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

from tests import md_cases as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--card", type=int, default=8)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--reps", type=int, default=120)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native
    from pgmpy_amd import engine as E
    from pgmpy_amd.estimators._md import MdPlan

    assert torch.cuda.is_available(), "md_bench needs a HIP device"
    _native.lib()
    card, cliques, edges = [args.card] * 5, C.STAR[1], C.STAR[2]
    case = C.make(card, cliques, edges, cliques, seed=40, n=1000.0, rows=max(args.rows), iterations=args.iters)
    theta = E.to_device(np.concatenate([t.ravel() for t in case["theta"]])[None, :])
    plan = MdPlan(card, cliques, edges, cliques)
    t0 = time.perf_counter()
    ref = C.run(case)
    host_ms = (time.perf_counter() - t0) * 1e3
    out = {"workload": "star_mirror_descent", "card": args.card, "iters": args.iters, "n_cells": plan.n_cells,
           "n_sep": plan.n_sep, "n_y": plan.n_y, "tier": plan.tier, "lds_bytes": int(plan.info.lds_bytes),
           "phases": int(plan.info.n_phases), "reps": args.reps, "windows": args.windows, "warmup": args.warmup,
           "host_restatement_ms_per_instance": host_ms, "restatement_trials": [ref["trials"], ref["rejected"]], "batches": []}
    for B in args.rows:
        targets, totals = E.to_device(case["targets"][:B]), E.to_device(case["totals"][:B])
        run = lambda: plan.run(targets, totals, theta, "L2", args.iters, None)
        for _ in range(args.warmup):
            got = run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.windows):
            t0 = time.perf_counter()
            for _ in range(args.reps):
                got = run()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / args.reps)
        trials = got[3].cpu().numpy()
        # no assertion on the counts: near convergence a float64 restatement may take an Armijo branch the other way
        gap = float(np.abs(got[1][0].cpu().numpy() - ref["mu"]).max()) / 1000.0
        assert gap < 1e-9, gap
        med = float(np.median(ms))
        out["batches"].append({"rows": B, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "window_s": med * args.reps * 1e-3,
                               "trials_row0": [int(trials[0, 0]), int(trials[0, 1])], "trials_total": int(trials[:, 0].sum()),
                               "us_per_calibration_row0": 1e3 * med / (1 + int(trials[0, 0])),
                               "us_per_instance": 1e3 * med / B, "mu_gap_to_restatement_over_n": gap})
    out.update({"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "kind": "measured"})
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump([out], f)
            f.write("\n")


if __name__ == "__main__":
    main()
