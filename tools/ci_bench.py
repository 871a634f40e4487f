#!/usr/bin/env python3
"""Time the CI-test path and PC on alarm (37 nodes) over rows sampled on the device.

    python tools/ci_bench.py [--rows 1000000] [--steps 10] [--warmup 3] [--max-cond-vars 5] [--out FILE.json]

Per row count the uint8 codes are sampled into device memory (BayesianModelSampling.forward_sample_codes)
and stay there.  One `stable` PC run (chi_square, alpha 0.01) records the tests of every level; then, per
level and after a warm-up, separately,

  count    the pgm_fit_count launches over the level's tests, one per round of SCORE_BIN_BUDGET bins (HIP
           events around each call, which also reads its bad-code flag back)
  citest   the pgm_fit_citest launches over the same tables: the chunk launch, the packed launch and the
           finishing launch (HIP events); model bytes = 8 B per bin read

and the whole estimate (perf_counter around PC.estimate on the resident codes, device synchronised; the
second run is the warm one).  Prints one JSON line per row count; --out also writes them to a file.
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

from tools.fit_bench import HBM_PEAK_GBS, event_ms  # noqa: E402


class Recorder:
    """A tester that forwards to a CITester and keeps the triples of every batch."""

    def __init__(self, tester):
        self.tester, self.batches = tester, []

    def independent(self, triples, significance_level):
        self.batches.append([(X, Y, tuple(Z)) for X, Y, Z in triples])
        return self.tester.independent(triples, significance_level, 1.0)


def run(model, n, args):
    import pandas as pd
    import torch

    from pgmpy_amd.estimators import PC, CITester
    from pgmpy_amd.estimators import _rounds as R
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.estimators.PC import pc_skeleton
    from pgmpy_amd.inference.batch import download
    from pgmpy_amd.sampling import BayesianModelSampling

    d_codes, nodes = BayesianModelSampling(model).forward_sample_codes(n, seed=args.seed)
    states = model.states
    names = {v: list(states[v]) for v in nodes}
    codes = download(d_codes)
    frame = pd.DataFrame({v: pd.Categorical.from_codes(codes[i].astype(np.int8), categories=names[v])
                          for i, v in enumerate(nodes)})
    col_of = {v: j for j, v in enumerate(nodes)}
    tester = CITester.from_codes(d_codes, nodes, names)  # the resident codes: nothing is encoded or uploaded
    rec = Recorder(tester)
    skeleton, sepsets = pc_skeleton(nodes, rec, variant="stable", significance_level=0.01,
                                    max_cond_vars=args.max_cond_vars)
    levels = {}
    for batch in rec.batches:
        levels.setdefault(len(batch[0][2]), []).extend(batch)

    rows = []
    for size in sorted(levels):
        triples = levels[size]
        fams = [tester._family(X, [Y] + list(Z), col_of) for X, Y, Z in triples]
        sizes = [int(np.prod(c, dtype=object)) for _, c in fams]
        count_ms = ci_ms = 0.0
        bins = rounds = 0
        for idx in R.rounds(sizes, R.SCORE_BIN_BUDGET):
            plan = FitPlan([fams[i] for i in idx])
            tables = torch.zeros(plan.total_bins, dtype=torch.int64, device=d_codes.device)

            def count():
                tables.zero_()
                plan.count(d_codes, tables=tables)

            count_ms += event_ms(count, args.steps, args.warmup)[0]
            ci_ms += event_ms(lambda: plan.citest(tables, 1.0), args.steps, args.warmup)[0]
            bins += plan.total_bins
            rounds += 1
        rows.append({"cond_vars": size, "tests": len(triples), "rounds": rounds, "bins": bins,
                     "count_ms_median": count_ms, "citest_ms_median": ci_ms, "citest_model_bytes": 8 * bins,
                     "citest_model_GBs": 8 * bins / (ci_ms * 1e-3) / 1e9})

    est_s, edges = [], None
    for _ in range(2):  # the second run is the warm one
        est = PC(frame, state_names=names, tester=CITester.from_codes(d_codes, nodes, names))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pdag = est.estimate(variant="stable", ci_test="chi_square", significance_level=0.01,
                            max_cond_vars=args.max_cond_vars, show_progress=False)
        torch.cuda.synchronize()
        est_s.append(time.perf_counter() - t0)
        edges = len(pdag.directed_edges) + len(pdag.undirected_edges)
    return {"model": "alarm", "rows": n, "max_cond_vars": args.max_cond_vars, "levels": rows,
            "tests_total": int(sum(r["tests"] for r in rows)), "skeleton_edges": skeleton.number_of_edges(),
            "estimate_stable_chi_square_s": est_s, "estimate_edges": edges, "hbm_peak_GBs": HBM_PEAK_GBS,
            "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
            "date": time.strftime("%Y-%m-%d"), "kind": "measured"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-cond-vars", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native
    from pgmpy_amd.utils import get_example_model

    assert torch.cuda.is_available(), "ci_bench needs a HIP device"
    _native.lib()
    model = get_example_model("alarm")
    lines = []
    for n in args.rows:
        res = run(model, n, args)
        print(json.dumps(res), flush=True)
        lines.append(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f)


if __name__ == "__main__":
    main()
