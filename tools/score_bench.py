#!/usr/bin/env python3
"""Time the structure-score path on alarm (37 nodes) over rows sampled on the device.

    python tools/score_bench.py [--rows 100000 1000000] [--steps 20] [--warmup 3] [--out FILE.json]

Per row count the uint8 codes are sampled into device memory (BayesianModelSampling.forward_sample_codes)
and stay there.  The plan holds the 1,369 families of a hill climb's first step on alarm: 37 without
parents and 37 * 36 with one.  After a warm-up, separately,

  plan     FitPlan(families): host validation and layout (perf_counter; no device work)
  count    one pgm_fit_count launch over the 1,369 families (HIP events around the call, which also reads
           its bad-code flag back)
  score    pgm_fit_score in LL mode (BIC / AIC / LL) and in BD mode (BDeu): the chunk launch and the
           per-family sum launch (HIP events); model bytes = 8 B per bin read
  estimate one full HillClimbSearch.estimate("bic-d", max_indegree=4) on the resident codes, with the
           number of operations it applied and of local_scores batches it asked for (perf_counter
           around the call, device synchronised)

and, for comparison on the same host, the same 1,369 BIC scores from np.bincount tables in fp64 numpy on
one core.  Prints one JSON line per row count; --out also writes them to a file.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.fit_bench import HBM_PEAK_GBS, event_ms  # noqa: E402


def first_step_families(cards):
    n = len(cards)
    fams = [([v], [cards[v]]) for v in range(n)]
    fams += [([v, p], [cards[v], cards[p]]) for v in range(n) for p in range(n) if p != v]
    return fams


def numpy_bic(codes, fams, n_rows):
    """The 1,369 BIC scores on the host: np.bincount tables, fp64 numpy logs."""
    out = []
    for cols, cards in fams:
        idx = np.zeros(codes.shape[1], dtype=np.int64)
        for c, k in zip(cols, cards):
            idx *= k
            idx += codes[c]
        t = np.bincount(idx, minlength=int(np.prod(cards))).reshape(cards[0], -1).astype(np.float64)
        nj = t.sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ll = np.where(t > 0, t * (np.log(t) - np.log(nj)[None, :]), 0.0).sum()
        out.append(ll - 0.5 * math.log(n_rows) * t.shape[1] * (cards[0] - 1))
    return np.array(out)


def run(model, n, args):
    import pandas as pd
    import torch

    from pgmpy_amd import _native as N
    from pgmpy_amd import engine as E
    from pgmpy_amd.estimators import BIC, HillClimbSearch
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.inference.batch import download
    from pgmpy_amd.sampling import BayesianModelSampling

    d_codes, nodes = BayesianModelSampling(model).forward_sample_codes(n, seed=args.seed)
    states = model.states
    cards = [len(states[v]) for v in nodes]
    fams = first_step_families(cards)

    plan_s = []
    for _ in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        plan = FitPlan(fams)
        plan_s.append(time.perf_counter() - t0)
    plan_ms = float(np.median(plan_s[args.warmup:])) * 1e3

    tables = torch.zeros(plan.total_bins, dtype=torch.int64, device=d_codes.device)

    def count():
        tables.zero_()
        plan.count(d_codes, tables=tables)

    count_ms, count_min = event_ms(count, args.steps, args.warmup)
    q = np.array([plan.sizes[f] // c[1][0] for f, c in enumerate(fams)], dtype=np.float64)
    r = np.array([c[1][0] for c in fams], dtype=np.float64)
    alpha, beta = E.to_device(10.0 / q), E.to_device(10.0 / (q * r))
    ll_ms, ll_min = event_ms(lambda: plan.score(tables, N.SCORE_LL), args.steps, args.warmup)
    bd_ms, bd_min = event_ms(lambda: plan.score(tables, N.SCORE_BD, alpha, beta), args.steps, args.warmup)
    ll = download(plan.score(tables, N.SCORE_LL))
    model_bytes = 8 * plan.total_bins

    codes = download(d_codes)
    t0 = time.perf_counter()
    want = numpy_bic(codes, fams, n)
    cpu_s = time.perf_counter() - t0
    got = ll - 0.5 * math.log(n) * q * (r - 1)
    assert np.allclose(got, want, rtol=1e-10, atol=0), "device scores differ from the numpy restatement"

    # one full search on the resident codes: the score object is handed its encoded columns
    frame = pd.DataFrame({v: pd.Categorical.from_codes(codes[i].astype(np.int8), categories=list(states[v]))
                          for i, v in enumerate(nodes)})
    names = {v: list(states[v]) for v in nodes}
    est_s, steps, batches = [], None, None
    for _ in range(2):  # the second run is the warm one
        score = BIC(frame, state_names=names)
        score._encoded = (d_codes, {v: j for j, v in enumerate(nodes)})
        calls = []
        inner = score.local_scores
        score.local_scores = lambda families, _inner=inner, _calls=calls: (_calls.append(len(families)), _inner(families))[1]
        est = HillClimbSearch(frame, state_names=names)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dag = est.estimate(scoring_method=score, max_indegree=4, show_progress=False)
        torch.cuda.synchronize()
        est_s.append(time.perf_counter() - t0)
        steps, batches = est.n_iterations, list(calls)
    return {
        "model": "alarm", "rows": n, "families": len(fams), "groups": int(plan.info.n_groups),
        "total_bins": plan.total_bins, "score_chunks": int(sum(-(-int(x) // N.SCORE_CHUNK) for x in q)),
        "plan_build_ms_median": plan_ms, "count_ms_median": count_ms, "count_ms_min": count_min,
        "score_ll_ms_median": ll_ms, "score_ll_ms_min": ll_min, "score_bd_ms_median": bd_ms, "score_bd_ms_min": bd_min,
        "score_model_bytes": model_bytes, "score_ll_model_GBs": model_bytes / (ll_ms * 1e-3) / 1e9,
        "score_bd_model_GBs": model_bytes / (bd_ms * 1e-3) / 1e9, "hbm_peak_GBs": HBM_PEAK_GBS,
        "step_ms_plan_count_score_ll": plan_ms + count_ms + ll_ms,
        "estimate_bic_s": est_s, "estimate_operations": steps, "estimate_batches": len(batches),
        "estimate_families_scored": int(sum(batches)), "estimate_edges": dag.number_of_edges(),
        "cpu_numpy_bic_s_one_core": cpu_s, "steps": args.steps, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "kind": "measured",
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native
    from pgmpy_amd.utils import get_example_model

    assert torch.cuda.is_available(), "score_bench needs a HIP device"
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
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
