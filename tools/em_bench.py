#!/usr/bin/env python3
"""Time the E-step of ExpectationMaximization on alarm with two interior nodes declared latent.

    python tools/em_bench.py [--rows 1000000] [--steps 20] [--warmup 3] [--out FILE.json]

The rows are sampled on the host (utils.sampling.forward_sample_codes) and made resident as uint8 codes; the
columns of the two latents (VENTLUNG: 4 states, CATECHOL: 2) stay in the buffer but pgm_fit_estep never reads
them.  The plan holds the families EM re-estimates: the latents' own and their children's (6 families, all with
a latent in scope, L = 8); the CPD values are the MLE of the complete rows.  After a warm-up, from HIP events:

  estep      one pgm_fit_estep launch (the call also reads its bad-code flag back), with the log-likelihood
  wcount     one weighted pgm_fit_count launch over the same families: the floor, the same code traffic and
             one fp64 atomic per family and row where the E-step does L
  iteration  what ExpectationMaximization does per iteration: zero the tables, E-step, pgm_fit_finish, the
             log-likelihood sum, the convergence test and its one scalar back

The reference's wall time for one iteration on 1,000 of these rows is `tests/golden/make_golden_em.py --time`.
Prints one JSON line; --out also writes it to a file.
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

LATENTS = {"VENTLUNG": 4, "CATECHOL": 2}


def run(args):
    import torch

    from pgmpy_amd import engine as E
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.inference.batch import download
    from pgmpy_amd.utils import get_example_model
    from pgmpy_amd.utils.sampling import forward_sample_codes

    model = get_example_model("alarm")
    n = args.rows
    codes, nodes = forward_sample_codes(model, n, seed=args.seed)
    col, states = {v: i for i, v in enumerate(nodes)}, model.states
    assert all(len(states[v]) == k for v, k in LATENTS.items())
    em_nodes = [v for v in nodes if v in LATENTS or any(p in LATENTS for p in model.get_parents(v))]
    fams = []
    for v in em_nodes:
        scope = [v] + sorted(model.get_parents(v))
        fams.append(([col[x] for x in scope], [len(states[x]) for x in scope]))
    latent_cols = [col[v] for v in LATENTS]
    plan = FitPlan(fams)
    info = plan.estep_info(latent_cols)
    d_codes = E.to_device_raw(codes)
    values = plan.finish(plan.count(d_codes))
    d_w = E.to_device_raw(np.random.default_rng(args.seed).random(n) + 0.5)
    tables = torch.zeros(plan.total_bins, dtype=torch.float64, device=d_codes.device)
    new_values = torch.empty_like(values)

    def estep():
        tables.zero_()
        plan.estep(latent_cols, values, d_codes, tables=tables, want_loglik=True)

    def wcount():
        tables.zero_()
        plan.count(d_codes, weights=d_w, tables=tables)

    def iteration():
        tables.zero_()
        _, loglik = plan.estep(latent_cols, values, d_codes, tables=tables, want_loglik=True)
        plan.finish(tables, out=new_values)
        ll = loglik.sum()
        close = ((values - new_values).abs() <= 1e-8 + 1e-5 * new_values.abs()).all()
        return int(download(close.to(torch.uint8).reshape(1))[0]), ll

    estep_ms, estep_min = event_ms(estep, args.steps, args.warmup)
    wcount_ms, wcount_min = event_ms(wcount, args.steps, args.warmup)
    iter_ms, iter_min = event_ms(iteration, args.steps, args.warmup)
    estep()
    total = float(download(tables).sum())
    assert abs(total - len(fams) * n) <= 1e-6 * n, "every family's table must sum to the row count"
    obs_bytes = sum(sum(c not in latent_cols for c in cols) for cols, _ in fams)
    return {
        "model": "alarm", "latents": LATENTS, "rows": n, "families": len(fams), "latent_families": int(info.n_latent_families),
        "configs": int(info.n_configs), "groups": int(plan.info.n_groups), "total_bins": plan.total_bins,
        "lds_bytes": int(info.lds_bytes), "observed_code_bytes_per_row": obs_bytes,
        "estep_ms_median": estep_ms, "estep_ms_min": estep_min, "estep_rows_per_s": n / (estep_ms * 1e-3),
        "weighted_count_ms_median": wcount_ms, "weighted_count_ms_min": wcount_min,
        "estep_over_weighted_count": estep_ms / wcount_ms,
        "iteration_ms_median": iter_ms, "iteration_ms_min": iter_min, "iteration_rows_per_s": n / (iter_ms * 1e-3),
        "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
        "date": time.strftime("%Y-%m-%d"), "kind": "measured",
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native

    assert torch.cuda.is_available(), "em_bench needs a HIP device"
    _native.lib()
    res = run(args)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
