#!/usr/bin/env python3
"""Time the rows E-step (pgm_fit_estep_rows: EM on rows with missing cells) on alarm.

    python tools/emrows_bench.py [--rows 1000000] [--steps 20] [--warmup 3] [--out profiles/emrows_bench.json]

The rows are sampled on the host and made resident as uint8 codes.  From HIP events, after a warm-up, the
median and minimum of `steps` repeats (each call also reads its flag word and its count of skipped rows back):

  missing_0 / _5 / _20   one estep_rows over all 37 families, no latent, with that share of the cells set missing
                         at random, with tables and loglik (what an EM iteration asks for); skipped_share is the
                         share of rows past a limit
  latent_rows / latent   the two latents of tools/em_bench.py (VENTLUNG, CATECHOL; 6 families, L = 8) and no missing
                         cell: one estep_rows, and pgm_fit_estep on the same input in the same run
  count                  the one-off pgm_fit_count of the 37 families at 20 % missing
  iteration              one EM iteration at 20 % missing: copy the counts, estep_rows, pgm_fit_finish, the
                         log-likelihood sum, the convergence test and its scalar back

Not measured here: hardware counters, munin.  Prints one JSON line; --out also writes it to a file.
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

from tools.em_bench import LATENTS  # noqa: E402
from tools.fit_bench import event_ms  # noqa: E402


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

    def families(vs):
        scopes = [[v] + sorted(model.get_parents(v)) for v in vs]
        return [([col[x] for x in sc], [len(states[x]) for x in sc]) for sc in scopes]

    def timed(fn):
        med, lo = event_ms(fn, args.steps, args.warmup)
        return {"ms_median": med, "ms_min": lo, "rows_per_s": n / (med * 1e-3)}

    res = {}
    # every family, no latent, cells missing at random
    plan = FitPlan(families(nodes))
    info = plan.estep_rows_info()
    d_full = E.to_device_raw(codes)
    values = plan.finish(plan.count(d_full))
    tables = torch.zeros(plan.total_bins, dtype=torch.float64, device=d_full.device)
    rng = np.random.default_rng(args.seed)
    for share in (0, 5, 20):
        holed = codes.copy()
        holed[rng.random(holed.shape) < share / 100.0] = 255
        d_codes = E.to_device_raw(holed)
        out = plan.estep_rows([], values, d_codes, tables=tables, want_loglik=True)
        res[f"missing_{share}"] = dict(timed(lambda: plan.estep_rows([], values, d_codes, tables=tables, want_loglik=True)),
                                       skipped_share=out["n_skipped"] / n,
                                       incomplete_share=float((holed == 255).any(axis=0).mean()))
    # d_codes is now the 20 % frame: the one-off count and a whole iteration
    res["count"] = timed(lambda: plan.count(d_codes))
    counts = plan.count(d_codes).to(torch.float64)
    new_values = torch.empty_like(values)

    def iteration():
        tables.copy_(counts)
        out = plan.estep_rows([], values, d_codes, tables=tables, want_loglik=True)
        plan.finish(tables, out=new_values)
        ll = torch.nan_to_num(out["loglik"], nan=0.0).sum()
        close = ((values - new_values).abs() <= 1e-8 + 1e-5 * new_values.abs()).all()
        return int(download(close.to(torch.uint8).reshape(1))[0]), ll

    res["iteration"] = timed(iteration)
    # the two latents of em_bench.py, no missing cell: the rows kernel beside the lane-per-row kernel
    em_nodes = [v for v in nodes if v in LATENTS or any(p in LATENTS for p in model.get_parents(v))]
    lplan, latent_cols = FitPlan(families(em_nodes)), [col[v] for v in LATENTS]
    lvalues = lplan.finish(lplan.count(d_full))
    ltables = torch.zeros(lplan.total_bins, dtype=torch.float64, device=d_full.device)
    res["latent_rows"] = timed(lambda: lplan.estep_rows(latent_cols, lvalues, d_full, tables=ltables, want_loglik=True))
    res["latent"] = timed(lambda: lplan.estep(latent_cols, lvalues, d_full, tables=ltables, want_loglik=True))
    res["latent_rows_over_latent"] = res["latent_rows"]["ms_median"] / res["latent"]["ms_median"]
    res.update({
        "model": "alarm", "rows": n, "families": len(nodes), "total_bins": plan.total_bins, "tile": int(info.tile),
        "lds_bytes": int(info.lds_bytes), "blocks_per_cu": int(info.blocks_per_cu), "block": int(info.block),
        "rows_per_block": int(info.rows_per_block), "latents": LATENTS, "latent_families": len(em_nodes),
        "not_measured": ["hardware counters", "munin"], "steps": args.steps, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "kind": "measured",
    })
    return res


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

    assert torch.cuda.is_available(), "emrows_bench needs a HIP device"
    _native.lib()
    res = run(args)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
