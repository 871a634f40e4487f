#!/usr/bin/env python3
"""Time the likelihood-weighted posterior (pgm_sample_posterior) on alarm and munin.

    python tools/approx_bench.py [--steps 5] [--warmup 1] [--out-dir profiles]

Per network, after a warm-up,

  posterior  one pgm_sample_posterior call (HIP events around it; the call also reads its bad-code flag
             back): alarm 10,000 evidence rows x 1,024 samples, munin 1,000 x 1,024, and on alarm one
             query with R = 1, S = 2^20.  The evidence rows are forward samples of the network with the
             target columns and a few more blanked; every family is OBSERVED.
  forward    one pgm_sample_forward launch over rows x samples rows of the same network on the same
             device: the sampler's node draws per second.  The fused kernel draws every sample twice
             (once for the row's largest log-weight, once to accumulate), so about half the sampler's
             rate is what to expect of it.
  exact      alarm only: DiscreteBayesianNetwork.predict_probability on the same 10,000 rows (the fused
             exact row plan), rows per second end to end.

Node draws per second of the posterior counts each sample's nodes once (rows x samples x nodes / time).
Prints one JSON line per case and writes profiles/approx_bench_<net>.json.
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

from tools.sample_bench import event_ms, wall_s  # noqa: E402


def case(model, name, targets, blank, R, S, args, exact=False):
    import torch

    from pgmpy_amd.inference.batch import download
    from pgmpy_amd.sampling import MISSING, BayesianModelSampling, compiled

    sampler = BayesianModelSampling(model)
    ev, nodes = sampler.forward_sample_codes(R, seed=args.seed + 1)
    c = compiled(model)
    full = download(ev) if exact else None  # before the target columns are blanked
    for v in list(targets) + list(blank):
        ev[c.col[v]].fill_(MISSING)
    values, cdf = c.tables()
    tplan = c.target_plan(tuple((v,) for v in targets))
    modes = np.full(len(c.order), 2, dtype=np.uint8)
    info = c.plan.posterior_info(tplan, R, S)
    out = {}

    def post():
        out["p"] = c.plan.posterior(tplan, values, cdf, ev, S, seed=args.seed, modes=modes)

    ms, ms_min, ms_max = event_ms(post, args.steps, args.warmup)
    ess = download(out["p"].ess)
    n_nodes = len(c.nodes)
    res = {
        "model": name, "rows": R, "samples": S, "nodes": n_nodes, "targets": len(targets),
        "observed_per_row": n_nodes - len(targets) - len(blank), "total_bins": int(info.total_bins),
        "block": int(info.block), "k": int(info.k), "lds_bytes": int(info.lds_bytes), "workgroups": int(info.workgroups),
        "posterior_ms_median": ms, "posterior_ms_min": ms_min, "posterior_ms_max": ms_max,
        "posterior_rows_per_s": R / (ms * 1e-3), "posterior_samples_per_s": R * S / (ms * 1e-3),
        "posterior_node_draws_per_s": R * S * n_nodes / (ms * 1e-3), "ess_median": float(np.median(ess)),
        "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
        "date": time.strftime("%Y-%m-%d"), "kind": "measured",
    }
    n = min(R * S, args.forward_rows)
    codes = torch.empty((n_nodes, n), dtype=torch.uint8, device=cdf.device)
    fwd_ms, _, _ = event_ms(lambda: c.plan.forward(cdf, codes, seed=args.seed), args.steps, args.warmup)
    res.update({"forward_rows": n, "forward_ms_median": fwd_ms, "forward_node_draws_per_s": n * n_nodes / (fwd_ms * 1e-3)})
    res["posterior_over_forward"] = res["posterior_node_draws_per_s"] / res["forward_node_draws_per_s"]
    del codes
    if exact:
        frame = sampler._frame(full, nodes, True)
        frame = frame[[v for v in frame.columns if v not in targets and v not in blank]]
        s, s_min, s_max = wall_s(lambda: model.predict_probability(frame), max(args.steps // 2, 2), 1)
        res.update({"exact_predict_probability_s_median": s, "exact_rows_per_s": R / s,
                    "exact_missing_variables": len(targets) + len(blank)})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--forward-rows", type=int, default=10_240_000, help="cap on the rows of the forward launch")
    ap.add_argument("--nets", nargs="+", default=["alarm", "munin"])
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native
    from pgmpy_amd.utils import get_example_model

    assert torch.cuda.is_available(), "approx_bench needs a HIP device"
    _native.lib()
    for net in args.nets:
        model = get_example_model(net)
        lines = []
        if net == "alarm":
            targets, blank = ["LVFAILURE", "HYPOVOLEMIA", "STROKEVOLUME"], []
            lines.append(case(model, net, targets, blank, 10_000, 1024, args, exact=True))
            lines.append(case(model, net, targets, blank, 1, 1 << 20, args))
        else:
            order = sorted(model.nodes())
            inner = [v for v in order if model.out_degree(v) > 0]
            targets, blank = inner[:8], inner[8:]  # the leaves are observed, eight inner nodes are queried
            lines.append(case(model, net, targets, blank, 1_000, 1024, args))
        for res in lines:
            print(json.dumps(res), flush=True)
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, f"approx_bench_{net}.json"), "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
