#!/usr/bin/env python3
"""Time the pairwise-count path (pgm_pair_count, pgm_pair_mi, pgm_pair_emi, a full TreeSearch.estimate) on
alarm and munin over rows sampled on the device, beside the same pair tables through FitPlan.count.

    python tools/pair_bench.py [--nets alarm munin] [--rows 100000 1000000] [--steps 20] [--warmup 3]

Per network and row count the uint8 codes are sampled into device memory and stay there
(BayesianModelSampling.forward_sample_codes).  Timings are medians of `steps` repetitions between HIP events
after `warmup` untimed ones (tools/fit_bench.py event_ms):
  pair_count   one pgm_pair_count over all columns into a zeroed [Sp, Sp] int64 table
  fit_count    the same tables through FitPlan.count, the family-count kernel: every pair (u, v) as the
               family (u | v).  alarm: all 666 pairs; munin: the pairs of the first 64 columns, scaled by
               the ratio of pair numbers (`fit_pairs`, `fit_scaled`)
  pair_mi      one pgm_pair_mi over the table
  pair_emi     one pgm_pair_emi (alarm only: the hypergeometric sums grow with rows x pairs; on munin it
               is not run)
  estimate     one full Chow-Liu estimate (mutual_info) on the resident codes, wall clock: count, statistics,
               download, spanning tree on the host
and the int8 multiply-add rate of the count against 2 x the bf16 MFMA peak, with the operand bytes its
lanes ask for per second, which says which pipe limits it.  Writes profiles/pair_bench_<net>.json.
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

I8_PEAK_OPS = 2 * 2.5e15  # 2 x the dense bf16 MFMA peak of the microarchitecture guide, multiply and add counted
FIT_COLUMNS = 64  # munin: the columns whose pairs go through FitPlan.count


def run(net, model, n, args):
    import torch

    from pgmpy_amd.estimators import BaseEstimator
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.estimators._pairs import PairPlan
    from pgmpy_amd.estimators.TreeSearch import tree_search
    from pgmpy_amd.inference.batch import download
    from pgmpy_amd.sampling import BayesianModelSampling

    d_codes, nodes = BayesianModelSampling(model).forward_sample_codes(n, seed=args.seed)
    states = model.states
    cards = [len(states[v]) for v in nodes]
    n_vars = len(nodes)
    plan = PairPlan(list(range(n_vars)), cards)
    counts = torch.zeros((1, plan.Sp, plan.Sp), dtype=torch.int64, device=d_codes.device)

    def pair_count():
        counts.zero_()
        plan.count(d_codes, counts=counts)

    zero_ms, _ = event_ms(counts.zero_, args.steps, args.warmup)
    count_ms, count_min = event_ms(pair_count, args.steps, args.warmup)
    mi_ms, mi_min = event_ms(lambda: plan.mi(counts), args.steps, args.warmup)
    emi_ms = emi_min = None
    if net == "alarm":
        emi_ms, emi_min = event_ms(lambda: plan.emi(counts), max(args.steps // 4, 3), 1)

    # the same tables through the family-count kernel
    fit_vars = n_vars if net == "alarm" else min(FIT_COLUMNS, n_vars)
    fams = [([u, v], [cards[u], cards[v]]) for u in range(fit_vars) for v in range(u + 1, fit_vars)]
    fplan = FitPlan(fams)
    tables = torch.zeros(fplan.total_bins, dtype=torch.int64, device=d_codes.device)

    def fit_count():
        tables.zero_()
        fplan.count(d_codes, tables=tables)

    fit_ms, fit_min = event_ms(fit_count, args.steps, args.warmup)
    host_counts, host_tables = download(counts), download(tables)
    for f in range(0, len(fams), max(1, len(fams) // 200)):  # the two paths agree, cell by cell
        u, v = fams[f][0]
        assert np.array_equal(np.asarray(plan.block(host_counts, u, v)), fplan.table(host_tables, f)), (u, v)
    scale = plan.n_pairs / len(fams)

    # one full estimate on the resident codes: the estimator is handed its encoded columns
    est = BaseEstimator()
    est.variables, est.state_names = list(nodes), {v: list(states[v]) for v in nodes}
    est._encoded = (d_codes, {v: j for j, v in enumerate(nodes)})
    est_s = []
    for _ in range(2):  # the second run is the warm one
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dag, root = tree_search(est, list(nodes), None, "chow-liu", None, "mutual_info")
        torch.cuda.synchronize()
        est_s.append(time.perf_counter() - t0)

    groups = plan.groups()
    slice_rows, n_slices, vec16 = plan.count_info(n, codes_ptr=d_codes.data_ptr(), ld=int(d_codes.shape[1]))
    steps = -(-n // 64)
    mfmas = sum(10 if I == J else 16 for I, J, _ in groups) * steps
    macs = mfmas * 16 * 16 * 64
    frag_bytes = len(groups) * steps * 8 * 64 * 16  # 8 fragments of 64 lanes x 16 bytes per group and step
    t = count_ms * 1e-3
    return {
        "model": net, "rows": n, "variables": n_vars, "S": plan.S, "Sp": plan.Sp, "pairs": plan.n_pairs,
        "tile_pairs": int(plan.info.n_tile_pairs), "groups": len(groups), "slice_rows": slice_rows, "slices": n_slices,
        "vec16": vec16, "count_table_bytes": plan.count_bytes(1), "zero_ms_median": zero_ms,
        "pair_count_ms_median": count_ms, "pair_count_ms_min": count_min,
        "pair_mi_ms_median": mi_ms, "pair_mi_ms_min": mi_min, "pair_emi_ms_median": emi_ms, "pair_emi_ms_min": emi_min,
        "fit_pairs": len(fams), "fit_count_ms_median": fit_ms, "fit_count_ms_min": fit_min, "fit_scale": scale,
        "fit_count_ms_scaled": fit_ms * scale, "fit_scaled": scale != 1.0,
        "pair_over_fit": count_ms / (fit_ms * scale),
        "mfma_instructions": mfmas, "int8_ops_per_s": 2 * macs / t, "int8_peak_ops_per_s": I8_PEAK_OPS,
        "int8_fraction_of_peak": 2 * macs / t / I8_PEAK_OPS,
        "useful_macs": n * plan.S * plan.S / 2, "operand_bytes_requested": frag_bytes,
        "operand_GBs_requested": frag_bytes / t / 1e9, "codes_bytes": n * n_vars, "codes_GBs_once": n * n_vars / t / 1e9,
        "hbm_peak_GBs": HBM_PEAK_GBS, "estimate_chow_liu_s": est_s, "estimate_edges": dag.number_of_edges(),
        "estimate_root": str(root), "steps": args.steps, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "kind": "measured",
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nets", nargs="+", default=["alarm", "munin"])
    ap.add_argument("--rows", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native
    from pgmpy_amd.utils import get_example_model

    assert torch.cuda.is_available(), "pair_bench needs a HIP device"
    _native.lib()
    os.makedirs(args.out_dir, exist_ok=True)
    for net in args.nets:
        model = get_example_model(net)
        lines = []
        for n in args.rows:
            res = run(net, model, n, args)
            print(json.dumps(res), flush=True)
            lines.append(res)
            with open(os.path.join(args.out_dir, f"pair_bench_{net}.json"), "w") as f:
                json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
