#!/usr/bin/env python3
"""Time DiscreteBayesianNetwork.fit on munin (1,041 nodes) over forward-sampled rows.

    python tools/fit_bench.py [--rows 100000 1000000] [--steps 20] [--warmup 3] [--out FILE.json]

Per row count: the rows are sampled on the host (utils.sampling.forward_sample_codes), the uint8 codes
are made resident on the device, then, after a warm-up,

  count    one pgm_fit_count launch over all 1,041 families (HIP events around the call; the call also
           reads its bad-code flag back), MLE (int64) and weighted (fp64)
  finish   one pgm_fit_finish launch (counts -> every CPD's values)
  total    model.fit(frame) from a categorical DataFrame of the same rows to CPDs on the device: host
           state-name collection and encoding, upload, both launches

and rows/s plus the fraction of the HBM peak under the byte model "code bytes read per row = sum over
families of (1 + parents)" (munin: 1,041 + its edges; weights add 8 B per family and row when weighted).
The same-host CPU baseline is this file's np.bincount restatement of the count (one core).  Prints one
JSON line per row count; --out also writes them to a file.
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

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec


def families_of(model, nodes):
    col = {v: i for i, v in enumerate(nodes)}
    states = model.states
    fams = []
    for n in nodes:
        scope = [n] + sorted(model.get_parents(n))
        fams.append(([col[v] for v in scope], [len(states[v]) for v in scope]))
    return fams


def bincount_counts(codes, fams):
    """The count tables on the host: one np.bincount per family (no missing codes in sampled rows)."""
    out = []
    for cols, cards in fams:
        idx = np.zeros(codes.shape[1], dtype=np.int64)
        for c, k in zip(cols, cards):
            idx *= k
            idx += codes[c]
        out.append(np.bincount(idx, minlength=int(np.prod(cards))))
    return np.concatenate(out)


def event_ms(fn, steps, warmup):
    """Median, min of `steps` timings of fn() between HIP events on the current stream."""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def run(model, n, args):
    import pandas as pd
    import torch

    from pgmpy_amd import engine as E
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.inference.batch import download
    from pgmpy_amd.models import DiscreteBayesianNetwork
    from pgmpy_amd.utils.sampling import forward_sample_codes

    t0 = time.perf_counter()
    codes, nodes = forward_sample_codes(model, n, seed=args.seed)
    sample_s = time.perf_counter() - t0
    fams = families_of(model, nodes)
    bytes_per_row = sum(len(cols) for cols, _ in fams)
    plan = FitPlan(fams)
    d_codes = E.to_device_raw(codes)
    d_w = E.to_device_raw(np.random.default_rng(args.seed).random(n) + 0.5)
    tables = torch.zeros(plan.total_bins, dtype=torch.int64, device=d_codes.device)
    wtables = torch.zeros(plan.total_bins, dtype=torch.float64, device=d_codes.device)
    values = torch.empty(plan.total_bins, dtype=torch.float64, device=d_codes.device)

    def count():
        tables.zero_()
        plan.count(d_codes, tables=tables)

    def wcount():
        wtables.zero_()
        plan.count(d_codes, weights=d_w, tables=wtables)

    count_ms, count_min = event_ms(count, args.steps, args.warmup)
    wcount_ms, _ = event_ms(wcount, max(args.steps // 4, 3), 1)
    finish_ms, _ = event_ms(lambda: plan.finish(tables, out=values), args.steps, args.warmup)
    got = download(tables)

    t0 = time.perf_counter()
    want = bincount_counts(codes, fams)
    cpu_s = time.perf_counter() - t0
    assert np.array_equal(got, want), "device counts differ from the bincount restatement"

    # frame -> CPDs: a categorical frame of the same rows through the public fit
    states = model.states
    frame = pd.DataFrame({v: pd.Categorical.from_codes(codes[i].astype(np.int8), categories=list(states[v]))
                          for i, v in enumerate(nodes)})
    bn = DiscreteBayesianNetwork(list(model.edges()))
    bn.add_nodes_from(model.nodes())
    total_s = []
    for _ in range(2):  # the second run is the warm one
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bn.fit(frame, state_names={v: list(states[v]) for v in nodes})
        torch.cuda.synchronize()
        total_s.append(time.perf_counter() - t0)
    gbs = bytes_per_row * n / (count_ms * 1e-3) / 1e9
    return {
        "model": "munin", "rows": n, "families": len(fams), "groups": int(plan.info.n_groups),
        "total_bins": plan.total_bins, "code_bytes_per_row": bytes_per_row,
        "count_ms_median": count_ms, "count_ms_min": count_min, "count_rows_per_s": n / (count_ms * 1e-3),
        "count_model_GBs": gbs, "count_frac_hbm_peak": gbs / HBM_PEAK_GBS, "hbm_peak_GBs": HBM_PEAK_GBS,
        "weighted_count_ms_median": wcount_ms, "finish_ms_median": finish_ms,
        "fit_frame_to_cpds_s": total_s, "fit_rows_per_s_warm": n / total_s[-1],
        "cpu_bincount_s_one_core": cpu_s, "cpu_bincount_rows_per_s": n / cpu_s,
        "count_speedup_vs_cpu_bincount": cpu_s / (count_ms * 1e-3), "host_sampling_s": sample_s,
        "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
        "date": time.strftime("%Y-%m-%d"), "kind": "measured",
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

    assert torch.cuda.is_available(), "fit_bench needs a HIP device"
    _native.lib()
    model = get_example_model("munin")
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
