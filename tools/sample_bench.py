#!/usr/bin/env python3
"""Time forward sampling on munin (1,041 nodes).

    python tools/sample_bench.py [--rows 1000000] [--steps 20] [--warmup 3] [--out FILE.json]

Per row count, after a warm-up,

  forward   one pgm_sample_forward launch over all 1,041 families into a resident code matrix (HIP events
            around the call; the call also reads its bad-code flag back), unweighted and with likelihood
            weights for 8 observed leaves
  cdf       one pgm_sample_cdf launch (values -> running sums)
  total     BayesianModelSampling.forward_sample_codes end to end: allocation of the code matrix and the
            launch (the plan and the running sums are cached on the model after the first call, which
            is timed separately as the cold call)

and rows/s plus the fraction of the HBM peak under the byte model "bytes per row = 1 code byte written
per node + 1 code byte read back per edge" (munin: 1,041 + 1,397; the running sums, under 1 MB, stay
cache-resident and are not counted).  The same-host baseline is the host generator this replaces,
pgmpy_amd.utils.sampling.forward_sample_codes (numpy, one core), which is followed by an upload when the
rows are needed on the device.  The device codes are checked against tests/sample_cases.py's numpy
restatement on the first 2,048 rows.  Prints one JSON line per row count; --out also writes them to a file.
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


def event_ms(fn, steps, warmup):
    """Median, min, max of `steps` timings of fn() between HIP events on the current stream."""
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
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def wall_s(fn, steps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def run(model, n, args):
    import torch

    from pgmpy_amd import engine as E
    from pgmpy_amd.inference.batch import download
    from pgmpy_amd.sampling import BayesianModelSampling, compiled
    from pgmpy_amd.sampling._sample import OBSERVED
    from pgmpy_amd.utils.sampling import forward_sample_codes as host_sample
    from tests import sample_cases as S

    sampler = BayesianModelSampling(model)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sampler.forward_sample_codes(1024, seed=args.seed)  # the cold call: plan, upload of the CPDs, running sums
    torch.cuda.synchronize()
    cold_s = time.perf_counter() - t0
    c = compiled(model)
    values, cdf = c.tables()
    plan = c.plan
    edges = sum(len(cols) - 1 for cols, _ in plan.families)
    bytes_per_row = len(plan.families) + edges
    codes = torch.empty((len(c.nodes), n), dtype=torch.uint8, device=cdf.device)
    weights = torch.empty(n, dtype=torch.float64, device=cdf.device)

    fwd_ms, fwd_min, fwd_max = event_ms(lambda: plan.forward(cdf, codes, seed=args.seed), args.steps, args.warmup)
    vec4 = int(plan.launch_info(codes.data_ptr(), n, 0).vec4)
    got = download(codes[:, :2048].contiguous())
    nodes, order, fams, tables = S.model_plan(model)
    want, _, _ = S.sample_ref(fams, tables, 2048, seed=args.seed, n_cols=len(nodes))
    assert nodes == c.nodes and np.array_equal(got, want), "device codes differ from the numpy restatement"

    leaves = sorted(v for v in model.nodes() if model.out_degree(v) == 0)[:8]
    modes = np.zeros(len(c.order), dtype=np.uint8)
    for v in leaves:
        modes[c.family_of[v]] = OBSERVED
        codes[c.col[v]].fill_(0)
    lw_ms, _, _ = event_ms(lambda: plan.forward(cdf, codes, seed=args.seed, modes=modes, values=values, weights=weights),
                           max(args.steps // 2, 3), 1)
    cdf_ms, _, _ = event_ms(lambda: plan.cdf(values, out=cdf), args.steps, args.warmup)

    e2e_s, e2e_min, e2e_max = wall_s(lambda: sampler.forward_sample_codes(n, seed=args.seed), max(args.steps // 2, 3), 1)

    t0 = time.perf_counter()
    host_codes, _ = host_sample(model, n, seed=args.seed)
    host_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    E.to_device_raw(host_codes)
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t0
    gbs = bytes_per_row * n / (fwd_ms * 1e-3) / 1e9
    return {
        "model": "munin", "rows": n, "families": len(plan.families), "edges": edges, "total_bins": plan.total_bins,
        "cdf_bytes": plan.total_bins * 8, "code_bytes_per_row": bytes_per_row, "four_rows_per_lane": vec4,
        "forward_ms_median": fwd_ms, "forward_ms_min": fwd_min, "forward_ms_max": fwd_max,
        "forward_rows_per_s": n / (fwd_ms * 1e-3), "forward_model_GBs": gbs, "forward_frac_hbm_peak": gbs / HBM_PEAK_GBS,
        "hbm_peak_GBs": HBM_PEAK_GBS, "weighted_forward_ms_median": lw_ms, "cdf_ms_median": cdf_ms,
        "forward_sample_codes_s_median": e2e_s, "forward_sample_codes_s_min": e2e_min,
        "forward_sample_codes_s_max": e2e_max, "forward_sample_codes_rows_per_s": n / e2e_s,
        "forward_sample_codes_cold_1024_rows_s": cold_s,
        "host_numpy_s_one_core": host_s, "host_numpy_rows_per_s": n / host_s, "host_upload_s": upload_s,
        "forward_speedup_vs_host_numpy": host_s / (fwd_ms * 1e-3), "end_to_end_speedup_vs_host_numpy": host_s / e2e_s,
        "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
        "date": time.strftime("%Y-%m-%d"), "kind": "measured",
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native
    from pgmpy_amd.utils import get_example_model

    assert torch.cuda.is_available(), "sample_bench needs a HIP device"
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
