#!/usr/bin/env python3
"""Time the per-row log-probability pass (pgm_fit_logprob) on resident codes.

    python tools/logp_bench.py [--nets munin alarm] [--rows 1000000] [--steps 20] [--warmup 3]

Per network, after a warm-up, over `rows` forward-sampled rows that stay on the device,

  logprob      one pgm_fit_logprob call with per-row output, total and skipped count (HIP events around the
               call; the call also reads its bad-code flag back), on the four-rows-per-lane path and, over
               the same rows shifted by one, on the one-row path
  total_only   the same call without the per-row output
  log_values   one pgm_fit_log_values launch (values -> log tables)
  end_to_end   BayesianModelProbability.log_probability_codes (the log tables are cached on the model after
               the first call, which is timed separately as the cold call)

and rows/s plus the fraction of the achievable HBM rate under the byte model "bytes per row = 1 code byte
read per (family, variable) + 8 bytes written" (munin: 1,041 + 1,397 + 8; a parent's column is read once
per family that lists it; the log tables, a few hundred KiB, stay cache-resident and are not counted).
The first 2,048 device rows are checked against tests/logp_cases.py's long-double restatement and the total
against its fixed-order sum.  Writes profiles/logp_bench_<net>.json and prints one JSON line per network.
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

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec
HBM_ACHIEVABLE_GBS = 6300.0  # what a streaming copy reaches on it (79 % of the spec)


def run(net, n, args):
    import torch

    from pgmpy_amd.inference.batch import download
    from pgmpy_amd.metrics import BayesianModelProbability
    from pgmpy_amd.sampling import BayesianModelSampling, compiled
    from pgmpy_amd.utils import get_example_model
    from tests import logp_cases as LC
    from tests import sample_cases as S

    model = get_example_model(net)
    n = n // 4 * 4
    codes, nodes = BayesianModelSampling(model).forward_sample_codes(n + 4, seed=args.seed)
    bmp = BayesianModelProbability(model)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bmp.log_probability_codes(codes, n_rows=1024)  # the cold call: the fit plan, the normalised log tables
    torch.cuda.synchronize()
    cold_s = time.perf_counter() - t0
    c = compiled(model)
    plan, logv = c._logp
    values, _ = c.tables()
    reads = sum(len(cols) for cols, _ in plan.families)
    bytes_per_row = reads + 8
    logp = torch.empty(n + 4, dtype=torch.float64, device=codes.device)

    def launch(row0):
        return plan.logprob(logv, codes, n_rows=n, row0=row0, logp=logp, total=True)

    assert plan.logprob_info(codes.data_ptr(), n + 4, 0, n).vec4 == 1 and plan.logprob_info(codes.data_ptr(), n + 4, 1, n).vec4 == 0
    v4_ms, v4_min, v4_max = event_ms(lambda: launch(0), args.steps, args.warmup)
    _, total, skipped = launch(0)
    got = download(logp)[:n]
    v1_ms, v1_min, v1_max = event_ms(lambda: launch(1), max(args.steps // 2, 3), 1)

    from pgmpy_amd import _native as N

    tot = torch.empty(1, dtype=torch.float64, device=codes.device)
    lib = N.lib()

    def total_only():  # no per-row output
        N.check(lib.pgm_fit_logprob(plan._h, N.ptr(logv), N.ptr(codes), int(codes.shape[0]), n + 4, 0, n, None, N.ptr(tot), None,
                                    N.stream_handle()), "fit_logprob")

    to_ms, _, _ = event_ms(total_only, args.steps, args.warmup)
    lv_ms, _, _ = event_ms(lambda: plan.log_values(values), args.steps, args.warmup)
    e2e_s, e2e_min, e2e_max = wall_s(lambda: bmp.log_probability_codes(codes, n_rows=n), max(args.steps // 2, 3), 1)

    # correctness of what was timed
    _, _, fams, tables = S.model_plan(model)
    head = download(codes[:, :2048].contiguous())
    _, exact, mag, sk, invalid = LC.restate(fams, LC.normalized(tables), head)
    assert not sk.any() and not invalid and skipped == 0
    assert (np.abs(got[:2048].astype(np.longdouble) - exact) <= LC.row_bound(len(fams), mag)).all(), "rows differ from the restatement"
    total = float(download(total)[0])
    assert np.float64(total).tobytes() == np.float64(LC.total_fixed_order(got)).tobytes(), "total is not the fixed-order sum"
    assert np.float64(total).tobytes() == np.float64(download(tot)[0]).tobytes()

    gbs = bytes_per_row * n / (v4_ms * 1e-3) / 1e9
    return {
        "model": net, "rows": n, "families": len(plan.families), "code_reads_per_row": reads, "bytes_per_row": bytes_per_row,
        "total_bins": plan.total_bins, "log_table_bytes": plan.total_bins * 8,
        "logprob_ms_median": v4_ms, "logprob_ms_min": v4_min, "logprob_ms_max": v4_max,
        "logprob_rows_per_s": n / (v4_ms * 1e-3), "logprob_model_GBs": gbs,
        "logprob_frac_hbm_achievable": gbs / HBM_ACHIEVABLE_GBS, "logprob_frac_hbm_peak": gbs / HBM_PEAK_GBS,
        "hbm_achievable_GBs": HBM_ACHIEVABLE_GBS, "hbm_peak_GBs": HBM_PEAK_GBS,
        "one_row_path_ms_median": v1_ms, "one_row_path_ms_min": v1_min, "one_row_path_ms_max": v1_max,
        "total_only_ms_median": to_ms, "log_values_ms_median": lv_ms,
        "log_probability_codes_s_median": e2e_s, "log_probability_codes_s_min": e2e_min,
        "log_probability_codes_s_max": e2e_max, "log_probability_codes_cold_1024_rows_s": cold_s,
        "total": total, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
        "date": time.strftime("%Y-%m-%d"), "kind": "measured",
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nets", nargs="+", default=["munin", "alarm"])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native

    assert torch.cuda.is_available(), "logp_bench needs a HIP device"
    _native.lib()
    os.makedirs(args.out_dir, exist_ok=True)
    for net in args.nets:
        res = run(net, args.rows, args)
        print(json.dumps(res), flush=True)
        with open(os.path.join(args.out_dir, f"logp_bench_{net}.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
