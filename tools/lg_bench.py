#!/usr/bin/env python3
"""Time the linear-Gaussian kernels (pgm_lg_colsum, pgm_lg_gram, pgm_lg_sample, pgm_lg_logpdf) on a resident
fp64 value matrix, beside torch's own fp64 X @ X.T on the same tensor.

    python tools/lg_bench.py [--rows 1000000] [--widths 37 128 1041] [--steps 10] [--warmup 2]

Per width d (37 and 1,041 are alarm's and munin's; 128 is the first sizes above one wave's 64 columns) a
network in which node j has the parents j - 1, j - 2, j - 3 is sampled into a [d, rows] device matrix
(simulate_values) and stays there.  Timings are medians of `steps` repetitions between HIP events after
`warmup` untimed ones (tools/fit_bench.py event_ms):
  colsum   one pgm_lg_colsum over all columns
  gram     one pgm_lg_gram (the MFMA kernel and its slice reduction)
  sample   one pgm_lg_sample of all rows
  logpdf   one pgm_lg_logpdf with its total
  torch    torch.matmul(X, X.T) in fp64 (no shift, no ones column: the comparison, not a replacement)
Reported: for d + 1 <= 64 the matrix bytes over the Gram time against the achievable HBM rate (the data is read
once); for every d the flops of the MFMAs as issued (2 x 16 x 16 x 4 each, the padding of the last tile included)
against the fp64 matrix peak.  Writes profiles/lg_bench.json.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.fit_bench import HBM_PEAK_GBS, event_ms  # noqa: E402

HBM_ACHIEVABLE_GBS = 6300.0  # a streaming copy on this part reaches about 79 % of the 8 TB/s specification
F64_MATRIX_PEAK = 78.6e12    # MI355X specification: fp64 matrix flop/s


def chain_model(d):
    from pgmpy_amd.factors.continuous import LinearGaussianCPD
    from pgmpy_amd.models import LinearGaussianBayesianNetwork

    names = [f"v{j:04d}" for j in range(d)]
    m = LinearGaussianBayesianNetwork()
    m.add_nodes_from(names)
    for j, v in enumerate(names):
        parents = names[max(0, j - 3):j]
        m.add_edges_from((u, v) for u in parents)
        m.add_cpds(LinearGaussianCPD(v, [0.5] + [0.25] * len(parents), 1.0, parents))
    return m, names


def run(d, n, args):
    import torch

    from pgmpy_amd import _native as N
    from pgmpy_amd.models._lg import GramPlan

    m, names = chain_model(d)
    X = m.simulate_values(n, seed=args.seed)
    plan = GramPlan(list(range(d)))
    sums, counts = plan.colsum(X)
    shift = (sums / counts.to(torch.float64)).contiguous()
    out = torch.zeros((d + 1, d + 1), dtype=torch.float64, device=X.device)
    colsum_ms, colsum_min = event_ms(lambda: plan.colsum(X), args.steps, args.warmup)
    gram_ms, gram_min = event_ms(lambda: plan.gram(X, shift, out=out), args.steps, args.warmup)
    sample_ms, sample_min = event_ms(lambda: m.simulate_values(n, seed=args.seed, out=X), max(args.steps // 2, 3), 1)
    logpdf_ms, logpdf_min = event_ms(lambda: m.log_likelihood_values(X, names), max(args.steps // 2, 3), 1)
    torch_ms, torch_min = event_ms(lambda: torch.matmul(X, X.T), max(args.steps // 2, 3), 1)
    # the device's S against torch's own centred product: a plausibility check, not a test
    Xc = X - X.mean(dim=1, keepdim=True)
    ref = Xc @ Xc.T
    g = out[:d, d:d + 1]
    S = out[:d, :d] - g @ g.T / n
    rel = float(((S - ref).abs().max() / ref.abs().max()).cpu())

    groups = plan.groups()
    slice_rows, n_slices, vec16 = plan.gram_info(n, X.data_ptr(), int(X.shape[1]), 0)
    tiles = int(plan.info.n_tiles)

    def group_mfmas(I, J):
        ta, tb = min(4, tiles - 4 * I), min(4, tiles - 4 * J)
        return ta * (ta + 1) // 2 if I == J else ta * tb

    steps = -(-n // N.LG_STEP)
    mfmas = sum(group_mfmas(I, J) for I, J in groups) * steps * N.LG_ROWS_PER_LANE
    flops = mfmas * 2 * 16 * 16 * 4
    t = gram_ms * 1e-3
    bytes_once = n * d * 8
    bytes_groups = sum((min(4, tiles - 4 * I) + (0 if I == J else min(4, tiles - 4 * J))) for I, J in groups) * 16 * 8 * n
    return {
        "d": d, "rows": n, "tiles": tiles, "groups": len(groups), "single_wave": bool(plan.info.single_wave),
        "slice_rows": slice_rows, "slices": n_slices, "vec16": vec16, "matrix_bytes": bytes_once,
        "colsum_ms_median": colsum_ms, "colsum_ms_min": colsum_min, "colsum_GBs": bytes_once / (colsum_ms * 1e-3) / 1e9,
        "gram_ms_median": gram_ms, "gram_ms_min": gram_min, "gram_GBs_once": bytes_once / t / 1e9,
        "gram_frac_hbm_achievable": bytes_once / t / 1e9 / HBM_ACHIEVABLE_GBS if plan.info.single_wave else None,
        "gram_operand_GBs_requested": bytes_groups / t / 1e9,
        "gram_mfma_instructions": mfmas, "gram_flops_issued": flops, "gram_flops_per_s": flops / t,
        "gram_frac_f64_matrix_peak": flops / t / F64_MATRIX_PEAK,
        "sample_ms_median": sample_ms, "sample_ms_min": sample_min, "sample_GBs_written": bytes_once / (sample_ms * 1e-3) / 1e9,
        "logpdf_ms_median": logpdf_ms, "logpdf_ms_min": logpdf_min, "logpdf_GBs_read": bytes_once / (logpdf_ms * 1e-3) / 1e9,
        "torch_matmul_ms_median": torch_ms, "torch_matmul_ms_min": torch_min,
        "torch_flops_per_s": 2.0 * n * d * d / (torch_ms * 1e-3), "gram_over_torch": gram_ms / torch_ms,
        "S_rel_diff_vs_torch_centred": rel, "hbm_peak_GBs": HBM_PEAK_GBS, "hbm_achievable_GBs": HBM_ACHIEVABLE_GBS,
        "f64_matrix_peak_flops": F64_MATRIX_PEAK, "steps": args.steps, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "kind": "measured",
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--widths", type=int, nargs="+", default=[37, 128, 1041])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lg_bench.json"))
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native

    assert torch.cuda.is_available(), "lg_bench needs a HIP device"
    _native.lib()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    lines = []
    for d in args.widths:
        res = run(d, args.rows, args)
        print(json.dumps(res), flush=True)
        lines.append(res)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
