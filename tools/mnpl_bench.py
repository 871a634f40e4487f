#!/usr/bin/env python3
"""Time the pseudo-likelihood fit of a Markov network (csrc/pgmmnpl.hip k_mn_pl, k_mn_pl_gather) on the Potts grid of
tools/mplp_bench.py and tools/lbp_bench.py.

    python tools/mnpl_bench.py [--side 16] [--states 4] [--rows 1000000] [--sweeps 30] [--steps 5] [--warmup 2]
                               [--out profiles/mnpl_bench.json]

The rows are drawn on the device (GibbsSampling.sample_codes: `rows` chains after `sweeps` sweeps) from the side x
side grid with psi = exp(J eye) on every edge, and stay there.  One run records: the one-off count of the blanket
families (pgm_fit_count); one evaluation of the objective and its gradient (pgm_mnpl_eval, both launches; `batch`
evaluations between two HIP events, divided); a full estimate() from theta = 0 (host clock around a synchronise), its
iterations and evaluations, and its split into kernel time (evaluations x the time of one) and the rest, the Python /
L-BFGS loop; one pgm_gibbs_sweep over the same rows, which is what an evaluation that streamed the rows would cost at
the least; and the numpy restatement of one evaluation from the same count tables on the host (wall clock), with the
gap of the device's value and gradient to it.  HIP events, `warmup` untimed runs, the median and minimum of `steps`.
Not measured: cardinalities past the LDS tier (there is none), hardware counters.  A run that finds no device fails.
Prints one JSON line; --out also writes it.
"""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.fit_bench import event_ms  # noqa: E402


def host_eval(plan, counts, theta):
    """(value, grad) of one evaluation from the count tables, in numpy fp64: per node, the logits of every blanket
    configuration by broadcasting the incident tables over the node's table."""
    value, grad = 0.0, np.zeros_like(theta)
    for i, (cols, cards) in enumerate(plan.families):
        at = plan.count_offsets[i]
        n = counts[at:at + int(np.prod(cards))].reshape(cards).astype(np.float64)
        logit, views = np.zeros(cards), []
        for f, (fcols, fcards) in enumerate(plan.factors):
            if i not in fcols:
                continue
            perm = sorted(range(len(fcols)), key=lambda a: cols.index(fcols[a]))
            shape = [k if c in fcols else 1 for c, k in zip(cols, cards)]
            table = theta[plan.offsets[f]:plan.offsets[f] + plan.sizes[f]].reshape(fcards)
            logit = logit + table.transpose(perm).reshape(shape)
            views.append((f, perm))
        top = logit.max(0)
        rel = logit - (top + np.log(np.exp(logit - top).sum(0)))
        value += float((n * rel).sum())
        resid = n - n.sum(0) * np.exp(rel)
        for f, perm in views:
            part = resid.sum(tuple(d for d, c in enumerate(cols) if c not in plan.factors[f][0]))  # axes in blanket order
            grad[plan.offsets[f]:plan.offsets[f] + plan.sizes[f]] += part.transpose(np.argsort(perm)).ravel()
    return value, grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16)
    ap.add_argument("--states", type=int, default=4)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--sweeps", type=int, default=30)
    ap.add_argument("--coupling", type=float, default=0.5)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native
    from pgmpy_amd.estimators import PseudoLikelihoodEstimator
    from pgmpy_amd.factors.discrete import DiscreteFactor
    from pgmpy_amd.models import DiscreteMarkovNetwork
    from pgmpy_amd.sampling import GibbsSampling
    from pgmpy_amd.sampling.gibbs import gibbs_compiled

    assert torch.cuda.is_available(), "mnpl_bench needs a HIP device"
    _native.lib()
    n, k = args.side, args.states
    at = lambda r, c: r * n + c
    edges = [(at(r, c), at(r, c + 1)) for r in range(n) for c in range(n - 1)]
    edges += [(at(r, c), at(r + 1, c)) for r in range(n - 1) for c in range(n)]
    names = [f"x{v:03d}" for v in range(n * n)]
    grid = DiscreteMarkovNetwork()
    grid.add_nodes_from(names)
    grid.add_edges_from((names[a], names[b]) for a, b in edges)
    grid.add_factors(*[DiscreteFactor([names[a], names[b]], [k, k], np.exp(args.coupling * np.eye(k))) for a, b in edges])
    codes, nodes = GibbsSampling(grid).sample_codes(args.rows, args.sweeps, seed=1)
    assert nodes == names
    est = PseudoLikelihoodEstimator.from_codes(grid, codes)
    plan, counts, _ = est._build()
    fit = plan.fit_plan()
    count_ms = event_ms(lambda: fit.count(codes), args.steps, args.warmup)
    theta = torch.zeros(plan.n_theta, dtype=torch.float64, device="cuda")
    many = lambda: [plan.eval(counts, theta) for _ in range(args.batch)]
    eval_ms = [t / args.batch for t in event_ms(many, args.steps, args.warmup)]
    c = gibbs_compiled(grid, False)
    scratch = codes.clone()
    sweep_ms = event_ms(lambda: c.plan.sweep(c.tables(), scratch, 1, seed=2), args.steps, args.warmup)
    est.estimate()  # warm: the optimiser's own kernels
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    est.estimate()
    torch.cuda.synchronize()
    fit_ms = (time.perf_counter() - t0) * 1e3
    fitted = est.theta
    value, grad = est.value_and_grad(fitted)
    host_counts, host_theta = counts.cpu().numpy(), fitted.cpu().numpy()
    t0 = time.perf_counter()
    want_value, want_grad = host_eval(plan, host_counts, host_theta)
    host_ms = (time.perf_counter() - t0) * 1e3
    gap_value = abs(float(value[0]) - want_value) / abs(want_value)
    gap_grad = float(np.abs(grad.cpu().numpy() - want_grad).max()) / args.rows
    assert gap_value < 1e-12 and gap_grad < 1e-12, (gap_value, gap_grad)
    # the couplings the fit recovers: theta_f(s, s) - theta_f(s, t) averaged per edge is gauge-free on a pair table
    tables = host_theta.reshape(len(edges), k, k)
    diag = np.einsum("fss->f", tables) / k
    coupling = float(np.mean(diag - (tables.sum((1, 2)) - k * diag) / (k * k - k)))
    info = plan.info
    out = {"workload": "potts_pseudo_likelihood_fit", "side": n, "states": k, "rows": args.rows, "sweeps": args.sweeps,
           "factors": int(info.n_factors), "theta_entries": plan.n_theta, "count_entries": plan.n_counts,
           "lds_bytes": int(info.lds_bytes), "count_ms_median": count_ms[0], "count_ms_min": count_ms[1],
           "eval_ms_median": eval_ms[0], "eval_ms_min": eval_ms[1], "eval_batch": args.batch,
           "gibbs_sweep_ms_median": sweep_ms[0], "gibbs_sweep_ms_min": sweep_ms[1],
           "estimate_ms": fit_ms, "estimate_iterations": est.n_iter, "estimate_evaluations": est.n_eval,
           "estimate_converged": bool(est.converged), "estimate_kernel_ms": est.n_eval * eval_ms[0],
           "estimate_loop_ms": fit_ms - est.n_eval * eval_ms[0], "host_restatement_eval_ms": host_ms,
           "value_gap_to_restatement_rel": gap_value, "grad_gap_to_restatement_per_row": gap_grad,
           "coupling_true": args.coupling, "coupling_fitted_mean": coupling, "steps": args.steps, "warmup": args.warmup,
           "not_measured": ["cardinalities past the LDS tier", "hardware counters"],
           "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "tool": "tools/mnpl_bench.py",
           "kind": "measured"}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump([out], f)
            f.write("\n")


if __name__ == "__main__":
    main()
