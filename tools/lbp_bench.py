#!/usr/bin/env python3
"""Time LoopyBeliefPropagation (csrc/pgmlbp.hip k_lbp) beside Mplp (k_mplp) on the same grid and the numpy
restatement of tests/lbp_cases.py on the host.

    python tools/lbp_bench.py [--side 16] [--states 4] [--rows 10000] [--iters 100] [--steps 3] [--warmup 1]
                              [--out profiles/lbp_bench.json]

The workload is the side x side Potts grid of tools/mplp_bench.py with one coupling for all edges (psi = exp(J eye),
theta = J eye), its edges listed colour by colour; `rows` instances with random node terms, `iters` iterations each
with tol = 0 (none stops early), resident: one launch, all inputs and outputs on the device.  HIP events, `warmup`
untimed runs, the median and minimum of `steps`; k_lbp and k_mplp alternate in the same process.
message_cell_updates_per_s = rows x iters x n_msg / time.  The restatement runs ONE instance for the same iterations on
the host (wall clock) and the device's marginals of that row are compared with it.  Occupancy is what the LDS leaves
(tools/mplp_bench.py occupancy).  A run that finds no device fails.  Prints one JSON line; --out also writes it.
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

from tests import lbp_cases as C  # noqa: E402
from tools.fit_bench import event_ms  # noqa: E402
from tools.mplp_bench import model_of, occupancy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16)
    ap.add_argument("--states", type=int, default=4)
    ap.add_argument("--rows", type=int, default=10_000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--coupling", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native
    from pgmpy_amd.factors.discrete import DiscreteFactor
    from pgmpy_amd.inference import LoopyBeliefPropagation, Mplp
    from pgmpy_amd.models import DiscreteMarkovNetwork

    assert torch.cuda.is_available(), "lbp_bench needs a HIP device"
    _native.lib()
    n, k = args.side, args.states
    at = lambda r, c: r * n + c
    edges = [(at(r, c), at(r, c + 1)) for par in (0, 1) for r in range(n) for c in range(par, n - 1, 2)]
    edges += [(at(r, c), at(r + 1, c)) for par in (0, 1) for r in range(par, n - 1, 2) for c in range(n)]
    theta = args.coupling * np.eye(k)
    names = [f"x{v:03d}" for v in range(n * n)]
    grid = DiscreteMarkovNetwork()  # the edge factors alone: the node terms arrive per instance
    grid.add_nodes_from(names)
    grid.add_edges_from((names[a], names[b]) for a, b in edges)
    grid.add_factors(*[DiscreteFactor([names[a], names[b]], [k, k], np.exp(theta)) for a, b in edges])
    lbp = LoopyBeliefPropagation(grid)
    mplp = Mplp(model_of(([k] * (n * n), [np.zeros(k)] * (n * n), [(e, theta) for e in edges], 0)))
    gen = torch.Generator(device="cuda").manual_seed(2)
    terms = torch.randn((args.rows, lbp.n_unary), dtype=torch.float64, device="cuda", generator=gen)
    potentials = torch.exp(terms)
    run_lbp = lambda: lbp.query_batch(potentials, args.iters, 0.0)
    run_mplp = lambda: mplp.map_query_batch(terms, args.iters, 0.0, 0.0)
    ms = {"lbp": [], "mplp": []}
    for _ in range(args.warmup):
        run_lbp(), run_mplp()
    for _ in range(args.steps):  # alternating, one timing each
        ms["lbp"].append(event_ms(run_lbp, 1, 0)[0])
        ms["mplp"].append(event_ms(run_mplp, 1, 0)[0])
    got = run_lbp()
    assert bool((got.n_iter == args.iters).all()) and bool(torch.isfinite(got.values).all())
    assert bool(((got.marginals.reshape(args.rows, n * n, k).sum(-1) - 1).abs() < 1e-12).all())
    case = ([k] * (n * n), np.split(potentials[0].cpu().numpy(), n * n), [(e, np.exp(theta)) for e in edges])
    assert [tuple(s) for s in lbp.scopes] == [tuple(vs) for vs, _ in case[2]]
    t0 = time.perf_counter()
    ref = C.run(case, args.iters)
    host_ms = (time.perf_counter() - t0) * 1e3
    gap = float(np.abs(got.marginals[0].cpu().numpy() - ref["marginals"]).max())
    assert gap < 1e-9, gap
    info = lbp.plan.info
    med = float(np.median(ms["lbp"]))
    out = {"workload": "potts_batch_lbp", "side": n, "states": k, "rows": args.rows, "iters": args.iters,
           "factors": int(info.n_factors), "pairs": int(info.n_pairs), "message_cells": int(info.n_msg),
           "tables_unique": int(info.n_tables_unique), "theta_bytes": 8 * int(info.n_theta),
           "theta_unique_bytes": 8 * int(info.n_theta_unique), "ms_median": med, "ms_min": float(np.min(ms["lbp"])),
           "message_cell_updates_per_s": args.rows * args.iters * int(info.n_msg) / (med * 1e-3),
           "device_ms_per_instance": med / args.rows, "mplp_ms_median": float(np.median(ms["mplp"])),
           "mplp_ms_min": float(np.min(ms["mplp"])), "mplp_lds_bytes": int(mplp.plan.info.lds_bytes),
           "host_restatement_ms_per_instance": host_ms, "marginals_gap_to_restatement": gap,
           "residual_median": float(got.residual.median()), "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "kind": "measured"}
    out.update(occupancy(info))
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump([out], f)
            f.write("\n")


if __name__ == "__main__":
    main()
