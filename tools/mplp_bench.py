#!/usr/bin/env python3
"""Time Mplp (csrc/pgmmplp.hip k_mplp) against the numpy restatement of tests/mplp_cases.py on the host.

    python tools/mplp_bench.py [--side 16] [--states 4] [--rows 10000] [--iters 100] [--steps 3] [--warmup 1]
                               [--out profiles/mplp_bench.json]

Two workloads:
  potts_batch    a side x side Potts grid of `states` states with random couplings, its edges listed colour by
                 colour (even / odd horizontal, even / odd vertical: 4 dependency levels; row-major order would
                 give a level per edge of a row); `rows` instances with random node terms, `iters` iterations each
                 (thresholds 0: none stops early) in one launch.  HIP events, `warmup` untimed runs, the median and
                 minimum of `steps`; cluster_updates_per_s = rows x iters x clusters / time; the restatement runs ONE
                 instance for the same iterations on the host (wall clock).
  tighten_query  one map_query with triplet tightening on a 4 x 4 binary grid with one diagonal per cell and random
                 signs (wall clock, host work included), and its first, pairwise run alone against the restatement.
Occupancy is what the LDS leaves: workgroups_per_cu = min(8, 160 KiB // lds_bytes), 4 waves each, of the 32 a CU
holds.  A path that finds no device fails.  Prints one JSON line per workload; --out also writes them to a file.
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

from tests import mplp_cases as M  # noqa: E402
from tools.fit_bench import event_ms  # noqa: E402


def model_of(case):
    from pgmpy_amd.factors.discrete import DiscreteFactor
    from pgmpy_amd.models import DiscreteMarkovNetwork

    card, unary, clusters, _ = case
    names = [f"x{v:03d}" for v in range(len(card))]
    model = DiscreteMarkovNetwork()
    model.add_nodes_from(names)
    factors = [DiscreteFactor([names[v]], [card[v]], unary[v]) for v in range(len(card))]
    for vs, theta in clusters:
        model.add_edge(names[vs[0]], names[vs[1]])
        factors.append(DiscreteFactor([names[v] for v in vs], [card[v] for v in vs], theta))
    model.add_factors(*factors)
    return model


def occupancy(info):
    per_cu = min(8, 163840 // int(info.lds_bytes))
    return {"lds_bytes": int(info.lds_bytes), "theta_in_lds": int(info.theta_in_lds), "workgroups_per_cu": per_cu,
            "waves_per_cu": 4 * per_cu, "wave_occupancy": 4 * per_cu / 32}


def potts_batch(args):
    import torch

    from pgmpy_amd.inference import Mplp

    n, k, rng = args.side, args.states, np.random.default_rng(1)
    at = lambda r, c: r * n + c
    edges = [(at(r, c), at(r, c + 1)) for par in (0, 1) for r in range(n) for c in range(par, n - 1, 2)]
    edges += [(at(r, c), at(r + 1, c)) for par in (0, 1) for r in range(par, n - 1, 2) for c in range(n)]
    case = ([k] * (n * n), [rng.normal(size=k) for _ in range(n * n)],
            [(e, rng.normal() * np.eye(k)) for e in edges], 0)
    mplp = Mplp(model_of(case))
    gen = torch.Generator(device="cuda").manual_seed(2)
    unaries = torch.randn((args.rows, mplp.n_unary), dtype=torch.float64, device="cuda", generator=gen)
    run = lambda: mplp.map_query_batch(unaries, args.iters, 0.0, 0.0)
    ms = event_ms(run, args.steps, args.warmup)
    got = run()
    assert bool((got.n_iter == args.iters).all()) and bool((got.primal <= got.dual_lp + 1e-9).all())
    row0 = unaries[0].cpu().numpy()
    t0 = time.perf_counter()
    ref = M.run(M.with_unary(case, row0), args.iters)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(got.codes[0].cpu().numpy(), ref["codes"]) and float(got.dual_lp[0]) == float(ref["dual_lp"])
    out = {"workload": "potts_batch", "side": n, "states": k, "rows": args.rows, "iters": args.iters,
           "clusters": len(edges), "levels": mplp.plan.n_levels, "ms_median": ms[0], "ms_min": ms[1],
           "cluster_updates_per_s": args.rows * args.iters * len(edges) / (ms[0] * 1e-3),
           "host_restatement_ms_per_instance": host_ms, "device_ms_per_instance": ms[0] / args.rows,
           "integrality_gap_median": float(got.integrality_gap.median())}
    out.update(occupancy(mplp.plan.info))
    return out


def tighten_query(args):
    from pgmpy_amd.inference import Mplp

    rng = np.random.default_rng(4)
    at = lambda r, c: r * 4 + c
    edges = M.grid_edges(4, 4) + [(at(r, c), at(r + 1, c + 1)) for r in range(3) for c in range(3)]
    case = ([2] * 16, [rng.normal(size=2) * 0.1 for _ in range(16)],
            [(e, np.array([[-1.0, 1.0], [1.0, -1.0]]) * rng.choice([-1.0, 1.0])) for e in edges], 0)
    model = model_of(case)
    Mplp(model).map_query(tighten_triplet=False)  # the first launch pays for the upload and the module
    first = Mplp(model)
    t0 = time.perf_counter()
    first.map_query(tighten_triplet=False)
    pair_ms, pair_gap = (time.perf_counter() - t0) * 1e3, first.get_integrality_gap()
    t0 = time.perf_counter()
    ref = M.run(case, 1000, 0.0002, 0.0002)
    host_ms = (time.perf_counter() - t0) * 1e3
    mplp = Mplp(model)
    t0 = time.perf_counter()
    found = mplp.map_query()
    ms = (time.perf_counter() - t0) * 1e3
    x = [found[f"x{v:03d}"] for v in range(16)]
    value = sum(case[1][v][x[v]] for v in range(16)) + sum(t[tuple(x[v] for v in vs)] for vs, t in case[2])
    return {"workload": "tighten_query", "nodes": 16, "clusters": len(edges), "triangles": len(mplp.find_triangles()),
            "triplets_added": len(mplp._triplets), "map_query_ms": ms, "pairwise_run_ms": pair_ms,
            "host_restatement_pairwise_ms": host_ms, "pairwise_iterations": ref["n_iter"],
            "pairwise_integrality_gap": pair_gap, "integrality_gap": mplp.get_integrality_gap(),
            "value": float(value), "brute_force": float(M.brute_force(case))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16)
    ap.add_argument("--states", type=int, default=4)
    ap.add_argument("--rows", type=int, default=10_000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native

    assert torch.cuda.is_available(), "mplp_bench needs a HIP device"
    _native.lib()
    out = []
    for work in (potts_batch, tighten_query):
        out.append(work(args))
        out[-1].update(steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
                       date=datetime.date.today().isoformat(), kind="measured")
        print(json.dumps(out[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f)
            f.write("\n")


if __name__ == "__main__":
    main()
