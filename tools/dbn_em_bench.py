#!/usr/bin/env python3
"""Time the E-step of the dynamic-network EM on resident codes, beside the smoother on the same codes.

    python tools/dbn_em_bench.py [--rows 100000] [--T 100] [--steps 5] [--warmup 2] [--out profiles/dbn_em_bench.json]

The two models of tools/dbn_bench.py (hmm: 8 hidden states under 8 observed nodes; factorial: six hidden binary
chains under one observed node), simulated into a resident uint8 code matrix [(T + 1) n, rows]; the hidden nodes'
cells are then set to 255, which is the learning workload: the chain is not in the data.  Recorded per model (HIP
events on the current stream, `warmup` untimed runs, then the median and the minimum of `steps`):
  smooth_ms          DBNInference.smooth_codes of the hidden nodes: the kernel the E-step extends
  estep_tile_ms      DbnPlan.estep on the path pgm_dbn_estep_info chooses (the LDS tile when it fits)
  estep_direct_ms    DbnPlan.estep(direct=True): every add a global atomic; null (not measured) when the run on
                     rows / 100 sequences says the full size would pass --direct-limit seconds
  estep_over_smooth, tile_over_direct   the ratios of the medians of this run
  small_*            both paths on the first rows / 100 sequences, and their ratio at that size
  iteration_ms       one iteration of fit_codes (E-step, two pgm_fit_finish, the convergence test and its scalar):
                     (wall clock of max_iter = 4 - wall clock of max_iter = 1) / 3, atol = 0
  adds_per_sequence_slice   J (n_cur + S n_prev): the table adds a slice of a sequence with every hidden cell
                     missing makes at t >= 1
A path that finds no device fails.  Prints one JSON line per model; --out also writes them to a file.
"""
import argparse
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.dbn_bench import MODELS  # noqa: E402
from tools.fit_bench import event_ms  # noqa: E402


def run(name, args):
    import torch

    from pgmpy_amd import _native as N
    from pgmpy_amd.inference import DBNInference

    model, hidden = MODELS[name]()
    inf = DBNInference(model)
    observed = [v for v in inf.names if v not in hidden]
    B, T1 = args.rows, args.T + 1
    codes = model.simulate_codes(B, T1, seed=11).clone()
    for v, node in enumerate(inf.names):
        if node in hidden:
            codes[v::len(inf.names)] = 255
    plan = inf.plan(observed, [])
    info, einfo = plan.info, plan.estep_info()
    values0, values1 = inf._tables()
    tables = [torch.zeros_like(values0), torch.zeros_like(values1)]

    def estep(direct, n_rows=None):
        return plan.estep(codes, values0, values1, tables[0], tables[1], n_rows=n_rows, direct=direct)

    smo = event_ms(lambda: inf.smooth_codes(codes, observed, hidden), args.steps, args.warmup)
    print(f"# {name}: smooth {smo[0]:.2f} ms", flush=True)
    tile = event_ms(lambda: estep(False), args.steps, args.warmup)
    print(f"# {name}: estep, chosen path {tile[0]:.2f} ms", flush=True)
    # both paths on the first rows / 100 sequences; the direct path at full size only when that run says it ends
    # within --direct-limit seconds (every add of every sequence lands on the same few hundred addresses)
    small = max(B // 100, 1)
    tile_small = event_ms(lambda: estep(False, small), max(args.steps // 2, 1), 1)
    direct_small = event_ms(lambda: estep(True, small), max(args.steps // 2, 1), 1)
    print(f"# {name}: {small} rows: chosen path {tile_small[0]:.2f} ms, direct {direct_small[0]:.2f} ms", flush=True)
    direct = None
    if direct_small[0] * 1e-3 * B / small <= args.direct_limit:
        direct = event_ms(lambda: estep(True), max(args.steps // 2, 1), 1)
        print(f"# {name}: estep, direct {direct[0]:.2f} ms", flush=True)
    # the counts of one E-step: every family's table holds one unit per sequence and slice
    for t in tables:
        t.zero_()
    _, _, loglik, flags = estep(False)
    assert bool(torch.isfinite(loglik).all()) and not bool(flags.any())
    assert abs(float(tables[0].sum()) - B * info.n) <= 1e-6 * B and abs(float(tables[1].sum()) - B * args.T * info.n) <= 1e-6 * B * args.T
    wall = {}
    for iters in (1, 4, 1, 4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.copy().fit_codes(codes, T1, observed=observed, max_iter=iters, atol=0)
        torch.cuda.synchronize()
        wall[iters] = time.perf_counter() - t0  # the second round of each stands: the first pays the warm-up
    return {"model": name, "rows": B, "T": args.T, "n": int(info.n), "J": int(info.n_configs), "S": int(info.n_interface),
            "n_prev_families": int(info.n_prev_families), "n_cur_families": int(info.n_cur_families),
            "seq_per_wave": int(info.seq_per_wave), "table_entries": int(info.values0 + info.values1),
            "path": "tile" if einfo.path == N.DBN_ESTEP_TILE else "direct", "estep_lds_bytes": int(einfo.lds_bytes),
            "smooth_lds_bytes": int(info.lds_bytes), "max_blocks": int(einfo.max_blocks),
            "adds_per_sequence_slice": int(info.n_configs * (info.n_cur_families + info.n_interface * info.n_prev_families)),
            "launches": max(1, -(-plan.scratch_bytes(B, T1) // (1 << 30))),
            "smooth_ms_median": smo[0], "smooth_ms_min": smo[1], "estep_tile_ms_median": tile[0], "estep_tile_ms_min": tile[1],
            "estep_direct_ms_median": direct and direct[0], "estep_direct_ms_min": direct and direct[1],
            "estep_over_smooth": tile[0] / smo[0], "tile_over_direct": direct and tile[0] / direct[0],
            "small_rows": small, "small_tile_ms_median": tile_small[0], "small_direct_ms_median": direct_small[0],
            "small_tile_over_direct": tile_small[0] / direct_small[0],
            "iteration_ms": (wall[4] - wall[1]) / 3 * 1e3, "fit_codes_1_iteration_s": wall[1], "fit_codes_4_iterations_s": wall[4],
            "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
            "date": datetime.date.today().isoformat(), "kind": "measured"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--models", nargs="+", default=list(MODELS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--direct-limit", type=float, default=10.0, help="seconds the full-size direct run may be expected to take")
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native

    assert torch.cuda.is_available(), "dbn_em_bench needs a HIP device"
    _native.lib()
    out = []
    for name in args.models:
        out.append(run(name, args))
        print(json.dumps(out[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f)
            f.write("\n")


if __name__ == "__main__":
    main()
