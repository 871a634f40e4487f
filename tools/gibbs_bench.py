#!/usr/bin/env python3
"""Time Gibbs sampling: alarm (37 nodes) with resident chains from the forward start, and munin for time only.

    python tools/gibbs_bench.py [--chains 1000000] [--sweeps 10] [--steps 20] [--warmup 3] [--out FILE.json]

Per model, after a warm-up, every timed step copies the forward-sampled start state into the resident code
matrix and runs ONE pgm_gibbs_sweep launch of `sweeps` sweeps over all chains (HIP events around the call;
the call also reads its flags back).  Reported:

  updates/s   chains x sweeps x variables over the launch time
  bytes       the code bytes a variable update moves under the model of the path: on the LDS path a launch
              reads and writes every code once (2 x n_cols bytes per chain, whatever the number of sweeps); on
              the global path an update writes its code and reads one code per other column of every incident
              factor.  The value tables (alarm: 752 entries, 6 KB) stay cache-resident and are not counted.
              Given as GB/s and as a fraction of the 8 TB/s HBM peak.
  global      alarm again with the state forced into the code matrix: the tool appends clamped one-factor
              binary columns until n_cols x block exceeds the LDS budget plan_info reports (they are never
              drawn; the launch reads each once to validate it).  The codes of the alarm columns are the same.
  host        the numpy restatement (tests/gibbs_cases.py), one core, same box, on --host-chains chains.

The device codes of the last step are checked against the restatement on the first 2,048 chains.  Prints one
JSON line per run; --out also writes them to a file.
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
CHECK_CHAINS = 2048


def timed_sweeps(plan, values, start, codes, n_sweeps, seed, clamp, steps, warmup):
    """Median, min, max ms of `steps` launches, each from the start state."""
    import torch

    ms = []
    for i in range(warmup + steps):
        codes[:start.shape[0]].copy_(start)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        plan.sweep(values, codes, n_sweeps, seed=seed, clamp=clamp)
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def byte_model(factors, n_cols, n_sweeps, lds):
    """Code bytes per variable update."""
    if lds:
        return 2.0 / n_sweeps
    reads = sum(len(cols) * (len(cols) - 1) for cols, _ in factors)
    return (n_cols + reads) / n_cols


def run(name, model, n, args, steps, warmup, force_global=False, check=True, host=False):
    import torch

    from pgmpy_amd.inference.batch import download
    from pgmpy_amd.sampling import BayesianModelSampling
    from pgmpy_amd.sampling._gibbs import LDS, PATH_NAMES, GibbsPlan
    from pgmpy_amd.sampling.gibbs import gibbs_compiled
    from tests import gibbs_cases as G
    from tests import sample_cases as S

    c = gibbs_compiled(model, True)
    values, factors, card = c.tables(), list(c.factors), list(c.card)
    start, _ = BayesianModelSampling(model).forward_sample_codes(n, seed=args.seed)
    n_model = len(card)
    clamp = None
    if force_global:
        info = c.plan.launch_info(n)
        pad = info.lds_budget // info.block + 1 - n_model
        assert pad > 0
        factors += [([n_model + i], [2]) for i in range(pad)]
        card += [2] * pad
        values = torch.cat([values, torch.full((2 * pad,), 0.5, dtype=torch.float64, device=values.device)])
        clamp = np.array([0] * n_model + [1] * pad, dtype=np.uint8)
    plan = GibbsPlan(factors, card) if force_global else c.plan
    info = plan.launch_info(n)
    assert (info.path != LDS) or not force_global
    codes = torch.zeros((len(card), n), dtype=torch.uint8, device=values.device)
    ms, lo, hi = timed_sweeps(plan, values, start, codes, args.sweeps, args.seed, clamp, steps, warmup)
    if check:
        got = download(codes[:n_model, :CHECK_CHAINS].contiguous())
        nodes, fams, tables, rcard = G.bn_factors(model)
        first = S.sample_ref(fams, tables, min(n, CHECK_CHAINS), seed=args.seed, n_cols=len(nodes))[0]
        want = G.gibbs_ref(fams, tables, rcard, first, args.sweeps, seed=args.seed)[0]
        assert nodes == c.nodes and np.array_equal(got, want), "device codes differ from the numpy restatement"
    updates = n * args.sweeps * n_model
    bpu = byte_model(factors[:len(c.factors)], n_model, args.sweeps, info.path == LDS)
    gbs = updates * bpu / (ms * 1e-3) / 1e9
    res = {
        "model": name, "chains": n, "sweeps": args.sweeps, "variables": n_model, "factors": len(c.factors),
        "table_entries": int(c.plan.total_entries), "max_degree": int(info.max_degree), "max_card": int(info.max_card),
        "path": PATH_NAMES[info.path], "forced_global": bool(force_global), "padded_columns": len(card) - n_model,
        "block": int(info.block), "lds_bytes": int(info.lds_bytes), "lds_budget": int(info.lds_budget),
        "sweep_ms_median": ms, "sweep_ms_min": lo, "sweep_ms_max": hi, "updates": updates,
        "updates_per_s": updates / (ms * 1e-3), "ms_per_sweep": ms / args.sweeps,
        "model_code_bytes_per_update": bpu, "model_GBs": gbs, "frac_hbm_peak": gbs / HBM_PEAK_GBS,
        "hbm_peak_GBs": HBM_PEAK_GBS, "checked_against_restatement": bool(check),
        "steps": steps, "warmup": warmup, "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
        "kind": "measured",
    }
    if host:
        nodes, fams, tables, rcard = G.bn_factors(model)
        first = S.sample_ref(fams, tables, args.host_chains, seed=args.seed, n_cols=len(nodes))[0]
        t0 = time.perf_counter()
        G.gibbs_ref(fams, tables, rcard, first, args.sweeps, seed=args.seed)
        host_s = time.perf_counter() - t0
        host_rate = args.host_chains * args.sweeps * n_model / host_s
        res.update({"host_numpy_chains": args.host_chains, "host_numpy_s_one_core": host_s,
                    "host_numpy_updates_per_s": host_rate, "speedup_vs_host_numpy": res["updates_per_s"] / host_rate})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--chains", type=int, default=1_000_000)
    ap.add_argument("--munin-chains", type=int, default=65_536)
    ap.add_argument("--host-chains", type=int, default=65_536)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--munin-steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-munin", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native
    from pgmpy_amd.utils import get_example_model

    assert torch.cuda.is_available(), "gibbs_bench needs a HIP device"
    _native.lib()
    alarm = get_example_model("alarm")
    lines = []

    def emit(res):
        print(json.dumps(res), flush=True)
        lines.append(res)

    emit(run("alarm", alarm, args.chains, args, args.steps, args.warmup, host=True))
    emit(run("alarm", alarm, args.chains, args, args.steps, args.warmup, force_global=True))
    if not args.no_munin:
        emit(run("munin", get_example_model("munin"), args.munin_chains, args, args.munin_steps, 1, check=False))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
