#!/usr/bin/env python3
"""Time the dynamic-network smoother on resident codes: simulate_codes -> smooth_codes, nothing leaving HBM.

    python tools/dbn_bench.py [--rows 100000] [--T 100] [--steps 5] [--warmup 2] [--out profiles/dbn_bench.json]

Two models, each simulated into a resident uint8 code matrix [(T + 1) n, rows] that the smoother then reads:
  hmm        one hidden node of 8 states, 8 binary observed children of it (clamped): J = S = 8, eight sequences
             share a wave
  factorial  6 hidden binary chains and one observed child of all six (clamped): J = S = 64, one sequence per wave,
             six transition families evaluated per (i, x')
Recorded per model (HIP events on the current stream, `warmup` untimed runs, then the median and the minimum of
`steps`):
  simulate_ms     DynamicBayesianNetwork.simulate_codes (the unrolled network's sampling launch)
  loglik_ms       DBNInference.log_likelihood_codes: the forward pass alone, no marginals
  filter_ms       filter_codes of the hidden nodes
  smooth_ms       smooth_codes of the hidden nodes: forward, then backward with alpha rebuilt from the message
  slice_updates_per_s   rows x (T + 1) / smooth time (median)
  end_to_end_s    wall clock of simulate_codes -> smooth_codes -> synchronize, three runs
  kernel_share    smooth_ms / the fastest end-to-end run
A path that finds no device fails.  Prints one JSON line per model; --out also writes them to a file.
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


def random_cpd(rng, var, card, evidence, evidence_card):
    from pgmpy_amd.factors.discrete import TabularCPD

    t = rng.random((card, int(np.prod(evidence_card)) if evidence else 1)) + 0.05
    return TabularCPD(var, card, t / t.sum(axis=0), evidence=evidence or None, evidence_card=evidence_card or None)


def build(hidden, observed, seed):
    """hidden: {name: card}, each a chain name_t -> name_t+1; observed: {name: card}, each a child of every hidden node."""
    from pgmpy_amd.models import DynamicBayesianNetwork

    rng = np.random.default_rng(seed)
    m = DynamicBayesianNetwork()
    m.add_nodes_from(list(hidden) + list(observed))
    m.add_edges_from([((h, 0), (o, 0)) for h in hidden for o in observed] + [((h, 0), (h, 1)) for h in hidden])
    for t in (0, 1):
        for h, k in hidden.items():
            m.add_cpds(random_cpd(rng, (h, t), k, [(h, 0)] if t else [], [k] if t else []))
        for o, k in observed.items():
            m.add_cpds(random_cpd(rng, (o, t), k, [(h, t) for h in hidden], list(hidden.values())))
    m.check_model()
    return m


MODELS = {
    "hmm": lambda: (build({"H": 8}, {f"O{i}": 2 for i in range(8)}, 1), ["H"]),
    "factorial": lambda: (build({f"H{i}": 2 for i in range(6)}, {"O": 3}, 2), [f"H{i}" for i in range(6)]),
}


def run(name, args):
    import torch

    from pgmpy_amd.inference import DBNInference

    model, hidden = MODELS[name]()
    inf = DBNInference(model)
    observed = [v for v in inf.names if v not in hidden]
    B, T1 = args.rows, args.T + 1
    codes = model.simulate_codes(B, T1, seed=11)
    info = inf.plan(observed, hidden).info
    sim = event_ms(lambda: model.simulate_codes(B, T1, seed=11), args.steps, args.warmup)
    ll = event_ms(lambda: inf.log_likelihood_codes(codes, observed), args.steps, args.warmup)
    fil = event_ms(lambda: inf.filter_codes(codes, observed, hidden), args.steps, args.warmup)
    smo = event_ms(lambda: inf.smooth_codes(codes, observed, hidden), args.steps, args.warmup)
    wall = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = model.simulate_codes(B, T1, seed=11)
        s, loglik, flags = inf.smooth_codes(c, observed, hidden)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    assert bool(torch.isfinite(loglik).all()) and not bool(flags.any())
    assert bool(((s.reshape(B, T1, len(hidden), -1).sum(dim=3) - 1).abs() < 1e-12).all())
    scratch = inf.plan(observed, hidden).scratch_bytes(B, T1)
    return {"model": name, "rows": B, "T": args.T, "n": int(info.n), "J": int(info.n_configs), "S": int(info.n_interface),
            "seq_per_wave": int(info.seq_per_wave), "lds_bytes": int(info.lds_bytes), "scratch_bytes": int(scratch),
            "smooth_launches": max(1, -(-scratch // (1 << 30))),
            "simulate_ms_median": sim[0], "simulate_ms_min": sim[1], "loglik_ms_median": ll[0], "loglik_ms_min": ll[1],
            "filter_ms_median": fil[0], "filter_ms_min": fil[1], "smooth_ms_median": smo[0], "smooth_ms_min": smo[1],
            "slice_updates_per_s": B * T1 / (smo[0] * 1e-3), "end_to_end_s": wall,
            "kernel_share": smo[0] * 1e-3 / min(wall), "steps": args.steps, "warmup": args.warmup,
            "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "kind": "measured"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--models", nargs="+", default=list(MODELS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native

    assert torch.cuda.is_available(), "dbn_bench needs a HIP device"
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
