#!/usr/bin/env python3
"""Time the dynamic-network smoother on resident codes: simulate_codes -> smooth_codes, nothing leaving HBM.

    python tools/dbn_bench.py [--rows 100000] [--T 100] [--steps 5] [--warmup 2] [--out profiles/dbn_bench.json]
                              [--viterbi-out profiles/dbn_viterbi_bench.json]

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
Viterbi (DBNInference.viterbi_codes, k_dbn_viterbi), a second record per model with the same rows, T, warm-up and
median, written by --viterbi-out (profiles/dbn_viterbi_bench.json):
  observed_codes          filter_ms and viterbi_ms on the codes above, where the hidden nodes' cells are observed
                          too (an x' that contradicts its cell is skipped), and viterbi_over_filter from this run
  hidden_cells_missing    both again with the hidden nodes' cells set to 255, the decoding workload: every (i, x')
                          pair is evaluated
  backpointer_bytes, viterbi_launches   the uint16 backpointers of the batch and the launches the 1 GiB scratch
                          limit splits it into
A path that finds no device fails.  Prints one JSON line per model and record; --out and --viterbi-out also write
them to files.
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
    # Viterbi on the same codes as the columns above (every cell observed, the hidden nodes' too: an x' that
    # contradicts its cell is skipped), and both kernels again with the hidden nodes' cells set to "not observed",
    # which is the decoding workload: every (i, x') pair is evaluated
    from pgmpy_amd.inference._dbn import SCRATCH_BYTES

    vit = event_ms(lambda: inf.viterbi_codes(codes, observed), args.steps, args.warmup)
    masked = codes.clone()
    for v, node in enumerate(inf.names):
        if node in hidden:
            masked[v::len(inf.names)] = 255
    fil_h = event_ms(lambda: inf.filter_codes(masked, observed, hidden), args.steps, args.warmup)
    vit_h = event_ms(lambda: inf.viterbi_codes(masked, observed), args.steps, args.warmup)
    path, logmap, vflags = inf.viterbi_codes(masked, observed)
    assert bool(torch.isfinite(logmap).all()) and not bool(vflags.any()) and bool((path != 255).all())
    vit_scratch = inf.plan(observed, []).viterbi_scratch_bytes(B, T1)
    viterbi = {"model": name, "rows": B, "T": args.T, "J": int(info.n_configs), "S": int(info.n_interface),
               "seq_per_wave": int(info.seq_per_wave), "backpointer_bytes": int(vit_scratch),
               "viterbi_launches": -(-B // max(1, min(B, SCRATCH_BYTES // max(vit_scratch // B, 1)))),
               "observed_codes": {"filter_ms_median": fil[0], "filter_ms_min": fil[1], "viterbi_ms_median": vit[0],
                                  "viterbi_ms_min": vit[1], "viterbi_over_filter": vit[0] / fil[0]},
               "hidden_cells_missing": {"filter_ms_median": fil_h[0], "filter_ms_min": fil_h[1], "viterbi_ms_median": vit_h[0],
                                        "viterbi_ms_min": vit_h[1], "viterbi_over_filter": vit_h[0] / fil_h[0]},
               "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
               "date": datetime.date.today().isoformat(), "kind": "measured"}
    return {"viterbi": viterbi, "model": name, "rows": B, "T": args.T, "n": int(info.n), "J": int(info.n_configs), "S": int(info.n_interface),
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
    ap.add_argument("--viterbi-out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native

    assert torch.cuda.is_available(), "dbn_bench needs a HIP device"
    _native.lib()
    out, viterbi = [], []
    for name in args.models:
        out.append(run(name, args))
        viterbi.append(out[-1].pop("viterbi"))
        print(json.dumps(out[-1]), flush=True)
        print(json.dumps(viterbi[-1]), flush=True)
    for path, records in ((args.out, out), (args.viterbi_out, viterbi)):
        if path:
            with open(path, "w") as f:
                json.dump(records, f)
                f.write("\n")


if __name__ == "__main__":
    main()
