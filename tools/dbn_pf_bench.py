#!/usr/bin/env python3
"""Time the dynamic-network particle filter on resident codes: simulate_codes -> particle_filter_codes.

    python tools/dbn_pf_bench.py [--rows 100000] [--T 100] [--particles 1024] [--steps 3] [--warmup 1]
                                 [--out profiles/dbn_pf_bench.json]

Three models (tools/dbn_bench.py builds them), each simulated into a resident uint8 code matrix [(T + 1) n, rows]
whose hidden cells are then set to 255, so every hidden node of every particle is drawn:
  hmm          one hidden node of 8 states, 8 binary observed children; the exact filter is timed in the same run
  factorial    6 hidden binary chains and one observed child of all six (J = 64); the exact filter too
  factorial16  16 hidden binary chains and one observed child of all sixteen (J = 65,536): past the exact filter
Recorded per model (HIP events on the current stream, `warmup` untimed runs, then the median and the minimum of
`steps`): pf_ms, exact_filter_ms and pf_over_exact where the exact filter runs, particle_slice_updates_per_s =
rows x (T + 1) x particles / pf time (median), the median effective sample size over all sequences and slices, the
plan's block and LDS bytes.  A path that finds no device fails.  Prints one JSON line per model; --out also writes
them to a file.
"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.dbn_bench import build  # noqa: E402
from tools.fit_bench import event_ms  # noqa: E402

MODELS = {
    "hmm": lambda: (build({"H": 8}, {f"O{i}": 2 for i in range(8)}, 1), ["H"], True),
    "factorial": lambda: (build({f"H{i}": 2 for i in range(6)}, {"O": 3}, 2), [f"H{i}" for i in range(6)], True),
    "factorial16": lambda: (build({f"H{i:02d}": 2 for i in range(16)}, {"O": 3}, 3), [f"H{i:02d}" for i in range(16)], False),
}


def run(name, args):
    import torch

    from pgmpy_amd.inference import DBNInference

    model, hidden, exact = MODELS[name]()
    inf = DBNInference(model)
    observed = [v for v in inf.names if v not in hidden]
    B, T1, P, n = args.rows, args.T + 1, args.particles, len(inf.names)
    codes = model.simulate_codes(B, T1, seed=11)
    for v, node in enumerate(inf.names):
        if node in hidden:
            codes[v::n] = 255
    info = inf.pf_plan(hidden).info_at(P)
    pf = event_ms(lambda: inf.particle_filter_codes(codes, P, seed=3, variables=hidden), args.steps, args.warmup)
    filt, loglik, ess, flags = inf.particle_filter_codes(codes, P, seed=3, variables=hidden)
    assert bool(torch.isfinite(loglik).all()) and not bool(flags.any())
    assert bool(((filt.reshape(B, T1, len(hidden), -1).sum(dim=3) - 1).abs() < 1e-9).all())
    out = {"model": name, "rows": B, "T": args.T, "particles": P, "n": n, "n_interface": int(info.n_interface),
           "block": int(info.block), "lds_bytes": int(info.lds_bytes), "pf_ms_median": pf[0], "pf_ms_min": pf[1],
           "particle_slice_updates_per_s": B * T1 * P / (pf[0] * 1e-3), "ess_median": float(ess.median()),
           "ess_min": float(ess.min())}
    if exact:
        fil = event_ms(lambda: inf.filter_codes(codes, observed, hidden), args.steps, args.warmup)
        want, want_ll, _ = inf.filter_codes(codes, observed, hidden)
        out.update(exact_filter_ms_median=fil[0], exact_filter_ms_min=fil[1], pf_over_exact=pf[0] / fil[0],
                   filter_abs_error_max=float((filt - want).abs().max()), filter_abs_error_mean=float((filt - want).abs().mean()),
                   loglik_abs_error_mean=float((loglik - want_ll).abs().mean()))
    out.update(steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               date=datetime.date.today().isoformat(), kind="measured")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--particles", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--models", nargs="+", default=list(MODELS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native

    assert torch.cuda.is_available(), "dbn_pf_bench needs a HIP device"
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
