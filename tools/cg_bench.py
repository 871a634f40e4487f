#!/usr/bin/env python3
"""Time the conditional-Gaussian scores on resident mixed data: alarm's 37 discrete columns sampled on the device
plus 8 continuous ones (and five synthetic four-state columns for the single families).

    python tools/cg_bench.py [--rows 1000000] [--steps 10] [--warmup 3] [--host-families 12] [--out profiles/cg_bench.json]

Recorded:
  step1     the 2,025 families of a first hill-climb step at max_indegree 1: moments_ms and score_ms (HIP events
            around pgm_cg_moments / pgm_cg_score on a plan made before), batch_s (BICCondGauss.local_scores end
            to end: plan, launches, download; wall clock, three runs), and the host baseline: the same definition
            in numpy on the downloaded data over the first --host-families families (host_s, host_s_per_family;
            host_full_s_estimate = per family x all families, an estimate and marked so)
  single    three single families, Q = 1 m = 7, Q = 16 m = 3 and Q mp = 4096 (Q = 1024, m = 3): moments_ms,
            score_ms, host_s; for Q = 1 also gram_ms (pgm_lg_gram over the same 7 columns, the same moments) and
            the fraction of copy_gbps, a device-to-device copy's rate in the same run, that its value bytes / time reach
A path that finds no device fails.  Prints one JSON line; --out also writes it to a file.
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

from tools.fit_bench import event_ms  # noqa: E402

LOG2PI, RCOND = float(np.log(2 * np.pi)), 1e-11


def host_density(n, s, G):
    """L(g; cols) from a group's count, sums and cross products (fp64)."""
    k = len(s)
    if n == 0 or k == 0:
        return 0.0
    sc = G - np.outer(s, s) / n
    if n == 1 or n < k:
        return -0.5 * n * k * LOG2PI - 0.5 * np.trace(sc)
    d = np.clip(np.diag(sc), 0.0, None)
    inv = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    R, r, logdet = sc * np.outer(inv, inv), 0, 0.0
    for j in range(k):
        p = R[j, j]
        if p > RCOND:
            r += 1
            logdet += np.log(d[j] * p / (n - 1))
            R[j + 1:, j + 1:] -= np.outer(R[j + 1:, j], R[j + 1:, j]) / p
    return -0.5 * n * (r * LOG2PI + logdet) - 0.5 * (n - 1) * r


def host_score(codes, X, fam):
    """The log-likelihood of one family from the downloaded codes and values."""
    dcols, cards, ccols, disc = fam
    cfg, Q = np.zeros(codes.shape[1], dtype=np.int64), 1
    for c, k in zip(dcols, cards):
        cfg, Q = cfg * k + codes[c], Q * k
    Z = np.vstack([np.ones(codes.shape[1])] + [X[c] - X[c].mean() for c in ccols])
    M = np.array([[np.bincount(cfg, weights=Z[i] * Z[j], minlength=Q) for j in range(len(Z))] for i in range(len(Z))])
    M = M.transpose(2, 0, 1)
    if not disc:
        return sum(host_density(m[0, 0], m[1:, 0], m[1:, 1:]) - host_density(m[0, 0], m[1:-1, 0], m[1:-1, 1:-1]) for m in M)
    Mh = M.reshape(cards[0], -1, len(Z), len(Z))
    n, ll = float(codes.shape[1]), 0.0
    for sign, groups in ((1.0, M), (-1.0, Mh.sum(axis=0))):
        for m in groups:
            if m[0, 0] > 0:
                ll += sign * (host_density(m[0, 0], m[1:, 0], m[1:, 1:]) + m[0, 0] * np.log(m[0, 0] / n))
    return ll


def timings(plan, codes, X, shift, n, args):
    mom = plan.moments(codes, X, shift, n)
    return {"moments_ms": event_ms(lambda: plan.moments(codes, X, shift, n), args.steps, args.warmup),
            "score_ms": event_ms(lambda: plan.score(mom), args.steps, args.warmup),
            "slices_passes": plan.moments_info(n, X.data_ptr(), int(X.shape[1]))[1:3]}


def run(args):
    import torch

    from pgmpy_amd.estimators import BICCondGauss
    from pgmpy_amd.estimators._cg import CgPlan
    from pgmpy_amd.models._lg import GramPlan
    from pgmpy_amd.sampling import BayesianModelSampling
    from pgmpy_amd.utils import get_example_model

    n = args.rows
    model = get_example_model("alarm")
    alarm, nodes = BayesianModelSampling(model).forward_sample_codes(n, seed=args.seed)[:2]
    gen = torch.Generator(device="cuda").manual_seed(args.seed)
    extra = torch.randint(0, 4, (5, n), dtype=torch.uint8, device="cuda", generator=gen)
    codes = torch.cat([alarm, extra]).contiguous()
    cards = [int(model.get_cardinality(v)) for v in nodes] + [4] * 5
    X = torch.randn((8, n), dtype=torch.float64, device="cuda", generator=gen)
    for j in range(8):  # group means of order 1 and a chain of coefficients of order 1
        X[j] += torch.cos(1.0 + j + codes[j].to(torch.float64)) + (0.7 * X[j - 1] if j else 0.0)
    values = [f"c{j}" for j in range(8)]
    scorer = BICCondGauss.from_columns(codes, nodes, cards[:37], X, values)
    names = list(nodes) + values
    fams = [(v, []) for v in names] + [(v, [u]) for v in names for u in names if u != v]
    res = {"rows": n, "families": len(fams)}

    cg = [scorer.family(v, ps)[0] for v, ps in fams]
    _, _, shift, _ = scorer.resident()
    step = timings(CgPlan(cg), codes, X, shift, n, args)
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scorer.local_scores(fams)
        walls.append(time.perf_counter() - t0)
    hc, hX = codes.cpu().numpy(), X.cpu().numpy()
    timed = cg[len(names):len(names) + args.host_families]
    t0 = time.perf_counter()
    for fam in timed:
        host_score(hc, hX, fam)
    host_s = time.perf_counter() - t0
    step.update({"batch_s": walls, "host_families_timed": len(timed), "host_s": host_s, "host_s_per_family": host_s / max(len(timed), 1),
                 "host_full_s_estimate": host_s / max(len(timed), 1) * len(fams)})
    res["step1"] = step

    big = torch.empty(1 << 27, dtype=torch.float64, device="cuda")  # 1 GiB: read + written by a copy
    copy_ms = event_ms(lambda: big.clone(), args.steps, args.warmup)[0]
    res["copy_gbps"] = 2 * big.numel() * 8 / copy_ms / 1e6
    del big
    single = {}
    for name, fam in (("Q1_m7", ([], [], list(range(7)), False)), ("Q16_m3", ([37, 38], [4, 4], [0, 1, 2], False)),
                      ("Qmp4096", ([37, 38, 39, 40, 41], [4] * 5, [0, 1, 2], False))):
        t = timings(CgPlan([fam]), codes, X, shift, n, args)
        t0 = time.perf_counter()
        host_score(hc, hX, fam)
        t["host_s"] = time.perf_counter() - t0
        if name == "Q1_m7":
            gp = GramPlan(range(7))
            t["gram_ms"] = event_ms(lambda: gp.gram(X, shift, n, 0), args.steps, args.warmup)
            gbps = 7 * 8 * n / t["moments_ms"][0] / 1e6
            t.update({"value_gbps": gbps, "fraction_of_copy_rate": gbps / res["copy_gbps"]})
        single[name] = t
    res["single"] = single
    res.update({"steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
                "kind": "measured"})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-families", type=int, default=12)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pgmpy_amd import _native

    assert torch.cuda.is_available(), "cg_bench needs a HIP device"
    _native.lib()
    res = run(args)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()
