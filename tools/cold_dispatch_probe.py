"""What a direct dispatch of the C3 row kernel costs when its bound launch was not the one just run.

    python tools/cold_dispatch_probe.py [--root TREE] [--out FILE.json] [--repeats 5]

bench.py's C3 window steps round robin over 96 resident batches, each its own bound launch
(PatternPlan.bind(...).direct(queue)); every committed floor measurement repeats ONE bound launch.  This
probe times both on the same buffers, through the queue timer only (timer_start / timer_stop_ticks /
dispatch_times), never through bench.py:

  a  one queue,   one bound launch repeated
  b  one queue,   96 bound launches round robin
  c  four queues, one bound launch each, repeated
  d  four queues, 96 bound launches round robin (launch i on queue i % 4), at 20, 50 and 400 dispatches

and reports, per case, the GPU span per dispatch (first start to last end, over the dispatches) and the
mean of the dispatches' own durations (end - start), each as the median and the range over --repeats
windows.  b - a and d - c are what rotating over distinct bound launches costs per dispatch.

The setup is bench.py's: the munin predict_probability template (3 missing variables, seed 0), 100,000
rows, 96 batches (batch i = a seeded row permutation of the sampled rows in its own evidence columns, its
own output; working set > the 256 MiB Infinity Cache).  --root names the tree whose pgmpy_amd is imported
(default: the tree this file is in), so one GPU visit can probe two builds of the library in turn.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--batches", type=int, default=96)
    ap.add_argument("--queues", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    import numpy as np
    import torch

    import pgmpy_amd
    from pgmpy_amd.inference.batch import upload_codes
    from pgmpy_amd.inference.plan import DirectQueue, PatternPlan
    from pgmpy_amd.utils import get_example_model
    from pgmpy_amd.utils.sampling import forward_sample_codes

    assert os.path.abspath(pgmpy_amd.__file__).startswith(os.path.abspath(args.root)), pgmpy_amd.__file__
    torch.cuda.set_device(0)
    rows, nb, nq = args.rows, args.batches, args.queues
    model = get_example_model("munin")
    missing = set(random.Random(0).sample(sorted(model.nodes()), 3))
    variables = list(missing)
    codes_all, nodes = forward_sample_codes(model, rows, seed=42)
    observed = [v for v in nodes if v not in missing]
    pos = {v: i for i, v in enumerate(nodes)}
    codes_one = np.ascontiguousarray(codes_all[[pos[v] for v in observed]])
    col_of = {v: i for i, v in enumerate(observed)}
    plan = PatternPlan(model, variables, observed, col_of)
    assert plan.kind == "fused", plan.describe()
    prng = np.random.default_rng(1000)
    used = sorted({col_of[v] for v in plan.ev_used})
    codes_ev = np.empty((codes_one.shape[0], rows * nb), dtype=np.uint8)
    for i in range(nb):
        codes_ev[:, i * rows:(i + 1) * rows] = codes_one
        if i:
            codes_ev[used, i * rows:(i + 1) * rows] = codes_one[used][:, prng.permutation(rows)]
    d_codes = upload_codes(codes_ev)
    del codes_ev
    outs = [plan.alloc_outputs(rows, marginals=True) for _ in range(nb)]
    err = torch.zeros(1, dtype=torch.int32, device=d_codes.device)
    bounds = [plan.bind(d_codes, rows * nb, i * rows, rows, outs[i], err=err) for i in range(nb)]
    qs = [DirectQueue.default()] + [DirectQueue() for _ in range(nq - 1)]
    t0 = time.perf_counter()
    rs = [b.direct(qs[i % nq]) for i, b in enumerate(bounds)]  # as bench.py's Launcher binds them
    bind_s = time.perf_counter() - t0
    torch.cuda.synchronize()

    def window(seq, used_qs, n):
        """n timed dispatches of seq (round robin) after a warm-up pass over all of seq and one untimed
        dispatch per queue that takes the system-scope acquire (bench.py's window, without the release)."""
        for r in seq:
            r.run()
        for q in used_qs:
            q.sync()
        for j in range(len(used_qs)):
            seq[j % len(seq)].run()
        for q in used_qs:
            q.wait()
        for q in used_qs:
            q.timer_start()
        for j in range(n):
            seq[j % len(seq)].run()
        for q in used_qs:
            q.wait()
        lo, hi, freq, durs = None, None, 1, []
        for q in used_qs:
            a, b, f = q.timer_stop_ticks()
            if b > a:
                lo = a if lo is None else min(lo, a)
                hi = b if hi is None else max(hi, b)
                freq = f
            durs += [e - s for s, e in q.dispatch_times() if e > s]
        for q in used_qs:
            q.sync()
        us = 1e6 / freq
        return (hi - lo) * us / n, (sum(durs) / len(durs)) * us, len(durs)

    def case(name, seq, used_qs, n):
        spans, means, counted = [], [], 0
        for _ in range(args.repeats):
            s, m, counted = window(seq, used_qs, n)
            spans.append(s)
            means.append(m)
        return {"case": name, "queues": len(used_qs), "bound_launches": len(seq), "dispatches": n,
                "dispatches_with_timestamps": counted,
                "span_us_per_dispatch": {"median": statistics.median(spans), "min": min(spans), "max": max(spans)},
                "dispatch_us_mean": {"median": statistics.median(means), "min": min(means), "max": max(means)}}

    cases = []
    one_q = [b.direct(qs[0]) for b in bounds]  # case b: all 96 on one queue
    for n in (20, 50, 400):
        cases.append(case("a", rs[:1], qs[:1], n))
        cases.append(case("b", one_q, qs[:1], n))
        cases.append(case("c", rs[:nq], qs, n))
        cases.append(case("d", rs, qs, n))
    assert int(err.item()) == 0
    by = {(c["case"], c["dispatches"]): c for c in cases}
    cold = {}
    for n in (20, 50, 400):
        for hot, rot in (("a", "b"), ("c", "d")):
            for k in ("span_us_per_dispatch", "dispatch_us_mean"):
                cold[f"{rot}-{hot}@{n}:{k}"] = by[(rot, n)][k]["median"] - by[(hot, n)][k]["median"]
    info = None
    if hasattr(rs[0], "info"):
        infos = [r.info() for r in rs]
        info = {"distinct_kernel_objects": len({i[0] for i in infos}), "sharers": infos[0][2],
                "kernarg_span_bytes": max(i[1] for i in infos) - min(i[1] for i in infos) + 256}
    res = {"probe": "cold_dispatch", "label": args.label, "rows": rows, "batches": nb, "queues": nq,
           "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "bind_seconds_for_all_bound_launches": bind_s, "bound_info": info,
           "working_set_bytes": plan.algorithmic_bytes_per_row(marginals=True) * rows * nb,
           "cases": cases, "cold_minus_hot_us": cold}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
