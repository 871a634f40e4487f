"""Worker for tests/test_plan_dev_gpu.py::test_destroyed_plans_leave_nothing_behind (-m gpu).

Destroys a FitPlan that never launched and one that ran only pgm_fit_score (the base and one stage on the
device, the other stage never built), prints torch.cuda.memory_allocated() before and after as JSON, and
exits: the test checks the figures and the exit status.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import torch

    from pgmpy_amd import _native as N
    from pgmpy_amd import engine as E
    from pgmpy_amd.estimators._fit import FitPlan

    N.lib()
    families = [([0], [2]), ([1, 0], [3, 2])]
    counts = E.to_device_raw(np.array([2, 3, 1, 0, 1, 1, 0, 2], dtype=np.int64))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    never = FitPlan(families)
    del never
    plan = FitPlan(families)
    scores = plan.score(counts, N.SCORE_LL).cpu().tolist()
    del plan
    torch.cuda.synchronize()
    print(json.dumps({"before": before, "after": torch.cuda.memory_allocated(), "scores": scores}))


if __name__ == "__main__":
    main()
