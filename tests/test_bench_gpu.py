"""bench.py's plain line and --dump-outputs on the device: one small run of the command itself.

The run is the C3 template at 1,537 rows (odd: the one-row-per-thread kernel takes the tail), one
resident batch on one queue, so the dumped batch is the seeded sample itself and the oracle can be
asked about its rows.
"""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 1537


def test_plain_line_and_dumped_marginals(gpu, tmp_path):
    """A plain run times exactly --steps steps, prints the headline fields and none of the --full
    parts, and --dump-outputs writes the last step's [17, rows] fp64 marginals (variables in sorted
    order): rows 0, 1 and the last against the oracle at BASELINE.json's 1e-6 relative."""
    from oracle import ve as OVE
    from oracle.network import load_network
    from pgmpy_amd.utils import get_example_model
    from pgmpy_amd.utils.sampling import forward_sample_codes

    d = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--rows", str(ROWS), "--batches", "1", "--queues", "1", "--dump-outputs", str(d)]
    r = subprocess.run(cmd, cwd=ROOT, timeout=240, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-3000:]
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["full"] is False
    assert res["unit"] == "queries/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(ROWS / (res["ms_per_step"] * 1e-3), rel=1e-9)
    assert len(res["roofline"]["dispatch_times"]["dispatches"]) == 3  # the timed steps, no more
    for k in ("parity", "cpu_baseline", "cpu_baseline_allcore", "api_e2e", "c5", "c1", "c2", "c4"):
        assert k not in res, k
    assert sorted(os.listdir(d)) == ["marginals.npy"]
    marg = np.load(d / "marginals.npy")
    assert marg.dtype == np.float64

    m = get_example_model("munin")
    net = load_network("munin")
    missing = sorted(random.Random(0).sample(sorted(m.nodes()), 3))
    assert marg.shape == (sum(len(net.states[v]) for v in missing), ROWS)
    codes, nodes = forward_sample_codes(m, ROWS, seed=42)
    pos = {v: i for i, v in enumerate(nodes)}
    for row in (0, 1, ROWS - 1):
        ev = {v: net.states[v][codes[pos[v], row]] for v in nodes if v not in missing}
        mg = OVE.query(net, missing, ev, joint_out=False)
        np.testing.assert_allclose(marg[:, row], np.concatenate([mg[v] for v in missing]), rtol=1e-6, atol=1e-12)
