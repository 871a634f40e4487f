"""Direct (AQL) bound launches share one loaded code object per plan and device and take their kernarg
segments from one slab (pgmpy_amd/csrc/pgmdq.cpp, pgm_share.h; pgm_dq_bound_info).  Every output is
compared bit for bit with the HIP-launched bound run of the same rows."""
import gc
import random

import numpy as np
import pytest

from tests.goldens import fac_values, load_json

pytestmark = pytest.mark.gpu

SLOT, CHUNK = 256, 64 * 1024


def _template(net, total, seed, missing_seed):
    """The predict_probability template of `net` with 3 missing variables, and `total` sampled rows of the
    observed columns.  A missing set of its own per test keeps the test's code object its own: the
    registry is process wide, and another test's launches of the same code would be counted as sharers."""
    from pgmpy_amd.inference.plan import PatternPlan
    from pgmpy_amd.utils import get_example_model
    from pgmpy_amd.utils.sampling import forward_sample_codes

    m = get_example_model(net)
    missing = random.Random(missing_seed).sample(sorted(m.nodes()), 3)
    codes, nodes = forward_sample_codes(m, total, seed=seed)
    obs = [v for v in nodes if v not in missing]
    pos = {v: i for i, v in enumerate(nodes)}
    ev = np.ascontiguousarray(codes[[pos[v] for v in obs]])
    return PatternPlan(m, missing, obs, {v: i for i, v in enumerate(obs)}), ev


def _windows(plan, d, total, rows, step, n):
    """n bound launches over the row windows [i * step, i * step + rows) with their own outputs, and the
    HIP-launched reference of each."""
    import torch

    refs, outs, bounds = [], [], []
    for i in range(n):
        ref = plan.alloc_outputs(rows, marginals=True, map_=True)
        plan.bind(d, total, i * step, rows, ref).run()
        refs.append(ref)
        out = plan.alloc_outputs(rows, marginals=True, map_=True)
        outs.append(out)
        bounds.append(plan.bind(d, total, i * step, rows, out))
    torch.cuda.synchronize()
    return refs, outs, bounds


def _same(outs, refs):
    import torch

    return all(torch.equal(o["marg"], r["marg"]) and torch.equal(o["map"], r["map"]) for o, r in zip(outs, refs))


def _clear(outs):
    import torch

    for o in outs:
        o["marg"].zero_()
        o["map"].fill_(-1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows,step,kernel", [(1000, 1000, "pgm_rows_jit"), (50_002, 2000, "pgm_rows_jit2")])
def test_bounds_share_code_and_slab(gpu, rows, step, kernel):
    """Six bound launches of one munin-template plan (distinct row windows, distinct outputs) on two
    queues: one kernel object, six sharers, six distinct 256-byte-aligned kernarg slots within one 64 KiB
    slab, and after interleaved launches on both queues every output equals its reference.  1,000 rows
    run the one-row kernel; 50,002 rows the two-row kernel with a partial last block."""
    from pgmpy_amd.inference.batch import upload_codes
    from pgmpy_amd.inference.plan import DirectQueue

    gc.collect()
    n = 6
    total = rows + (n - 1) * step
    plan, ev = _template("munin", total, seed=31, missing_seed=101 + rows)
    d = upload_codes(ev)
    refs, outs, bounds = _windows(plan, d, total, rows, step, n)
    assert all(b.kernel()[0] == kernel for b in bounds)
    qs = [DirectQueue(), DirectQueue()]
    rs = [b.direct(qs[i % 2]) for i, b in enumerate(bounds)]
    infos = [r.info() for r in rs]
    assert len({ko for ko, _, _ in infos}) == 1 and infos[0][0] != 0
    assert all(sh == n for _, _, sh in infos)
    ka = [a for _, a, _ in infos]
    assert len(set(ka)) == n and all(a and a % SLOT == 0 for a in ka)
    assert max(ka) - min(ka) + SLOT <= CHUNK
    _clear(outs)
    for _ in range(3):
        for r in rs:  # alternates the queues
            r.run()
    for q in qs:
        q.sync()
    assert _same(outs, refs)


def test_shared_code_lifetime(gpu):
    """The first-created bound launch and then its queue are destroyed while the others keep launching:
    outputs stay right; a new bind reuses the executable and the freed kernarg slot; after the last
    bound launch is gone a fresh bind loads the code again and is correct."""
    from pgmpy_amd.inference.batch import upload_codes
    from pgmpy_amd.inference.plan import DirectQueue

    gc.collect()
    rows, n = 1000, 4
    total = rows * n
    plan, ev = _template("munin", total, seed=33, missing_seed=211)
    d = upload_codes(ev)
    refs, outs, bounds = _windows(plan, d, total, rows, rows, n)
    q0, q1 = DirectQueue(), DirectQueue()
    rs = [bounds[0].direct(q0)] + [b.direct(q1) for b in bounds[1:]]
    ko, slot0, sharers = rs[0].info()
    assert sharers == n
    _clear(outs)
    for r in rs:
        r.run()
    q0.sync()
    q1.sync()
    assert _same(outs, refs)
    # the launch whose bind loaded the code object goes first, then the queue it was loaded through
    first = rs[0]
    rs[0] = None
    del first
    del q0
    gc.collect()
    assert [r.info()[2] for r in rs[1:]] == [n - 1] * (n - 1)
    _clear(outs[1:])
    for _ in range(2):
        for r in rs[1:]:
            r.run()
    q1.sync()
    assert _same(outs[1:], refs[1:])
    again = bounds[0].direct(q1)
    assert again.info() == (ko, slot0, n)  # same executable, the freed slot
    _clear(outs)
    again.run()
    for r in rs[1:]:
        r.run()
    q1.sync()
    assert _same(outs, refs)
    del again, r
    rs.clear()
    gc.collect()
    fresh = bounds[2].direct(q1)
    assert fresh.info()[2] == 1  # nothing was left to share: loaded again
    _clear(outs)
    fresh.run()
    q1.sync()
    assert _same(outs[2:3], refs[2:3])


def test_two_plans_do_not_share(gpu):
    """Two plans of the same template with different missing sets are different code objects: different
    kernel objects, each counted on its own, and interleaved launches give each plan's own results."""
    from pgmpy_amd.inference.batch import upload_codes
    from pgmpy_amd.inference.plan import DirectQueue

    gc.collect()
    rows = 1000
    q = DirectQueue()
    sets = []
    for missing_seed in (307, 308):
        plan, ev = _template("munin", rows * 2, seed=35, missing_seed=missing_seed)
        d = upload_codes(ev)
        refs, outs, bounds = _windows(plan, d, rows * 2, rows, rows, 2)
        sets.append((plan, d, refs, outs, [b.direct(q) for b in bounds]))
    (ia, ib) = (s[4][0].info() for s in sets)
    assert ia[0] != ib[0] and ia[2] == 2 and ib[2] == 2
    assert sets[0][4][1].info()[0] == ia[0] and sets[1][4][1].info()[0] == ib[0]
    for s in sets:
        _clear(s[3])
    for k in range(4):
        for s in sets:
            s[4][k % 2].run()
    q.sync()
    for s in sets:
        assert _same(s[3], s[2])


def test_query_chain_kernargs_in_slab(gpu, monkeypatch):
    """A compiled single query as one AQL chain (pgm_dq_bind_pm / pgm_dq_run_chain) with its steps'
    kernarg segments in the slab: 256-byte-aligned, pairwise distinct, launches of one plan sharing its
    code object — and the alarm queries still match their goldens."""
    from pgmpy_amd.inference import VariableElimination
    from pgmpy_amd.inference.plan import bound_info
    from pgmpy_amd.utils import get_example_model

    monkeypatch.setenv("PGM_QUERY_DIRECT", "1")
    g = load_json("alarm_queries.json")
    ve = VariableElimination(get_example_model("alarm"))
    chains = 0
    for p in g["patterns"][:12]:
        for _ in range(2):
            sep = ve.query(p["variables"], p["evidence"], joint=False, show_progress=False)
        for v in p["variables"]:
            np.testing.assert_allclose(np.asarray(sep[v].values), fac_values(p["marginals"][v]), atol=1e-10, rtol=0)
    seen = []
    for rn in ve._compiled.values():
        for prog, *_ in rn.plan.__dict__.get("_progs", {}).values():
            if not prog._direct:
                continue
            chains += 1
            infos = [bound_info(h) for h in prog._direct]
            assert all(ko and ka and ka % SLOT == 0 and sh >= 1 for ko, ka, sh in infos)
            seen += [ka for _, ka, _ in infos]
    assert chains >= 1, "no alarm query ran as an AQL chain"
    assert len(set(seen)) == len(seen)
