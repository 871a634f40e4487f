"""The streaming form of the specialised row kernels (nontemporal evidence-code loads, write-through
nontemporal output stores: a second hipRTC program per plan) against the default form, in one process
through the PGM_ROWS_STREAM switch: marginals, MAP indices and MAP gaps bit for bit on every kernel of the
program (one row per thread, two rows per thread, the resident ring, the dispatch floors), launched through
pgm_rows_bound_run and through a direct queue, with a row of impossible evidence and a row with an
out-of-range code among the rows."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ROWS = 50_002       # the largest window; even, so every window at row 0 keeps the two-row contract
DEAD_ROW, BAD_ROW = 0, 1
# the forms compared with the default one (PGM_ROWS_STREAM=0): word 3 = nontemporal code loads + sc1 nt stores
# for every launch (both halves of the policy at every size); None = the switch unset, the library's own
# rule (sc1 nt stores from 50,000 rows: streaming at 50,000 / 50,002 rows, the default program below)
FORMS = ("3", None)


def _bits(t):
    import torch

    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    import torch

    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in ("marg", "map", "gap"))


@pytest.fixture(scope="module", params=["munin_c3", "alarm_3"])
def forms(request, gpu):
    """(default-form plan, the plans of FORMS, device codes, host codes, has a dead row) of one model plan:
    the same PatternPlan built once per form, each handle created under its own value of the switch.  munin's CPTs
    are sparse, so uniform code rows hold impossible evidence; alarm has five zero entries in the whole
    network and its plan admits no impossible row (none among 4,096 uniform draws), so there only the
    out-of-range row is planted."""
    import os

    import torch

    from pgmpy_amd.inference.batch import upload_codes
    from pgmpy_amd.inference.plan import PatternPlan
    from pgmpy_amd.utils import get_example_model
    from pgmpy_amd.utils.sampling import forward_sample_codes

    net, seed, k = {"munin_c3": ("munin", 0, 3), "alarm_3": ("alarm", 0, 3)}[request.param]
    m = get_example_model(net)
    missing = random.Random(seed).sample(sorted(m.nodes()), k)
    codes, nodes = forward_sample_codes(m, N_ROWS, seed=23)
    obs = [v for v in nodes if v not in missing]
    pos = {v: i for i, v in enumerate(nodes)}
    ev = np.ascontiguousarray(codes[[pos[v] for v in obs]])
    col_of = {v: i for i, v in enumerate(obs)}
    plans = []
    saved = os.environ.get("PGM_ROWS_STREAM")
    try:
        for word in ("0",) + FORMS:
            if word is None:
                os.environ.pop("PGM_ROWS_STREAM", None)
            else:
                os.environ["PGM_ROWS_STREAM"] = word
            p = PatternPlan(m, missing, obs, col_of)
            assert p.kind == "fused" and p.kernel_name() == "pgm_rows_jit"
            p._build_fused()  # the switch is read when the handle is created
            plans.append(p)
    finally:
        if saved is None:
            os.environ.pop("PGM_ROWS_STREAM", None)
        else:
            os.environ["PGM_ROWS_STREAM"] = saved
    default, streams = plans[0], plans[1:]
    # impossible evidence in DEAD_ROW: the first combination of the plan's evidence codes whose mass is 0
    used = [col_of[v] for v in default.ev_used]
    cards = [len(m.states[v]) for v in default.ev_used]
    rng = np.random.default_rng(5)
    trial = np.stack([rng.integers(0, c, 4096).astype(np.uint8) for c in cards])
    probe = np.ascontiguousarray(np.repeat(ev[:, :1], 4096, axis=1))
    probe[used] = trial
    d_probe = upload_codes(probe)
    out = default.alloc_outputs(4096, marginals=True, map_=True, gap=True)
    default.bind(d_probe, 4096, 0, 4096, out).run()
    torch.cuda.synchronize()
    dead = torch.isnan(out["marg"]).all(dim=0).nonzero().flatten()
    assert (dead.numel() > 0) == (request.param == "munin_c3")
    if dead.numel():
        ev[:, DEAD_ROW] = probe[:, int(dead[0])]
    ev[used[0], BAD_ROW] = 255  # out of range for every cardinality
    return default, streams, upload_codes(ev), ev, dead.numel() > 0


def _run(plan, d, rows, how, floor=False, err=None):
    import torch

    from pgmpy_amd.inference.plan import DirectQueue

    out = plan.alloc_outputs(rows, marginals=True, map_=True, gap=True)
    for t in out.values():
        t.fill_(-7)
    torch.cuda.synchronize()
    b = plan.bind(d, N_ROWS, 0, rows, out, err=err, floor=floor)
    if how == "direct":
        q = DirectQueue.default()
        r = b.direct(q)
        r.run()
        q.sync()
    else:
        b.run()
    torch.cuda.synchronize()
    return out, b.kernel()[0]


@pytest.mark.parametrize("how", ["bound", "direct"])
@pytest.mark.parametrize("rows", [1, 2, 191, 192, 193, 50_000, 50_002])
def test_streaming_form_equals_default_form(forms, rows, how):
    """Around the 192-thread workgroup of the one-row kernel and at the two-row kernel's 50,000-row
    threshold: every output bit for bit, the impossible row NaN / MAP 0 / gap 0, the error flag raised by the
    out-of-range code (from two rows up) and by nothing else."""
    import torch

    default, streams, d, _, has_dead = forms
    err0 = torch.zeros(1, dtype=torch.int32, device=d.device)
    ref, name_ref = _run(default, d, rows, how, err=err0)
    for stream in streams:
        err = torch.zeros(1, dtype=torch.int32, device=d.device)
        got, name = _run(stream, d, rows, how, err=err)
        assert name == name_ref == ("pgm_rows_jit2" if rows >= 50_000 else "pgm_rows_jit")
        assert _same(got, ref)
        if has_dead:
            assert torch.isnan(got["marg"][:, DEAD_ROW]).all() and int(got["map"][DEAD_ROW]) == 0
            assert float(got["gap"][DEAD_ROW]) == 0.0
        assert int(err0.item()) == int(err.item()) == (1 if rows > BAD_ROW else 0)
        live = got["marg"][:, 2:]
        assert not torch.isnan(live).any() and bool((live != -7).all())


def test_out_of_range_code_leaves_the_other_rows_alone(forms):
    """The same window with the out-of-range code put right: only the bad row's outputs differ."""
    import torch

    from pgmpy_amd.inference.batch import upload_codes

    default, (stream, _), d, ev, _ = forms
    fixed = ev.copy()
    fixed[:, BAD_ROW] = ev[:, 2]
    d_fixed = upload_codes(fixed)
    err = torch.zeros(1, dtype=torch.int32, device=d.device)
    clean, _ = _run(stream, d_fixed, 193, "bound", err=err)
    assert int(err.item()) == 0
    got, _ = _run(stream, d, 193, "bound")
    keep = [r for r in range(193) if r != BAD_ROW]
    for k in ("marg", "map", "gap"):
        assert torch.equal(_bits(got[k])[..., keep], _bits(clean[k])[..., keep]), k


@pytest.mark.parametrize("how", ["bound", "direct"])
@pytest.mark.parametrize("rows", [1000, 50_002])
def test_floor_kernels_carry_the_policy(forms, rows, how):
    """pgm_rows_floor / pgm_rows_floor2 of the streaming program write what the default program's do."""
    default, streams, d, _, _ = forms
    ref, name_ref = _run(default, d, rows, how, floor=True)
    for stream in streams:
        got, name = _run(stream, d, rows, how, floor=True)
        assert name == name_ref == ("pgm_rows_floor2" if rows >= 50_000 else "pgm_rows_floor")
        assert _same(got, ref)


@pytest.mark.parametrize("rows", [256, 258])
def test_ring_of_the_streaming_program(forms, rows):
    """The resident ring over 3 slots (windows 0, rows, 2 rows; the first holds the impossible and the
    out-of-range row): each slot equals the default program's ring and the default one-batch launch."""
    import torch

    default, streams, d, _, has_dead = forms
    results = []
    for plan in (default, streams[0]):
        slots = []
        for s in range(3):
            out = plan.alloc_outputs(rows, marginals=True, map_=True, gap=True)
            for t in out.values():
                t.fill_(-7)
            slots.append((d, N_ROWS, s * rows, out))
        err = torch.zeros(1, dtype=torch.int32, device=d.device)
        torch.cuda.synchronize()
        ring = plan.ring(slots, rows, err=err)
        assert ring.kernel()[0] == "pgm_rows_ring"
        ring.run(3)
        torch.cuda.synchronize()
        assert int(err.item()) == 1
        results.append([s[3] for s in slots])
    for s in range(3):
        assert _same(results[1][s], results[0][s]), s
        one = default.alloc_outputs(rows, marginals=True, map_=True, gap=True)
        default.bind(d, N_ROWS, s * rows, rows, one).run()
        torch.cuda.synchronize()
        assert _same(results[1][s], one), s
    if has_dead:
        assert torch.isnan(results[1][0]["marg"][:, DEAD_ROW]).all() and int(results[1][0]["map"][DEAD_ROW]) == 0
