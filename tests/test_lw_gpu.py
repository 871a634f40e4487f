"""The likelihood-weighted posterior on the device (pgm_sample_posterior) and the public API on top of it
(ApproxInference, DiscreteBayesianNetwork.predict(algo=ApproxInference)).

The reference is tests/lw_cases.py's long-double restatement on top of tests/sample_cases.sample_ref,
which tests/test_lw_cpu.py pins to exact posteriors.  Tolerances (tests/lw_cases.py): for post
atol = S * 2^(1 - K) + 4e-13 * n_observed against the unquantised restatement, the same expression relative
for log_evidence; ess against the restatement's with q' floored to 20 bits, at the relative bound of every
q' being off by one (lw_cases.ess_tolerance).  acc is compared bit for bit between launch geometries and
batches."""
import functools
import json
import os

import numpy as np
import pandas as pd
import pytest

from tests import lw_cases as LW
from tests import sample_cases as SC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dev(a):
    from pgmpy_amd import engine as E

    return E.to_device_raw(np.ascontiguousarray(a))


def _host(t):
    from pgmpy_amd.inference.batch import download

    return None if t is None else download(t)


def run(fams, tables, modes, ev, targets, S, seed=0, first_row=0, block=0, row0=0, pad=0, raises=False,
        expect_block=None):
    """pgm_sample_posterior over the evidence columns `ev` [n_cols, R], placed at rows [row0, row0 + R) of a
    buffer with `pad` more rows behind them: (acc, scale, post, log_evidence, ess) on the host."""
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.sampling._sample import SamplePlan

    sp, tp = SamplePlan(fams), FitPlan(targets)
    R = ev.shape[1]
    info = sp.posterior_info(tp, R, S, block)
    assert info.chunk == LW.CHUNK and info.k == LW.k_of(S)
    if expect_block is not None:
        assert info.block == expect_block
    buf = np.full((ev.shape[0], row0 + R + pad), 0xAB, dtype=np.uint8)
    buf[:, row0:row0 + R] = ev
    values = _dev(np.concatenate([np.asarray(t, dtype=np.float64).ravel() for t in tables]))
    cdf = sp.cdf(values)
    try:
        out = sp.posterior(tp, values, cdf, _dev(buf), S, n_rows=R, row0=row0, first_row=first_row, seed=seed,
                           modes=modes, block=block)
        assert not raises
    except IndexError as e:
        assert raises, e
        out = e.posterior
    return tuple(_host(t) for t in out)


def check_rows(got, ref, fams, modes, ev, S, rows=None):
    """post, log_evidence and ess of the device rows against the restatement's."""
    acc, scale, post, le, ess = got
    for r in (range(ev.shape[1]) if rows is None else rows):
        want = ref[r]
        tol = LW.tolerance(S, LW.n_observed(fams, modes, ev[:, r]))
        wp = want["post"].astype(np.float64)
        if np.isnan(wp).all():
            assert np.isnan(post[r]).all() and (acc[r] == 0).all(), r
        else:
            err = np.abs(post[r].astype(np.longdouble) - want["post"]).max()
            print(f"row {r}: post err {float(err):.3e} tol {tol:.3e}")
            assert err <= tol, (r, float(err), tol)
        wl = float(want["log_evidence"])
        if np.isfinite(wl):
            print(f"row {r}: log_evidence {le[r]!r} want {wl!r}")
            assert abs(le[r] - wl) <= tol * abs(wl), (r, le[r], wl)
        else:
            assert le[r] == wl or (np.isnan(wl) and np.isnan(le[r])), (r, le[r], wl)
        if want["w"].max() > 0 and not want["bad"]:
            we, sq1 = LW.ess_ref(want["w"])
            assert abs(ess[r] - we) <= LW.ess_tolerance(S, sq1) * we, (r, ess[r], we)
        else:
            assert ess[r] == 0, (r, ess[r])


# ---------------------------------------------------------------------------- 1: plan order, sample counts
@pytest.mark.parametrize("S", LW.SAMPLE_COUNTS)
def test_plan_order_and_sample_count_edges(gpu, S):
    fams, tables, _ = LW.plan_order_net()
    ev = LW.PLAN_ORDER_EVIDENCE
    ref = LW.posterior_ref(fams, tables, LW.PLAN_ORDER_MODES, ev, LW.PLAN_ORDER_TARGETS, S, seed=5)
    got = run(fams, tables, LW.PLAN_ORDER_MODES, ev, LW.PLAN_ORDER_TARGETS, S, seed=5, expect_block=256)
    check_rows(got, ref, fams, LW.PLAN_ORDER_MODES, ev, S)
    acc = got[0]
    layout, _ = LW.target_layout(LW.PLAN_ORDER_TARGETS)
    for r in range(ev.shape[1]):  # every family's bins hold the same total, between 2^K and S 2^K
        sums = {int(acc[r, off:off + size].sum()) for off, size in layout}
        assert len(sums) == 1 and (1 << LW.k_of(S)) <= sums.pop() <= (S << LW.k_of(S))
    # the row with everything observed is one-hot in every table, the row with nothing observed weighs 1
    assert np.array_equal(np.sort(got[2][1])[-len(layout):], np.ones(len(layout)))
    assert got[3][0] == 0.0 and got[4][0] == S and got[1][0] == 0.0


def test_given_mode_takes_the_code_without_weight(gpu):
    """GIVEN holds a column at its code and leaves the weight alone; FREE never reads the evidence."""
    fams, tables, _ = LW.plan_order_net()
    ev = LW.PLAN_ORDER_EVIDENCE
    modes = [LW.GIVEN, LW.OBSERVED, LW.FREE, LW.OBSERVED]
    ref = LW.posterior_ref(fams, tables, modes, ev, LW.PLAN_ORDER_TARGETS, 200, seed=9)
    got = run(fams, tables, modes, ev, LW.PLAN_ORDER_TARGETS, 200, seed=9)
    check_rows(got, ref, fams, modes, ev, 200)


# ---------------------------------------------------------------------------- 2: underflow
def test_log_weights_do_not_underflow(gpu):
    fams, tables, ev = LW.chain_net()
    modes = [LW.OBSERVED] * len(fams)
    targets = [([c], [2]) for c in (300, 305, 319)] + [([310, 301], [2, 2])]
    S = 256
    ref = LW.posterior_ref(fams, tables, modes, ev, targets, S, seed=4)
    for r in range(2):
        assert float(ref[r]["w"].astype(np.float64).max()) == 0.0  # a product of the weights is 0 in fp64
        assert -2200 < float(ref[r]["log_evidence"]) < -1800
    # 320 columns: 256 lanes would need 8 * 10 + 2048 + 320 * 256 = 84,048 bytes, inside the budget, so no
    # step-down is forced by the columns alone; the info must say what the formula says
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.sampling._sample import SamplePlan

    info = SamplePlan(fams).posterior_info(FitPlan(targets), 2, S)
    assert (info.block, info.lds_bytes) == (256, 8 * 10 + 2048 + 320 * 256)
    got = run(fams, tables, modes, ev, targets, S, seed=4)
    assert np.isfinite(got[2]).all()
    check_rows(got, ref, fams, modes, ev, S)
    # the step-down itself, with enough bins that 256 lanes do not fit: 8 * 10240 + 2048 + 320 * 256 > 163,840
    big = [([300 + i for i in range(13)], [2] * 13), ([305 + i for i in range(11)], [2] * 11)]
    info = SamplePlan(fams).posterior_info(FitPlan(big), 2, S)
    assert (info.block, info.lds_bytes) == (128, 8 * 10240 + 2048 + 320 * 128)
    got = run(fams, tables, modes, ev, big, S, seed=4, expect_block=128)
    check_rows(got, LW.posterior_ref(fams, tables, modes, ev, big, S, seed=4), fams, modes, ev, S)


# ---------------------------------------------------------------------------- 3: zero probability
def test_zero_probability(gpu):
    fams, tables, ev = LW.zero_net()
    targets = [([0], [2]), ([1], [2]), ([0, 1], [2, 2])]
    modes = [LW.OBSERVED, LW.OBSERVED]
    ref = LW.posterior_ref(fams, tables, modes, ev, targets, 300, seed=2)
    acc, scale, post, le, ess = got = run(fams, tables, modes, ev, targets, 300, seed=2)
    assert np.isnan(post[0]).all() and (acc[0] == 0).all() and le[0] == -np.inf and ess[0] == 0 and scale[0] == -np.inf
    assert 0 < (ref[1]["w"] == 0).sum() < 300  # only some samples of row 1 have weight 0
    check_rows(got, ref, fams, modes, ev, 300)
    assert np.array_equal(post[1], [0, 1, 0, 1, 0, 0, 0, 1])


# ---------------------------------------------------------------------------- 4: bad code
def test_bad_code_spoils_its_row_only(gpu):
    fams, tables, _ = LW.plan_order_net()
    ev = LW.PLAN_ORDER_EVIDENCE.copy()
    S = LW.CHUNK + 1
    clean = run(fams, tables, LW.PLAN_ORDER_MODES, ev, LW.PLAN_ORDER_TARGETS, S, seed=5)
    ev[2, 3] = 4  # C has 4 states
    acc, scale, post, le, ess = run(fams, tables, LW.PLAN_ORDER_MODES, ev, LW.PLAN_ORDER_TARGETS, S, seed=5, raises=True)
    assert np.isnan(post[3]).all() and (acc[3] == 0).all() and ess[3] == 0 and np.isnan(le[3]) and np.isnan(scale[3])
    keep = [0, 1, 2, 4, 5]
    for a, b in zip(clean, (acc, scale, post, le, ess)):
        assert np.array_equal(a[keep], b[keep], equal_nan=True)
    # a 254 in a FREE column is never read
    modes = [LW.OBSERVED, LW.OBSERVED, LW.FREE, LW.OBSERVED]
    ev[2, 3] = 254
    run(fams, tables, modes, ev, LW.PLAN_ORDER_TARGETS, 10, seed=5)


# ---------------------------------------------------------------------------- 5: geometry and batch independence
def test_acc_is_bit_identical_across_geometry_and_batches(gpu):
    fams, tables, _ = LW.plan_order_net()
    ev = LW.PLAN_ORDER_EVIDENCE[:, 1:6]  # 5 rows
    S = 2 * LW.CHUNK + 3
    kw = dict(seed=8, first_row=1000)
    base = run(fams, tables, LW.PLAN_ORDER_MODES, ev, LW.PLAN_ORDER_TARGETS, S, block=256, **kw)
    for block in (64, 128):
        other = run(fams, tables, LW.PLAN_ORDER_MODES, ev, LW.PLAN_ORDER_TARGETS, S, block=block, expect_block=block, **kw)
        for a, b in zip(base, other):
            assert np.array_equal(a, b, equal_nan=True), block
    for r in range(5):  # each row alone, its stream shifted
        alone = run(fams, tables, LW.PLAN_ORDER_MODES, ev[:, r:r + 1], LW.PLAN_ORDER_TARGETS, S, seed=8,
                    first_row=1000 + r * S)
        for a, b in zip(base, alone):
            assert np.array_equal(a[r], b[0], equal_nan=True), r
    moved = run(fams, tables, LW.PLAN_ORDER_MODES, ev, LW.PLAN_ORDER_TARGETS, S, row0=3, pad=6, **kw)
    for a, b in zip(base, moved):
        assert np.array_equal(a, b, equal_nan=True)
    # and the integer scheme itself: the device's sums are the contract's up to the last bits of log / exp
    ref = LW.posterior_ref(fams, tables, LW.PLAN_ORDER_MODES, ev, LW.PLAN_ORDER_TARGETS, S, **kw)
    for r in range(5):
        want = LW.acc_ref(fams, tables, LW.PLAN_ORDER_MODES, ev[:, r], LW.PLAN_ORDER_TARGETS, ref[r]["codes"])[0]
        n_obs = LW.n_observed(fams, LW.PLAN_ORDER_MODES, ev[:, r])
        assert np.abs(base[0][r].astype(np.float64) - want.astype(np.float64)).max() <= S * 2.0 ** LW.k_of(S) * 4e-13 * max(n_obs, 1)


def test_rows_past_one_launch(gpu):
    """A launch covers 65,535 rows when a row is one chunk: the rows behind that go to a second launch of the
    same call, with their own evidence window, stream rows and outputs."""
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.sampling._sample import SamplePlan

    fams, tables, _ = LW.plan_order_net()
    S, R, tail = 3, 65535 + 5, 5
    assert SamplePlan(fams).posterior_info(FitPlan(LW.PLAN_ORDER_TARGETS), R, S).rows_per_launch == R - tail
    ev = np.tile(LW.PLAN_ORDER_EVIDENCE, (1, R // 6 + 1))[:, :R]
    batch = run(fams, tables, LW.PLAN_ORDER_MODES, ev, LW.PLAN_ORDER_TARGETS, S, seed=6, first_row=11)
    last = ev[:, R - tail:]
    alone = run(fams, tables, LW.PLAN_ORDER_MODES, last, LW.PLAN_ORDER_TARGETS, S, seed=6, first_row=11 + (R - tail) * S)
    for a, b in zip(batch, alone):
        assert np.array_equal(a[R - tail:], b, equal_nan=True)
    ref = LW.posterior_ref(fams, tables, LW.PLAN_ORDER_MODES, last, LW.PLAN_ORDER_TARGETS, S, seed=6,
                           first_row=11 + (R - tail) * S)
    check_rows(alone, ref, fams, LW.PLAN_ORDER_MODES, last, S)
    layout, _ = LW.target_layout(LW.PLAN_ORDER_TARGETS)
    sums = batch[0][:, :layout[0][1]].sum(axis=1)  # every row was accumulated once: between 2^K and S 2^K
    assert (sums >= 1 << LW.k_of(S)).all() and (sums <= S << LW.k_of(S)).all()


# ---------------------------------------------------------------------------- 6: the sampler's stream
@functools.lru_cache(maxsize=None)
def alarm():
    from pgmpy_amd.utils import get_example_model

    with open(os.path.join(GOLDEN, "alarm_predict.json")) as f:
        g = json.load(f)
    m = get_example_model("alarm")
    return (m, g) + SC.model_plan(m)


def alarm_evidence(m, g, nodes, rows, columns):
    ev = np.full((len(nodes), len(rows)), LW.MISSING, dtype=np.uint8)
    for r, row in enumerate(rows):
        for v, s in zip(g["columns"], row):
            if v in columns and s is not None:
                ev[nodes.index(v), r] = list(m.states[v]).index(s)
    return ev


def test_same_stream_as_the_forward_sampler(gpu):
    import torch

    from pgmpy_amd.sampling._sample import SamplePlan

    m, g, nodes, order, fams, tables = alarm()
    S, R = 500, 3
    ev = alarm_evidence(m, g, nodes, g["rows"][:R], set(g["columns"]))
    targets = [([nodes.index(v)], [len(m.states[v])]) for v in g["missing"]]
    modes = [LW.OBSERVED] * len(fams)
    acc, scale, post, le, ess = run(fams, tables, modes, ev, targets, S, seed=21)
    sp = SamplePlan(fams)
    values = _dev(np.concatenate([np.asarray(t, dtype=np.float64).ravel() for t in tables]))
    codes = _dev(np.repeat(ev, S, axis=1))
    w = torch.empty(R * S, dtype=torch.float64, device=codes.device)
    sp.forward(sp.cdf(values), codes, seed=21, modes=modes, values=values, weights=w)
    codes, w = _host(codes), _host(w).astype(np.longdouble)
    bins = LW.target_bins(targets, codes)
    for r in range(R):
        hist = np.zeros(post.shape[1], dtype=np.longdouble)
        for t in range(len(targets)):
            np.add.at(hist, bins[t, r * S:(r + 1) * S], w[r * S:(r + 1) * S])
        want = hist / w[r * S:(r + 1) * S].sum()
        tol = LW.tolerance(S, LW.n_observed(fams, modes, ev[:, r]))
        assert np.abs(post[r] - want).max() <= tol, r
        wl = float(np.log(w[r * S:(r + 1) * S].sum() / S))
        assert abs(le[r] - wl) <= tol * abs(wl)


# ---------------------------------------------------------------------------- 7: the public API
def test_query_and_map_query_on_alarm(gpu):
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.inference import ApproxInference

    m, g, nodes, order, fams, tables = alarm()
    evidence = {"HRBP": "HIGH", "CVP": "NORMAL", "BP": "LOW"}
    virt = TabularCPD("HISTORY", 2, [[0.9], [0.1]], state_names={"HISTORY": list(m.states["HISTORY"])})
    variables = ["LVFAILURE", "STROKEVOLUME"]
    S, seed = 3000, 33
    # the restatement on the rewritten model: __HISTORY, a binary child held at 0, in a column after the model's
    m2 = m.copy()
    m2.add_edge("HISTORY", "__HISTORY")
    m2.add_cpds(TabularCPD("__HISTORY", 2, [[0.9, 0.1], [0.1, 0.9]], evidence=["HISTORY"], evidence_card=[2],
                           state_names={"__HISTORY": [0, 1], "HISTORY": list(m.states["HISTORY"])}))
    nodes2, _, fams2, tables2 = SC.model_plan(m2, nodes=nodes + ["__HISTORY"])
    ev = np.full((len(nodes2), 1), LW.MISSING, dtype=np.uint8)
    for v, s in evidence.items():
        ev[nodes2.index(v), 0] = list(m.states[v]).index(s)
    ev[nodes2.index("__HISTORY"), 0] = 0
    cards = [len(m.states[v]) for v in variables]
    joint_t = [([nodes2.index(v) for v in variables], cards)]
    ref = LW.posterior_ref(fams2, tables2, [LW.OBSERVED] * len(fams2), ev, joint_t, S, seed=seed)[0]
    tol = LW.tolerance(S, 4)
    infer = ApproxInference(m)
    f = infer.query(variables, n_samples=S, evidence=evidence, virtual_evidence=[virt], seed=seed)
    assert list(f.variables) == variables and list(f.cardinality) == cards
    assert np.abs(np.asarray(f.values).ravel() - ref["post"].astype(np.float64)).max() <= tol
    want = ref["post"].astype(np.float64).reshape(cards)
    per = infer.query(variables, n_samples=S, evidence=evidence, virtual_evidence=[virt], seed=seed, joint=False)
    for i, v in enumerate(variables):
        assert np.abs(np.asarray(per[v].values) - want.sum(axis=1 - i)).max() <= 2 * max(cards) * tol
    top = np.sort(want.ravel())[-2:]
    assert top[1] - top[0] > 1e-9 * top[1]
    idx = np.unravel_index(int(np.argmax(want)), cards)
    assert infer.map_query(variables, n_samples=S, evidence=evidence, virtual_evidence=[virt], seed=seed) == \
        {v: m.states[v][k] for v, k in zip(variables, idx)}
    # state_names selects and orders
    sub = infer.query(["LVFAILURE"], n_samples=S, evidence=evidence, seed=seed, state_names={"LVFAILURE": ["FALSE", "nope"]})
    full = infer.query(["LVFAILURE"], n_samples=S, evidence=evidence, seed=seed)
    assert sub.state_names["LVFAILURE"] == ["FALSE", "nope"]
    assert np.array_equal(np.asarray(sub.values), [np.asarray(full.values)[list(m.states["LVFAILURE"]).index("FALSE")], 0.0])


def test_query_batch_and_predict_on_alarm(gpu):
    from pgmpy_amd.inference import ApproxInference

    m, g, nodes, fams, tables, keep, missing, ev = LW.alarm_api_case()
    data = pd.DataFrame([dict(zip(g["columns"], row)) for row in g["rows"][:LW.API_ROWS]])[keep]
    modes = [LW.OBSERVED] * len(fams)
    assert len(missing) == 5
    S, seed = LW.API_S, LW.API_SEED
    # query_batch: the marginals of every missing variable, log_evidence, ess
    singles = [([nodes.index(v)], [len(m.states[v])]) for v in missing]
    ref = LW.posterior_ref(fams, tables, modes, ev, singles, S, seed=seed)
    out = ApproxInference(m).query_batch(data, variables=missing, n_samples=S, seed=seed)
    names = [f"{v}_{s}" for v in missing for s in m.states[v]]
    assert list(out.columns) == names + ["log_evidence", "ess"] and out.index.equals(data.index)
    for r in range(LW.API_ROWS):
        tol = LW.tolerance(S, LW.n_observed(fams, modes, ev[:, r]))
        assert np.abs(out[names].to_numpy()[r] - ref[r]["post"].astype(np.float64)).max() <= tol, r
        wl = float(ref[r]["log_evidence"])
        assert abs(out["log_evidence"].iloc[r] - wl) <= tol * abs(wl)
        we, sq1 = LW.ess_ref(ref[r]["w"])
        assert abs(out["ess"].iloc[r] - we) <= LW.ess_tolerance(S, sq1) * we
    # predict: the joint MAP of the five missing variables
    pred = m.predict(data, algo=ApproxInference, n_samples=S, seed=seed)
    assert list(pred.columns[:len(keep)]) == keep and set(pred.columns[len(keep):]) == set(missing)
    cards = [len(m.states[v]) for v in missing]
    joint = LW.posterior_ref(fams, tables, modes, ev, [([nodes.index(v) for v in missing], cards)], S, seed=seed)
    left_out = 0
    for r in range(LW.API_ROWS):
        p = joint[r]["post"].astype(np.float64)
        top = np.sort(p)[-2:]
        if top[1] - top[0] <= 1e-9 * top[1]:
            left_out += 1
            continue
        idx = np.unravel_index(int(np.argmax(p)), cards)
        assert {v: pred[v].iloc[r] for v in missing} == {v: m.states[v][k] for v, k in zip(missing, idx)}, r
    assert left_out == 0
    # by default the targets are the variables missing in some row: two rows lack an observed cell as well
    nan_cols = [v for v in keep if data[v].isna().any()]
    assert nan_cols
    auto = ApproxInference(m).query_batch(data, n_samples=S, seed=seed)
    assert {c.rsplit("_", 1)[0] for c in auto.columns[:-2]} == set(missing) | set(nan_cols)
    assert np.array_equal(auto[names].to_numpy(), out[names].to_numpy())
    for v in nan_cols:  # a target that a row observes is one-hot there
        cols = [f"{v}_{s}" for s in m.states[v]]
        seen = ~data[v].isna().to_numpy()
        onehot = (np.asarray(m.states[v], dtype=object)[None, :] == data[v].to_numpy()[seen, None]).astype(float)
        assert np.array_equal(auto[cols].to_numpy()[seen], onehot)


def test_get_distribution_and_map_query_match_the_golden(gpu):
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.inference import ApproxInference
    from pgmpy_amd.models import DiscreteBayesianNetwork

    with open(os.path.join(GOLDEN, "approx_cases.json")) as f:
        g = json.load(f)
    with open(os.path.join(GOLDEN, "metrics_cases.json")) as f:
        meta = json.load(f)
    states = meta["states"]
    m = DiscreteBayesianNetwork([tuple(e) for e in meta["edges"]])
    for v in meta["nodes"]:
        variables = meta["cpds"][v]["variables"]
        m.add_cpds(TabularCPD(v, len(states[v]), meta["cpds"][v]["values"], evidence=variables[1:] or None,
                              evidence_card=[len(states[u]) for u in variables[1:]] or None,
                              state_names={u: states[u] for u in variables}))
    nodes = sorted(states)
    codes = np.load(os.path.join(GOLDEN, "metrics_cases.npz"))["net5_codes1000"][:, :g["n_rows"]]
    frame = pd.DataFrame({v: [states[v][k] for k in codes[i]] for i, v in enumerate(nodes)})
    infer = ApproxInference(m)
    for state_names in (None, states):
        j = infer.get_distribution(frame, g["joint"]["variables"], state_names=state_names)
        assert list(j.variables) == g["joint"]["variables"] and list(j.cardinality) == g["joint"]["cardinality"]
        assert np.array_equal(np.asarray(j.values).ravel(), g["joint"]["values"])
        per = infer.get_distribution(frame, nodes, state_names=state_names, joint=False)
        for v in nodes:
            assert np.array_equal(np.asarray(per[v].values).ravel(), g["marginals"][v]["values"])
    assert infer.map_query(g["joint"]["variables"], samples=frame) == g["map_joint"]
    assert infer.map_query(g["map2_variables"], samples=frame) == g["map2"]
    sub = infer.get_distribution(frame, g["subset"]["variables"], state_names=g["subset"]["state_names"])
    assert np.array_equal(np.asarray(sub.values).ravel(), g["subset"]["values"])
    assert {v: list(sub.state_names[v]) for v in sub.variables} == g["subset"]["state_names"]
    assert np.array_equal(np.asarray(infer.query(["A"], samples=frame).values), g["marginals"]["A"]["values"])


def test_predict_errors(gpu):
    from pgmpy_amd.inference import ApproxInference

    m, g, nodes, order, fams, tables = alarm()
    data = pd.DataFrame([dict(zip(g["columns"], row)) for row in g["rows"][:2]])
    with pytest.raises(NotImplementedError):
        m.predict(data, algo=ApproxInference, stochastic=True)
    # 14 columns left: the joint of the other 23 variables is far past the bin budget
    with pytest.raises(ValueError, match=r"bin budget for this model is \d+"):
        m.predict(data[g["columns"][:14]], algo=ApproxInference, n_samples=100, seed=1)
