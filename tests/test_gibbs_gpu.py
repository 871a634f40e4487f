"""Gibbs sampling on the device: the sweep kernel on both paths (K1-K4), clamp and trace (K5), the error
flags (K6), the public API on a Bayesian and a Markov network (P1-P3), the distribution (D1, D2) and the
round trip sample -> count -> fit -> sample (R1, R2).

The reference is tests/gibbs_cases.py's numpy restatement, which tests/test_gibbs_cpu.py pins to the
generator, to the exact sweep transition matrix and to the distribution.  Codes are compared exactly."""
import functools

import numpy as np
import pandas as pd
import pytest

from tests import gibbs_cases as G
from tests import sample_cases as S

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB


def _dev(a):
    from pgmpy_amd import engine as E

    return E.to_device_raw(np.ascontiguousarray(a))


def _host(t):
    from pgmpy_amd.inference.batch import download

    return download(t)


def _plan(factors, card):
    from pgmpy_amd.sampling._gibbs import GibbsPlan

    return GibbsPlan(factors, card)


def run_device(factors, tables, card, start, n_sweeps, ld=None, row0=0, first_chain=0, first_sweep=1, seed=0,
               clamp=None, explicit=None, thin=None, expect_path=None, calls=None, raises=None):
    """The kernel over a sentinel-filled buffer: (codes [n_cols, n], records or None).  Asserts that nothing
    outside [row0, row0 + n) was written.  calls: [n_sweeps] of consecutive calls (default: one)."""
    import torch

    plan = _plan(factors, card)
    n_cols, n = start.shape
    ld = row0 + n if ld is None else ld
    values = _dev(np.concatenate([np.asarray(t, dtype=np.float64).ravel() for t in tables]))
    buf = np.full((n_cols, ld), SENTINEL, dtype=np.uint8)
    buf[:, row0:row0 + n] = start
    codes = _dev(buf)
    if expect_path is not None:
        assert plan.launch_info(n).path == expect_path
    err, records, done = None, [], 0
    for k in (calls or [n_sweeps]):
        uni = None
        if explicit is not None:
            ub = np.full((k, n_cols, ld), 0.5)
            ub[:, :, row0:row0 + n] = explicit[done:done + k]
            uni = _dev(ub)
        trace = torch.full((n_cols, (k // thin) * n + 3), SENTINEL, dtype=torch.uint8, device=codes.device) if thin else None
        try:
            plan.sweep(values, codes, k, n_chains=n, row0=row0, first_chain=first_chain, first_sweep=first_sweep + done,
                       seed=seed, clamp=clamp, trace=trace, thin=thin or 1, uniforms=uni)
        except (IndexError, ValueError) as e:
            err = e
        if thin:
            t = _host(trace)
            assert (t[:, (k // thin) * n:] == SENTINEL).all(), "bytes past the last record were written"
            records += [t[:, i * n:(i + 1) * n] for i in range(k // thin)]
        done += k
    assert (err is not None) == bool(raises), err
    if raises:
        assert isinstance(err, raises), err
    out = _host(codes)
    outside = np.ones(ld, dtype=bool)
    outside[row0:row0 + n] = False
    assert (out[:, outside] == SENTINEL).all(), "bytes outside the chain window were written"
    return out[:, row0:row0 + n], (records if thin else None)


@functools.lru_cache(maxsize=None)
def alarm():
    from pgmpy_amd.utils import get_example_model

    m = get_example_model("alarm")
    return (m,) + G.bn_factors(m)


@functools.lru_cache(maxsize=None)
def alarm_start(n, seed=11):
    _, nodes, fams, tables, _ = alarm()
    codes = S.sample_ref(fams, tables, n, seed=seed, n_cols=len(nodes))[0]
    codes.flags.writeable = False
    return codes


@functools.lru_cache(maxsize=None)
def alarm_ref(n, n_sweeps, seed=11):
    _, _, fams, tables, card = alarm()
    out = G.gibbs_ref(fams, tables, card, alarm_start(n, seed), n_sweeps, seed=seed)[0]
    out.flags.writeable = False
    return out


def _paths():
    from pgmpy_amd.sampling._gibbs import GLOBAL, LDS

    return LDS, GLOBAL


# ---------------------------------------------------------------------------- K1: alarm on the LDS path
@pytest.mark.parametrize("row0", [0, 3])
@pytest.mark.parametrize("n", [1, 5, 64, 257, 1030])
def test_alarm_codes_exact(gpu, n, row0):
    """K1: 3 sweeps of alarm from the forward start: the codes equal the restatement's at chain counts
    around the wave and the workgroup, anywhere in a wider buffer, and nothing else is written."""
    _, _, fams, tables, card = alarm()
    got, _ = run_device(fams, tables, card, alarm_start(1030)[:, :n], 3, ld=row0 + n + 5, row0=row0, seed=11,
                        expect_path=_paths()[0])
    want = alarm_ref(1030, 3)[:, :n]
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert n < 64 or (got != alarm_start(1030)[:, :n]).any()


# ---------------------------------------------------------------------------- K2: split and offset invariance
def test_split_and_offset_invariance(gpu):
    """K2: 6 sweeps in one call equal 2 + 4 with first_sweep; chains [100, 130) drawn alone equal that
    slice of a 300-chain call."""
    _, _, fams, tables, card = alarm()
    start = alarm_start(1030)[:, :300]
    want = G.gibbs_ref(fams, tables, card, start, 6, seed=11)[0]
    one, _ = run_device(fams, tables, card, start, 6, seed=11)
    split, _ = run_device(fams, tables, card, start, 6, seed=11, calls=[2, 4])
    part, _ = run_device(fams, tables, card, start[:, 100:130], 6, seed=11, first_chain=100, row0=1, ld=40)
    assert np.array_equal(one, want) and np.array_equal(split, want) and np.array_equal(part, want[:, 100:130])
    later, _ = run_device(fams, tables, card, start, 2, seed=11, first_sweep=2 ** 32 - 2)
    assert np.array_equal(later, G.gibbs_ref(fams, tables, card, start, 2, seed=11, first_sweep=2 ** 32 - 2)[0])


# ---------------------------------------------------------------------------- K3: the global path
@functools.lru_cache(maxsize=None)
def chain_case(n_vars):
    factors, tables, card = G.chain_network(n_vars, seed=5)
    start = G.start_ref(card, 130, seed=8)
    want = G.gibbs_ref(factors, tables, card, start, 2, seed=8)[0]
    return factors, tables, card, start, want


def test_global_path_codes_exact(gpu):
    """K3: a 4,096-variable binary chain (4,096 x 64 B is more than a CU's LDS: the state stays in the code
    matrix), 130 chains, 2 sweeps; and the same network cut to the largest size of the LDS path and to one
    column more, the thresholds read from plan_info: both paths give the restatement's codes."""
    LDS, GLOBAL = _paths()
    factors, tables, card, start, want = chain_case(4096)
    assert 4096 * 64 > 160 * 1024
    got, _ = run_device(factors, tables, card, start, 2, seed=8, row0=2, ld=135, expect_path=GLOBAL)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    info = _plan(factors, card).launch_info(130)
    edge = info.lds_budget // info.block
    for n_vars, path in ((edge, LDS), (edge + 1, GLOBAL)):
        factors, tables, card, start, want = chain_case(n_vars)
        got, _ = run_device(factors, tables, card, start, 2, seed=8, expect_path=path)
        assert np.array_equal(got, want), (n_vars, np.argwhere(got != want)[:8])


def test_global_path_clamp_trace_and_uniforms(gpu):
    """K3: the global path with a clamp, a trace and explicit uniforms (every kernel instance of the path)."""
    LDS, GLOBAL = _paths()
    info = _plan(*[G.chain_network(4)[i] for i in (0, 2)]).launch_info(1)
    n_vars = info.lds_budget // info.block + 1
    factors, tables, card = G.chain_network(n_vars, seed=6)
    start = G.start_ref(card, 70, seed=9)
    clamp = np.zeros(n_vars, dtype=np.uint8)
    clamp[[0, 7, n_vars - 1]] = 1
    want, recs, _, _ = G.gibbs_ref(factors, tables, card, start, 3, seed=9, clamp=clamp, thin=1)
    got, got_recs = run_device(factors, tables, card, start, 3, seed=9, clamp=clamp, thin=1, expect_path=GLOBAL)
    assert np.array_equal(got, want) and all(np.array_equal(a, b) for a, b in zip(got_recs, recs)) and len(got_recs) == 3
    rng = np.random.default_rng(3)
    explicit = rng.random((2, n_vars, 70))
    want = G.gibbs_ref(factors, tables, card, start, 2, explicit=explicit)[0]
    got, _ = run_device(factors, tables, card, start, 2, explicit=explicit, expect_path=GLOBAL)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------- K4: rounding and boundaries
@pytest.mark.parametrize("K", [5, 254])
def test_rounding_and_boundaries(gpu, K):
    """K4: a variable with four incident factors of full-mantissa random values and exact zeros (first,
    middle and last state); explicit uniforms at every c_s / c_{K-1}, one ulp below, one and two ulps
    above, at 0 and at 1 - 2^-53: the chosen state equals the restatement's for every one of them.  An
    FMA in the running sums or a reordered product moves a boundary.  K = 5 keeps the weights in
    registers, K = 254 recomputes them."""
    factors, tables, card = G.boundary_case(K, seed=K)
    info = _plan(factors, card).launch_info(1)
    assert (K <= info.reg_card) == (K == 5) and info.max_degree == 4
    clamp = [0, 1, 1, 1]
    for others in ([1, 0, 1], [0, 1, 0]):
        state = np.array([K // 3] + others, dtype=np.uint8)
        us = G.boundary_uniforms(factors, tables, card, state)
        assert len(us) >= 3 * K and us[0] == 0.0 and us[1] == 1.0 - 2.0 ** -53
        start = np.repeat(state[:, None], len(us), axis=1)
        explicit = np.full((1, 4, len(us)), 0.5)
        explicit[0, 0] = us
        want, _, undrawn, bad = G.gibbs_ref(factors, tables, card, start, 1, clamp=clamp, explicit=explicit)
        assert not undrawn and not bad
        w = G.conditional(factors, tables, G.incident(factors, 4)[0], state.reshape(-1, 1), K)[:, 0]
        assert w[0] == 0 and w[K // 2] == 0 and w[K - 1] == 0 and (w[want[0]] > 0).all()
        assert want[0, 0] == 1 and want[0, 1] == K - 2 and len(set(want[0])) >= K - 3
        got, _ = run_device(factors, tables, card, start, 1, clamp=clamp, explicit=explicit, row0=1, ld=len(us) + 2)
        assert np.array_equal(got, want), [(float(us[i]).hex(), int(got[0, i]), int(want[0, i]))
                                           for i in np.argwhere(got[0] != want[0]).ravel()[:8]]


def test_degree_past_any_register_budget(gpu):
    """K4: no bound on the degree: a variable in 40 factors, with a small and with a large cardinality."""
    for K in (3, 100):
        rng = np.random.default_rng(K)
        factors = [([v, 0], [2, K]) for v in range(1, 41)]
        tables = [rng.uniform(0.5, 1.5, size=2 * K) for _ in factors]
        card = [K] + [2] * 40
        assert _plan(factors, card).launch_info(1).max_degree == 40
        start = G.start_ref(card, 77, seed=4)
        want = G.gibbs_ref(factors, tables, card, start, 2, seed=4)[0]
        got, _ = run_device(factors, tables, card, start, 2, seed=4)
        assert np.array_equal(got, want)


# ---------------------------------------------------------------------------- K5: clamp and trace
def test_clamp_and_trace(gpu):
    """K5: clamped columns never change; with thin = 2 and 7 sweeps the three records and the final state
    equal the restatement's (the LDS path)."""
    _, nodes, fams, tables, card = alarm()
    start = alarm_start(1030)[:, :300]
    clamp = np.zeros(len(nodes), dtype=np.uint8)
    clamp[[0, 5, 17, 36]] = 1
    want, recs, _, _ = G.gibbs_ref(fams, tables, card, start, 7, seed=11, clamp=clamp, thin=2)
    got, got_recs = run_device(fams, tables, card, start, 7, seed=11, clamp=clamp, thin=2, row0=3, ld=310,
                               expect_path=_paths()[0])
    assert len(got_recs) == 3 == len(recs)
    for a, b in zip(got_recs, recs):
        assert np.array_equal(a, b)
    assert np.array_equal(got, want)
    for c in (0, 5, 17, 36):
        assert (got[c] == start[c]).all() and all((r[c] == start[c]).all() for r in got_recs)
    assert not np.array_equal(got_recs[2], got)  # the seventh sweep moved some chain
    # records of split calls continue: 4 + 4 sweeps with thin 2 are the records of 8
    want8, recs8, _, _ = G.gibbs_ref(fams, tables, card, start, 8, seed=11, clamp=clamp, thin=2)
    got8, got_recs8 = run_device(fams, tables, card, start, 8, seed=11, clamp=clamp, thin=2, calls=[4, 4])
    assert np.array_equal(got8, want8) and len(got_recs8) == 4 and all(np.array_equal(a, b) for a, b in zip(got_recs8, recs8))


def _frame(model, records, nodes, n_chains):
    """The restatement's frame: records [size][n_nodes, n_chains] -> chain-major rows of state numbers."""
    pos = {v: i for i, v in enumerate(nodes)}
    rec = np.stack(records)  # [size, n_nodes, n_chains]
    df = pd.DataFrame({v: rec[:, pos[v], :].T.reshape(-1).astype(np.int64) for v in model.nodes()}, columns=list(model.nodes()))
    if n_chains > 1:
        df["_chain"] = np.repeat(np.arange(n_chains, dtype=np.int64), len(records))
    return df


@pytest.mark.parametrize("n_chains", [1, 3])
def test_sample_frame(gpu, n_chains):
    """K5 / P1: sample(size=8) on hand_model() equals the restatement's frame, row 0 the start state; with
    n_chains = 3 the rows are chain-major with a _chain column; burn_in, thin and evidence likewise."""
    from pgmpy_amd.sampling import GibbsSampling, State

    m = S.hand_model()
    nodes, fams, tables, card = G.bn_factors(m)
    g = GibbsSampling(m)
    start = S.sample_ref(fams, tables, n_chains, seed=5)[0]
    _, recs, _, _ = G.gibbs_ref(fams, tables, card, start, 7, seed=5, thin=1)
    got = g.sample(size=8, seed=5, n_chains=n_chains)
    want = _frame(m, [start] + recs, nodes, n_chains)
    pd.testing.assert_frame_equal(got, want)
    assert list(got.columns)[:4] == list(m.nodes()) and got[list(m.nodes())].dtypes.eq(np.int64).all()
    # a given start state, for every chain
    state = {"A": 1, "B": 2, "C": 0, "D": 1}
    fixed = np.repeat(np.array([[state[v]] for v in nodes], dtype=np.uint8), n_chains, axis=1)
    _, recs, _, _ = G.gibbs_ref(fams, tables, card, fixed, 7, seed=6, thin=1)
    for given in (state, [State(v, s) for v, s in state.items()]):
        got = g.sample(start_state=given, size=8, seed=6, n_chains=n_chains)
        pd.testing.assert_frame_equal(got, _frame(m, [fixed] + recs, nodes, n_chains))
    assert (got.iloc[::8][list(m.nodes())].to_numpy() == [state[v] for v in m.nodes()]).all()
    # burn-in, thinning and evidence: rows after 3, 5, 7, 9 sweeps, D clamped at d2
    given = np.full((4, n_chains), 255, dtype=np.uint8)
    given[3] = 2
    modes = [S.GIVEN if cols[0] == 3 else S.FREE for cols, _ in fams]
    start = S.sample_ref(fams, tables, n_chains, seed=7, given=given, modes=modes)[0]
    _, recs, _, _ = G.gibbs_ref(fams, tables, card, start, 9, seed=7, clamp=[0, 0, 0, 1], thin=1)
    got = g.sample(size=4, seed=7, n_chains=n_chains, burn_in=3, thin=2, evidence=[("D", "d2")])
    pd.testing.assert_frame_equal(got, _frame(m, [recs[2], recs[4], recs[6], recs[8]], nodes, n_chains))
    assert (got["D"] == 2).all()
    # the generator yields the states after each sweep
    if n_chains == 1:
        _, recs, _, _ = G.gibbs_ref(fams, tables, card, fixed, 3, seed=6, thin=1)
        states = list(g.generate_sample(start_state=state, size=3, seed=6))
        pos = {v: i for i, v in enumerate(nodes)}
        assert states == [[State(v, int(r[pos[v], 0])) for v in m.nodes()] for r in recs]


def test_launches_are_split_invisibly(gpu, monkeypatch):
    """P1: a run longer than the launch bound is issued as several launches with the same result."""
    from pgmpy_amd.sampling import GibbsSampling
    from pgmpy_amd.sampling import gibbs as gibbs_module

    m = S.hand_model()
    g = GibbsSampling(m)
    whole, _ = g.sample_codes(70, 9, seed=3)
    frame = g.sample(size=5, seed=3, n_chains=4, thin=2, burn_in=1)
    monkeypatch.setattr(gibbs_module, "LAUNCH_UPDATES", 70 * 4 * 2)  # two sweeps per launch
    calls = []
    plan = gibbs_module.gibbs_compiled(m, True).plan
    sweep = plan.sweep
    monkeypatch.setattr(plan, "sweep", lambda *a, **k: (calls.append(a[2]), sweep(*a, **k))[1])
    parts, _ = g.sample_codes(70, 9, seed=3)
    assert calls == [2, 2, 2, 2, 1] and np.array_equal(_host(parts), _host(whole))
    monkeypatch.setattr(gibbs_module, "LAUNCH_UPDATES", 1)  # one sweep per launch: rounded up to thin
    pd.testing.assert_frame_equal(g.sample(size=5, seed=3, n_chains=4, thin=2, burn_in=1), frame)


# ---------------------------------------------------------------------------- K6: errors
def test_probability_zero_start_raises_value_error(gpu):
    """K6: a CPD with a zero entry: a start state of probability 0 leaves a conditional without a total.
    The call raises ValueError, the variable keeps its code and the walk goes on."""
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.models import DiscreteBayesianNetwork
    from pgmpy_amd.sampling import GibbsSampling

    factors = [([0], [2]), ([1, 0], [2, 2]), ([2, 1], [2, 2])]
    tables = [np.array([0.5, 0.5]), np.array([0.0, 0.0, 1.0, 1.0]), np.array([0.3, 0.6, 0.7, 0.4])]  # P(X1 = 0 | .) = 0
    start = np.array([[1, 0], [0, 1], [1, 1]], dtype=np.uint8)  # chain 0 holds X1 = 0
    want, _, undrawn, bad = G.gibbs_ref(factors, tables, [2, 2, 2], start, 1, seed=2)
    assert undrawn and not bad and want[0, 0] == 1 and want[1, 0] == 1
    got, _ = run_device(factors, tables, [2, 2, 2], start, 1, seed=2, raises=ValueError)
    assert np.array_equal(got, want)
    m = DiscreteBayesianNetwork([("X0", "X1"), ("X1", "X2")])
    m.add_cpds(TabularCPD("X0", 2, [[0.5], [0.5]]), TabularCPD("X1", 2, [[0.0, 0.0], [1.0, 1.0]], ["X0"], [2]),
               TabularCPD("X2", 2, [[0.3, 0.6], [0.7, 0.4]], ["X1"], [2]))
    with pytest.raises(ValueError, match="the start state has probability 0 under the model"):
        GibbsSampling(m).sample(start_state={"X0": 1, "X1": 0, "X2": 1}, size=3, seed=2)
    assert len(GibbsSampling(m).sample(start_state={"X0": 1, "X1": 1, "X2": 1}, size=3, seed=2)) == 3


def test_code_that_is_no_state_raises_index_error(gpu):
    """K6: a start code >= card, in a free or in a clamped column, raises IndexError; the chain is not
    advanced (nothing was indexed with the code) and the other chains are."""
    from pgmpy_amd.sampling import GibbsSampling

    _, nodes, fams, tables, card = alarm()
    start = np.array(alarm_start(1030)[:, :70])
    start[4, 9] = card[4]
    start[20, 33] = 255
    clamp = np.zeros(len(nodes), dtype=np.uint8)
    clamp[20] = 1
    want, _, undrawn, bad = G.gibbs_ref(fams, tables, card, start, 2, seed=11, clamp=clamp)
    assert bad and not undrawn and (want[:, 9] == start[:, 9]).all() and (want[:, 33] == start[:, 33]).all()
    got, _ = run_device(fams, tables, card, start, 2, seed=11, clamp=clamp, raises=IndexError)
    assert np.array_equal(got, want)
    m = S.hand_model()
    bad_start = np.zeros((4, 5), dtype=np.uint8)
    bad_start[1, 2] = 3
    with pytest.raises(IndexError, match="state code is >= its variable's cardinality"):
        GibbsSampling(m).sample_codes(5, 2, seed=1, start_codes=bad_start)
    with pytest.raises(IndexError):
        GibbsSampling(m).sample(start_state={"A": 0, "B": 3, "C": 0, "D": 0}, size=2, seed=1)


# ---------------------------------------------------------------------------- P2: a Markov network
def test_markov_network_codes_exact(gpu):
    """P2: a triangle with cardinalities 2, 3, 2: the start is floor(u * card) from the sweep-0 uniform, the
    codes after 5 sweeps equal the restatement's; evidence is written over the start and clamped."""
    from pgmpy_amd.sampling import GibbsSampling

    m = G.triangle_model()
    nodes, factors, tables, card = G.mn_factors(m)
    g = GibbsSampling(m)
    start = G.start_ref(card, 300, seed=9)
    assert all(set(start[c]) == set(range(card[c])) for c in range(3))
    got0, cols = g.sample_codes(300, 0, seed=9)
    assert cols == nodes == ["A", "B", "C"] and np.array_equal(_host(got0), start)
    got, _ = g.sample_codes(300, 5, seed=9)
    assert np.array_equal(_host(got), G.gibbs_ref(factors, tables, card, start, 5, seed=9)[0])
    start[1] = 2
    got, _ = g.sample_codes(300, 5, seed=9, evidence=[("B", 2)])
    assert np.array_equal(_host(got), G.gibbs_ref(factors, tables, card, start, 5, seed=9, clamp=[0, 1, 0])[0])
    frame = g.sample(size=4, seed=9)
    _, recs, _, _ = G.gibbs_ref(factors, tables, card, G.start_ref(card, 1, seed=9), 3, seed=9, thin=1)
    pd.testing.assert_frame_equal(frame, _frame(m, [G.start_ref(card, 1, seed=9)] + recs, nodes, 1))


# ---------------------------------------------------------------------------- D: the distribution
def test_posterior_with_evidence(gpu):
    """D1: hand_model() given D = d0, 8,192 chains after the burn-in computed from the exact 12-state sweep
    matrix (worst-start total variation below 1e-6): every cell of the joint over A, B, C within six sigma
    of the exact posterior.  tests/test_gibbs_cpu.py runs the restatement through the same check."""
    from pgmpy_amd.sampling import GibbsSampling

    nodes, fams, tables, card, joint, burn = G.hand_posterior()
    assert burn <= 64
    got, cols = GibbsSampling(S.hand_model()).sample_codes(G.N_DIST, burn, seed=G.SEED_DIST, evidence=[("D", "d0")])
    got = _host(got)
    assert cols == nodes and (got[3] == 0).all()
    worst = S.six_sigma_cells(got[:3], joint, G.N_DIST)
    print(f"burn-in {burn}, worst cell deviation {worst:.2f} sigma")
    assert worst <= 6.0


def test_triangle_distribution(gpu):
    """D2: the triangle network without evidence, likewise."""
    from pgmpy_amd.sampling import GibbsSampling

    nodes, factors, tables, card, joint, burn = G.triangle_posterior()
    assert burn <= 64
    got, _ = GibbsSampling(G.triangle_model()).sample_codes(G.N_DIST, burn, seed=G.SEED_DIST)
    worst = S.six_sigma_cells(_host(got), joint, G.N_DIST)
    print(f"burn-in {burn}, worst cell deviation {worst:.2f} sigma")
    assert worst <= 6.0


# ---------------------------------------------------------------------------- R: round trips
def test_sample_codes_then_count_on_the_device(gpu):
    """R1: sample_codes -> FitPlan.count without a host copy: the counts are np.bincount of the downloaded
    codes, and the codes are the restatement's."""
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.sampling import GibbsSampling

    m, nodes, fams, tables, card = alarm()
    n = 1030
    codes, cols = GibbsSampling(m).sample_codes(n, 3, seed=11)
    assert cols == nodes and codes.is_cuda and tuple(codes.shape) == (len(nodes), n)
    host = _host(codes)
    assert np.array_equal(host, alarm_ref(1030, 3))
    got = _host(FitPlan(fams).count(codes))
    want = []
    for fcols, cards in fams:
        idx = np.zeros(n, dtype=np.int64)
        for c, k in zip(fcols, cards):
            idx = idx * k + host[c]
        want.append(np.bincount(idx, minlength=int(np.prod(cards))))
    assert np.array_equal(got, np.concatenate(want))


def test_fit_then_gibbs_uses_the_new_cpds(gpu):
    """R2: fit leaves the CPDs on the device; GibbsSampling draws from them, and from the next fit's after
    that (the cache follows the model's change counter)."""
    from pgmpy_amd.models import DiscreteBayesianNetwork
    from pgmpy_amd.sampling import GibbsSampling

    m = S.hand_model()
    data = m.simulate(3000, seed=1)
    learner = DiscreteBayesianNetwork(list(m.edges()))
    seen = []
    for rows in (3000, 400):
        learner.fit(data.iloc[:rows])
        assert all(c._dev is not None for c in learner.cpds)
        got, cols = GibbsSampling(learner).sample_codes(257, 4, seed=2)
        nodes, fams, tables, card = G.bn_factors(learner)
        start = S.sample_ref(fams, tables, 257, seed=2)[0]
        assert cols == nodes and np.array_equal(_host(got), G.gibbs_ref(fams, tables, card, start, 4, seed=2)[0])
        seen.append(np.concatenate([t.ravel() for t in tables]))
    assert not np.array_equal(seen[0], seen[1])
