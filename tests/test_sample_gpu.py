"""Forward sampling on the device: the sampling kernel on every path (K1-K5), the running-sum kernel (K6),
the public API (P1-P4) and the round trip sample -> count -> fit -> sample (R1, R2).

The reference is tests/sample_cases.py's numpy restatement, which tests/test_sample_cpu.py pins to the
known answers of the generator, to the selection rule and to the distribution.  Codes are compared
exactly; weights against the long-double restatement at relative 2 * n_observed * 2^-53 (one division and
one multiplication per observed node, each rounded once).

One case of the issue cannot exist: a node with PGM_MAX_DIMS - 1 BINARY parents has 2^31 parent
configurations, past the 2^31 - 1 entries the fit plan's layout (which the sampler reuses) allows, and
its running sums alone would be 16 GiB.  tests/test_sample_cpu.py asserts that the plan rejects it; the
kernel is run here with PGM_MAX_DIMS - 1 parents of which 12 are binary and the rest have one state."""
import functools

import numpy as np
import pandas as pd
import pytest

from tests import sample_cases as S

pytestmark = pytest.mark.gpu

BLOCK_ROWS = 1024  # rows of one workgroup (pgm_sample_info_t.rows_per_block; asserted below)
SENTINEL = 0xAB
EPS = 2.0 ** -53


def _dev(a):
    from pgmpy_amd import engine as E

    return E.to_device_raw(np.ascontiguousarray(a))


def _host(t):
    from pgmpy_amd.inference.batch import download

    return download(t)


def _plan(fams):
    from pgmpy_amd.sampling._sample import SamplePlan

    plan = SamplePlan(fams)
    assert plan.info.rows_per_block == BLOCK_ROWS and plan.info.block == 256
    return plan


def run_device(fams, tables, n, ld=None, row0=0, first_row=0, seed=0, given=None, modes=None, explicit=None,
               weights=False, n_cols=None, expect_vec4=None, windows=None, raises=None):
    """The kernel over a sentinel-filled buffer: (codes [n_cols, n], weights [n] or None).  Asserts that
    nothing outside [row0, row0 + n) was written.  windows: [(begin, end)] row ranges drawn by one call
    each (default: one call)."""
    import torch

    plan = _plan(fams)
    n_cols = plan.n_cols if n_cols is None else n_cols
    ld = row0 + n if ld is None else ld
    values = _dev(np.concatenate([np.asarray(t, dtype=np.float64).ravel() for t in tables]))
    cdf = plan.cdf(values)
    buf = np.full((n_cols, ld), SENTINEL, dtype=np.uint8)
    if given is not None:
        buf[:, row0:row0 + n] = given
    codes = _dev(buf)
    uni = None
    if explicit is not None:
        ub = np.full((n_cols, ld), 0.5)
        ub[:, row0:row0 + n] = explicit
        uni = _dev(ub)
    w = torch.full((ld,), -7.0, dtype=torch.float64, device=codes.device) if weights else None
    if expect_vec4 is not None:
        assert plan.launch_info(codes.data_ptr(), ld, row0).vec4 == int(expect_vec4)
    err = None
    for a, b in (windows or [(0, n)]):
        try:
            plan.forward(cdf, codes, n_rows=b - a, row0=row0 + a, first_row=first_row + a, seed=seed, modes=modes,
                         values=values if weights else None, weights=w, uniforms=uni)
        except IndexError as e:
            err = e
    assert (err is not None) == bool(raises), err
    out = _host(codes)
    outside = np.ones(ld, dtype=bool)
    outside[row0:row0 + n] = False
    assert (out[:, outside] == SENTINEL).all(), "bytes outside the row window were written"
    wh = None
    if weights:
        wh = _host(w)
        assert (wh[outside] == -7.0).all()
        wh = wh[row0:row0 + n]
    return out[:, row0:row0 + n], wh


def assert_weights(got, want, n_observed):
    want = np.asarray(want, dtype=np.longdouble)
    err = np.abs(got.astype(np.longdouble) - want)
    bound = 2 * n_observed * EPS * np.abs(want)
    worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if len(want) else 0.0
    print(f"worst weight error / bound = {worst:.3f}")
    assert (err <= bound).all()


@functools.lru_cache(maxsize=None)
def alarm():
    from pgmpy_amd.utils import get_example_model

    m = get_example_model("alarm")
    return (m,) + S.model_plan(m)


@functools.lru_cache(maxsize=None)
def alarm_ref(n, first_row=0, seed=11):
    _, nodes, order, fams, tables = alarm()
    codes, _, _ = S.sample_ref(fams, tables, n, seed=seed, first_row=first_row, n_cols=len(nodes))
    codes.flags.writeable = False
    return codes


# ---------------------------------------------------------------------------- K1: geometry and alignment
ROW_COUNTS = [1, 3, 4, 5, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1, 2 * BLOCK_ROWS + 3]
GEOMETRY = {  # name: (row0, ld % 4, the four-rows-per-lane path)
    "aligned": (0, 0, True), "row0_4": (4, 0, True), "row0_1": (1, 0, False), "ld_odd": (0, 1, False),
    "row0_4_ld_3": (4, 3, False),
}


@pytest.mark.parametrize("geom", list(GEOMETRY))
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_alarm_codes_exact(gpu, n, geom):
    """K1: alarm's device codes equal the restatement's at every row count around the workgroup size, on
    aligned buffers (four rows per lane, with and without a tail) and misaligned ones (one row)."""
    _, nodes, _, fams, tables = alarm()
    row0, ld_mod, vec4 = GEOMETRY[geom]
    ld = (row0 + n + 8) // 4 * 4 + ld_mod
    got, _ = run_device(fams, tables, n, ld=ld, row0=row0, seed=11, n_cols=len(nodes), expect_vec4=vec4)
    want = alarm_ref(n)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("row0", [0, 1])
@pytest.mark.parametrize("first_row,n", [(12345, n) for n in ROW_COUNTS] + [(2 ** 32 - 2, 8)])
def test_stream_offset(gpu, first_row, n, row0):
    """K1: rows [first_row, first_row + n) of the stream, across the 2^32 boundary of the row counter."""
    _, nodes, _, fams, tables = alarm()
    got, _ = run_device(fams, tables, n, ld=(n + 7) // 4 * 4, row0=row0, first_row=first_row, seed=11, n_cols=len(nodes),
                        expect_vec4=row0 == 0)
    assert np.array_equal(got, alarm_ref(n, first_row))
    if first_row == 12345:  # the same rows as a window of a longer draw from row 0
        m = min(n, 64)
        assert np.array_equal(got[:, :m], alarm_ref(12345 + 64)[:, 12345:12345 + m])


@pytest.mark.parametrize("n,k", [(n, n // 2) for n in ROW_COUNTS] + [(2 * BLOCK_ROWS + 3, k) for k in (BLOCK_ROWS, BLOCK_ROWS + 6, 7)])
def test_one_call_equals_two(gpu, n, k):
    """K1: [0, n) in one call equals [0, k) and [k, n) drawn into the same buffer by two calls (the
    second one starts on a dword boundary or not)."""
    _, nodes, _, fams, tables = alarm()
    got, _ = run_device(fams, tables, n, ld=(n + 4) // 4 * 4, seed=11, n_cols=len(nodes), windows=[(0, k), (k, n)])
    assert np.array_equal(got, alarm_ref(n))


# ---------------------------------------------------------------------------- K2: synthetic plans
def _random_tables(fams, rng, zeros=0.0):
    tables = []
    for cols, cards in fams:
        t = rng.random((cards[0], int(np.prod(cards[1:])))) + 0.05
        if zeros:
            t[rng.random(t.shape) < zeros] = 0.0
            t[0, t.sum(axis=0) == 0] = 1.0
        tables.append(t / t.sum(axis=0, keepdims=True))
    return tables


def _synthetic(name):
    rng = np.random.default_rng(7)
    if name == "max_parents":  # 31 parents: 12 binary, 19 with one state (module docstring)
        cards = [2] * 12 + [1] * 19
        order = rng.permutation(31)
        fams = [([int(v)], [cards[v]]) for v in range(31)]
        fams.append(([31] + [int(v) for v in order], [3] + [cards[v] for v in order]))
        return fams, 1029
    if name == "card_255":
        return [([1], [3]), ([0, 1], [255, 3]), ([2, 0], [2, 255])], 2 * BLOCK_ROWS + 1
    if name == "card_1":
        return [([0], [1]), ([1, 0], [4, 1]), ([2, 1, 0], [1, 4, 1]), ([3, 2], [3, 1])], 261
    if name == "chain_300":  # every node reads the code the lane stored one step before
        cards = [int(k) for k in rng.integers(2, 5, size=300)]
        cols = [int(c) for c in rng.permutation(300)]
        fams = [([cols[0]], [cards[0]])]
        fams += [([cols[i], cols[i - 1]], [cards[i], cards[i - 1]]) for i in range(1, 300)]
        return fams, BLOCK_ROWS + 5
    raise KeyError(name)


@pytest.mark.parametrize("row0", [0, 3], ids=["four_rows", "one_row"])
@pytest.mark.parametrize("name", ["max_parents", "card_255", "card_1", "chain_300"])
def test_synthetic_plans_exact(gpu, name, row0):
    """K2: the most parents a family may have, 255 states, a single state, and a chain of 300 dependent nodes."""
    fams, n = _synthetic(name)
    tables = _random_tables(fams, np.random.default_rng(1), zeros=0.2 if name == "card_255" else 0.0)
    got, _ = run_device(fams, tables, n, ld=(n + row0 + 7) // 4 * 4, row0=row0, seed=99, first_row=5,
                        expect_vec4=row0 == 0)
    want, _, _ = S.sample_ref(fams, tables, n, seed=99, first_row=5)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    if name == "card_255":
        assert len(np.unique(got[0])) > 100  # far more states than any other case has


# ---------------------------------------------------------------------------- K3: explicit uniforms
@pytest.mark.parametrize("row0", [0, 1], ids=["four_rows", "one_row"])
@pytest.mark.parametrize("name,p", S.BOUNDARY_COLUMNS, ids=[c[0] for c in S.BOUNDARY_COLUMNS])
def test_boundaries_with_explicit_uniforms(gpu, name, p, row0):
    """K3: u at, just below and just above every boundary of the running sums, 0 and 1 - 2^-53."""
    us = S.boundary_uniforms(p)
    us = np.concatenate([us, np.full(-len(us) % 4 + 4, 0.5)])
    n = len(us)
    fams, tables = [([0], [len(p)])], [np.array(p, dtype=np.float64).reshape(-1, 1)]
    got, _ = run_device(fams, tables, n, ld=n + 4, row0=row0, explicit=us[None, :], expect_vec4=row0 == 0)
    want = [S.expected_state(p, u) for u in us]
    assert got[0].tolist() == want
    assert all(p[s] > 0 for s in got[0])


def test_explicit_uniforms_per_column(gpu):
    """K3: the uniform matrix has the layout of the codes: column c of the matrix drives code column c."""
    rng = np.random.default_rng(5)
    fams = [([2], [3]), ([0, 2], [4, 3]), ([1, 0, 2], [5, 4, 3])]
    tables = _random_tables(fams, rng, zeros=0.3)
    n = 517
    u = rng.random((3, n))
    for row0 in (0, 2):
        got, _ = run_device(fams, tables, n, ld=n + 7, row0=row0, explicit=u)
        want, _, _ = S.sample_ref(fams, tables, n, explicit=u)
        assert np.array_equal(got, want)


# ---------------------------------------------------------------------------- K4: modes and weights
def _alarm_modes(kind, n, rng):
    _, nodes, order, fams, tables = alarm()
    col = {v: i for i, v in enumerate(nodes)}
    picked = ["HYPOVOLEMIA", "CATECHOL", "HR", "BP", "VENTLUNG"]  # roots, inner nodes and a leaf
    given = np.full((len(nodes), n), S.MISSING, dtype=np.uint8)
    base = alarm_ref(n, seed=23)
    modes = [S.FREE] * len(order)
    for v in picked:
        card = fams[order.index(v)][1][0]
        given[col[v]] = rng.integers(0, card, size=n) if "rows" in kind else rng.integers(0, card)
        if "missing" in kind:
            given[col[v], rng.random(n) < 0.3] = S.MISSING
        modes[order.index(v)] = S.OBSERVED if "observed" in kind else S.GIVEN
    return given, modes, len(picked), base


@pytest.mark.parametrize("row0", [0, 1], ids=["four_rows", "one_row"])
@pytest.mark.parametrize("kind", ["given_constants", "given_rows_missing", "observed_constants",
                                  "observed_rows_missing"])
def test_modes_and_weights(gpu, kind, row0):
    """K4: GIVEN and OBSERVED columns (constants, per-row codes, some rows PGM_EV_MISSING and so drawn)."""
    _, nodes, order, fams, tables = alarm()
    n = BLOCK_ROWS + 5
    given, modes, n_obs, _ = _alarm_modes(kind, n, np.random.default_rng(3))
    weighted = "observed" in kind
    got, w = run_device(fams, tables, n, ld=n + 7, row0=row0, seed=23, given=given, modes=modes, weights=weighted,
                        n_cols=len(nodes))
    want, ww, bad = S.sample_ref(fams, tables, n, seed=23, given=given, modes=modes, weights=weighted, n_cols=len(nodes))
    assert not bad and np.array_equal(got, want)
    keep = given != S.MISSING
    assert np.array_equal(got[keep], given[keep])
    if weighted:
        assert_weights(w, ww, n_obs)
        assert (w > 0).all() and (w < 1).any()
    else:  # a GIVEN column draws no weight: the unweighted launch of the same modes gives the same codes
        got2, w2 = run_device(fams, tables, n, ld=n + 7, row0=row0, seed=23, given=given, modes=modes, weights=True,
                              n_cols=len(nodes))
        assert np.array_equal(got2, got) and (w2 == 1.0).all()


# ---------------------------------------------------------------------------- K5: guards
@pytest.mark.parametrize("row0", [0, 1], ids=["four_rows", "one_row"])
def test_bad_given_code_is_index_error(gpu, row0):
    """K5: a given code that is neither a state nor 255 raises IndexError; the nodes after it in plan
    order are 255 in that row, its weight is 0, and every other row is what it is without the bad code."""
    _, nodes, order, fams, tables = alarm()
    n = BLOCK_ROWS + 5
    given, modes, n_obs, _ = _alarm_modes("observed_rows_missing", n, np.random.default_rng(4))
    col = {v: i for i, v in enumerate(nodes)}
    clean, wc, _ = S.sample_ref(fams, tables, n, seed=23, given=given, modes=modes, weights=True, n_cols=len(nodes))
    bad_rows = {0: "HR", 6: "HYPOVOLEMIA", n - 1: "VENTLUNG"}
    for r, v in bad_rows.items():
        given[col[v], r] = fams[order.index(v)][1][0]  # == the cardinality
    given[col["BP"], 6] = 254
    got, w = run_device(fams, tables, n, ld=n + 7, row0=row0, seed=23, given=given, modes=modes, weights=True,
                        n_cols=len(nodes), raises=True)
    want, ww, bad = S.sample_ref(fams, tables, n, seed=23, given=given, modes=modes, weights=True, n_cols=len(nodes))
    assert bad and np.array_equal(got, want)
    others = np.setdiff1d(np.arange(n), list(bad_rows))
    assert np.array_equal(got[:, others], clean[:, others])
    assert_weights(w[others], wc[others], n_obs)
    for r, v in bad_rows.items():
        f = order.index(v)
        after = [col[u] for u in order[f + 1:]]
        assert got[col[v], r] == given[col[v], r] and (got[after, r] == S.MISSING).all() and w[r] == 0.0
        before = [col[u] for u in order[:f]]
        assert (got[before, r] != S.MISSING).all()


# ---------------------------------------------------------------------------- K6: running sums
def test_cdf_exact_and_rejected(gpu):
    """K6: pgm_sample_cdf equals numpy's cumsum over the states, exactly; a column of zeros, a NaN, an
    infinity or a negative total raise ValueError."""
    _, nodes, order, fams, tables = alarm()
    plan = _plan(fams)
    flat = np.concatenate([t.ravel() for t in tables])
    got = _host(plan.cdf(_dev(flat)))
    for f, t in enumerate(tables):
        want = np.cumsum(t, axis=0)
        assert np.array_equal(plan.table(got, f), want) and np.array_equal(want, S.running_sums(t))
    big = max(range(len(tables)), key=lambda f: tables[f].shape[1])
    for bad in ("zeros", "nan", "inf", "negative"):
        v = flat.copy()
        column = plan.table(v, big)[:, tables[big].shape[1] - 1]
        column[:] = {"zeros": 0.0, "nan": column, "inf": column, "negative": -column}[bad]
        if bad in ("nan", "inf"):
            column[1] = {"nan": np.nan, "inf": np.inf}[bad]
        with pytest.raises(ValueError, match="total is not finite or not > 0"):
            plan.cdf(_dev(v))
    fams3, t3 = [([0], [3])], [np.array([[1.5], [0.75], [0.75]])]
    assert _host(_plan(fams3).cdf(_dev(t3[0].ravel()))).tolist() == [1.5, 2.25, 3.0]


# ---------------------------------------------------------------------------- P: the public API
def _codes_of(model, frame, nodes):
    states = model.states
    return np.stack([np.array([states[v].index(s) for s in frame[v].astype(object)], dtype=np.int64) for v in nodes])


def _same_frame(got, want):
    assert list(got.columns) == list(want.columns) and len(got) == len(want)
    for c in want.columns:
        a, b = got[c].astype(object).to_numpy(), want[c].astype(object).to_numpy()
        same = (a == b) | (pd.isna(a) & pd.isna(b))
        assert same.all(), (c, np.nonzero(~same)[0][:8])


def test_forward_sample_and_simulate_equal_the_restatement(gpu):
    """P1: forward_sample(seed) and simulate(seed) are the frame of the restatement's codes."""
    from pgmpy_amd.sampling import BayesianModelSampling

    m, nodes, order, fams, tables = alarm()
    n = 203
    want = S.frame_of(m, alarm_ref(n, seed=42), nodes)
    got = BayesianModelSampling(m).forward_sample(size=n, seed=42, show_progress=False)
    _same_frame(got, want)
    assert list(got.columns) == list(m.nodes())
    sim = m.simulate(n_samples=n, seed=42, show_progress=False)
    assert all(isinstance(t, pd.CategoricalDtype) for t in sim.dtypes)
    _same_frame(sim, want)
    codes, cols = BayesianModelSampling(m).forward_sample_codes(n, seed=42)
    assert cols == nodes and np.array_equal(_host(codes), alarm_ref(n, seed=42))
    a = BayesianModelSampling(m).forward_sample(size=5)  # fresh entropy
    b = BayesianModelSampling(m).forward_sample(size=5)
    assert not a.equals(b)


def test_likelihood_weighted_sample_equals_the_restatement(gpu):
    """P1: likelihood_weighted_sample: the evidence columns are constant, `_weight` is their likelihood."""
    from pgmpy_amd.sampling import BayesianModelSampling, State

    m, nodes, order, fams, tables = alarm()
    n = 301
    ev = [State("HR", "HIGH"), State("BP", "LOW"), State("HYPOVOLEMIA", "TRUE")]
    col = {v: i for i, v in enumerate(nodes)}
    given = np.full((len(nodes), n), S.MISSING, dtype=np.uint8)
    modes = [S.FREE] * len(order)
    for v, s in ev:
        given[col[v]] = m.states[v].index(s)
        modes[order.index(v)] = S.OBSERVED
    codes, w, _ = S.sample_ref(fams, tables, n, seed=8, given=given, modes=modes, weights=True, n_cols=len(nodes))
    got = BayesianModelSampling(m).likelihood_weighted_sample(evidence=ev, size=n, seed=8)
    assert list(got.columns) == list(m.nodes()) + ["_weight"]
    _same_frame(got.drop(columns="_weight"), S.frame_of(m, codes, nodes))
    assert_weights(got["_weight"].to_numpy(), w, len(ev))
    assert (got["HR"] == "HIGH").all() and got["_weight"].nunique() > 1


@pytest.mark.parametrize("size", [3, 1000])
def test_rejection_sample_is_the_first_accepted_rows_of_the_stream(gpu, size):
    """P2: evidence of probability 0.12: the result is the first `size` rows of the stream that match,
    whatever the batch sizes were."""
    from pgmpy_amd.sampling import BayesianModelSampling, State

    m = S.hand_model()
    nodes, order, fams, tables = S.model_plan(m)
    stream, _, _ = S.sample_ref(fams, tables, 20000, seed=77)
    ok = (stream[0] == 1) & (stream[1] == 1)
    assert ok.sum() >= 1000 and abs(ok.mean() - 0.12) < 0.02
    want = S.frame_of(m, stream[:, ok][:, :size], nodes)
    s = BayesianModelSampling(m)
    got = s.rejection_sample(evidence=[State("A", "a1"), State("B", "b1")], size=size, seed=77, show_progress=False)
    _same_frame(got, want)
    assert got.index.tolist() == list(range(size))
    sim = m.simulate(n_samples=size, evidence={"A": "a1", "B": "b1"}, seed=77)
    _same_frame(sim, want)


def test_rejection_sample_gives_up_on_impossible_evidence(gpu):
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.models import DiscreteBayesianNetwork
    from pgmpy_amd.sampling import BayesianModelSampling, State

    m = DiscreteBayesianNetwork([("X", "Y")])
    m.add_cpds(TabularCPD("X", 2, [[1.0], [0.0]]), TabularCPD("Y", 2, [[0.5, 0.5], [0.5, 0.5]], ["X"], [2]))
    with pytest.raises(ValueError, match="no row matched the evidence in 64 consecutive batches"):
        BayesianModelSampling(m).rejection_sample(evidence=[State("X", 1)], size=2, seed=1)


def test_partial_samples_and_latents(gpu):
    """P3: partial_samples columns are taken as given by state name (NaN: drawn); latents are dropped
    unless asked for."""
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.models import DiscreteBayesianNetwork
    from pgmpy_amd.sampling import BayesianModelSampling

    m = S.hand_model()
    nodes, order, fams, tables = S.model_plan(m)
    n = 130
    rng = np.random.default_rng(2)
    b = rng.integers(0, 3, size=n)
    c = rng.integers(0, 2, size=n)
    partial = pd.DataFrame({"C": np.array(["c0", "c1"], dtype=object)[c], "B": np.array(["b0", "b1", "b2"], dtype=object)[b]})
    partial.loc[::5, "B"] = np.nan
    given = np.full((4, n), S.MISSING, dtype=np.uint8)
    given[1], given[2] = b, c
    given[1, ::5] = S.MISSING
    modes = [S.GIVEN if v in ("B", "C") else S.FREE for v in order]
    want, _, _ = S.sample_ref(fams, tables, n, seed=9, given=given, modes=modes)
    got = BayesianModelSampling(m).forward_sample(size=n, seed=9, partial_samples=partial)
    _same_frame(got, S.frame_of(m, want, nodes))
    _same_frame(m.simulate(n, seed=9, partial_samples=partial), S.frame_of(m, want, nodes))
    assert (got["C"].to_numpy() == partial["C"].to_numpy()).all()

    lm = DiscreteBayesianNetwork([("L", "X"), ("X", "Y")], latents={"L"})
    lm.add_cpds(TabularCPD("L", 2, [[0.5], [0.5]]), TabularCPD("X", 2, [[0.9, 0.2], [0.1, 0.8]], ["L"], [2]),
                TabularCPD("Y", 3, [[0.2, 0.1], [0.3, 0.1], [0.5, 0.8]], ["X"], [2]))
    lnodes, lorder, lfams, ltables = S.model_plan(lm)
    lwant, _, _ = S.sample_ref(lfams, ltables, 64, seed=4)
    full = S.frame_of(lm, lwant, lnodes)
    _same_frame(BayesianModelSampling(lm).forward_sample(64, seed=4, include_latents=True), full)
    _same_frame(BayesianModelSampling(lm).forward_sample(64, seed=4), full[["X", "Y"]])
    _same_frame(lm.simulate(64, seed=4, include_latents=True), full)
    _same_frame(lm.simulate(64, seed=4), full[["X", "Y"]])


def _augmented(base, extra_cpds):
    """`base` plus one node per CPD (edges from its parents): the model simulate builds, built here."""
    from pgmpy_amd.models import DiscreteBayesianNetwork

    m = DiscreteBayesianNetwork()
    m.add_nodes_from(base.nodes())
    m.add_edges_from(base.edges())
    for cpd in extra_cpds:
        m.add_node(cpd.variable)
        m.add_edges_from([(p, cpd.variable) for p in cpd.variables[1:]])
    m.add_cpds(*[c.copy() for c in base.cpds], *extra_cpds)
    return m, sorted(base.nodes()) + [c.variable for c in extra_cpds]


def test_missing_prob(gpu):
    """P3: a `var*` node is drawn from the CPD given (here depending on C and on A itself) in a column
    after the model's own; `var` is blanked where it drew 1 and `var_full` keeps the drawn value."""
    from pgmpy_amd.factors.discrete import TabularCPD

    m = S.hand_model()
    miss = [TabularCPD("A*", 2, [[0.9, 0.3, 0.6, 0.5], [0.1, 0.7, 0.4, 0.5]], ["C", "A"], [2, 2],
                       state_names={"A*": [0, 1], "C": ["c0", "c1"], "A": ["a0", "a1"]}),
            TabularCPD("D*", 2, [[0.75], [0.25]])]
    aug, columns = _augmented(m, miss)
    nodes, order, fams, tables = S.model_plan(aug, nodes=columns)
    n = 400
    codes, _, _ = S.sample_ref(fams, tables, n, seed=31)
    assert np.array_equal(codes[:4], S.sample_ref(*S.model_plan(m)[2:], n, seed=31)[0])  # the model's own columns
    full = S.frame_of(aug, codes, nodes, columns=list(m.nodes()))
    want = full.copy()
    want["A_full"], want["D_full"] = full["A"], full["D"]
    want.loc[codes[4] == 1, "A"] = np.nan
    want.loc[codes[5] == 1, "D"] = np.nan
    got = m.simulate(n, missing_prob=miss, seed=31, return_full=True)
    _same_frame(got, want)
    assert 0 < got["A"].isna().sum() < n and 0 < got["D"].isna().sum() < n
    _same_frame(m.simulate(n, missing_prob=miss, seed=31), want[list(m.nodes())])
    _same_frame(m.simulate(n, missing_prob=miss[1], seed=31)[["A", "B", "C"]], full[["A", "B", "C"]])


N_STAT = 2 ** 16


def test_do(gpu):
    """P3 + P4: do={C: c1} is a GIVEN constant on the mutilated graph: exact against the restatement, and
    the empirical distribution of (A, B, D) is P(A) P(B) P(D | c1) at 6 sigma."""
    m = S.hand_model()
    cut = m.do(["C"])
    assert sorted(cut.edges()) == [("C", "D")] and sorted(m.edges()) == [("A", "C"), ("B", "C"), ("C", "D")]
    assert cut.get_cpds("C").variables == ["C"] and m.get_cpds("C").variables == ["C", "A", "B"]
    np.testing.assert_allclose(np.asarray(cut.get_cpds("C").values), np.asarray(m.get_cpds("C").values).sum(axis=(1, 2)) / 6,
                               rtol=1e-12)
    nodes, order, fams, tables = S.model_plan(cut)
    given = np.full((4, N_STAT), S.MISSING, dtype=np.uint8)
    given[2] = 1
    modes = [S.GIVEN if v == "C" else S.FREE for v in order]
    want, _, _ = S.sample_ref(fams, tables, N_STAT, seed=13, given=given, modes=modes)
    got = m.simulate(N_STAT, do={"C": "c1"}, seed=13)
    _same_frame(got, S.frame_of(cut, want, nodes, columns=list(m.nodes())))
    assert (got["C"] == "c1").all()
    joint = S.joint_of(*S.model_plan(m)[2:], (2, 3, 2, 3))
    pa, pb = joint.sum(axis=(1, 2, 3)), joint.sum(axis=(0, 2, 3))
    pd_c1 = np.asarray(m.get_cpds("D").values)[:, 1]
    target = np.zeros((2, 3, 2, 3))
    target[:, :, 1, :] = pa[:, None, None] * pb[None, :, None] * pd_c1[None, None, :]
    codes = _codes_of(m, got, nodes)
    cells = target > 0
    counts = np.bincount(np.ravel_multi_index(tuple(codes), target.shape), minlength=target.size).reshape(target.shape)
    dev = np.abs(counts - N_STAT * target)[cells] / np.sqrt(N_STAT * target * (1 - target))[cells]
    print(f"do: worst cell deviation {dev.max():.2f} sigma")
    assert dev.max() <= 6.0 and counts[~cells].sum() == 0


@pytest.mark.parametrize("kind", ["virtual_evidence", "virtual_intervention"])
def test_virtual_evidence_and_intervention(gpu, kind):
    """P3 + P4: a binary child `__var` with CPD [v; 1 - v] held at 0 (rejection): exact against the
    restatement of the rewritten model; for virtual evidence the empirical distribution is the posterior
    P(x) v[x_var] / Z at 6 sigma."""
    from pgmpy_amd.factors.discrete import TabularCPD

    m = S.hand_model()
    var, v = ("A", [0.8, 0.2]) if kind == "virtual_evidence" else ("C", [0.3, 0.7])
    names = m.states[var]
    virt = TabularCPD(var, 2, [[v[0]], [v[1]]], state_names={var: names})
    base = m if kind == "virtual_evidence" else m.do([var])
    child = TabularCPD("__" + var, 2, [v, [1 - v[0], 1 - v[1]]], [var], [2], state_names={"__" + var: [0, 1], var: names})
    aug, columns = _augmented(base, [child])
    nodes, order, fams, tables = S.model_plan(aug, nodes=columns)
    stream, _, _ = S.sample_ref(fams, tables, 4 * N_STAT, seed=21)
    ok = stream[4] == 0
    assert ok.sum() >= N_STAT
    want = S.frame_of(aug, stream[:, ok][:, :N_STAT], nodes, columns=list(m.nodes()) + ["__" + var])
    got = m.simulate(N_STAT, seed=21, **{kind: [virt]})
    _same_frame(got, want)
    assert (got["__" + var] == 0).all()
    joint = S.joint_of(*S.model_plan(base)[2:], (2, 3, 2, 3))
    shape = [1, 1, 1, 1]
    shape[nodes.index(var)] = 2
    target = joint * np.asarray(v).reshape(shape)
    target /= target.sum()
    worst = S.six_sigma_cells(_codes_of(m, got, nodes[:4]), target, N_STAT)
    print(f"{kind}: worst cell deviation {worst:.2f} sigma")
    assert target.min() > 0.001 and worst <= 6.0


# ---------------------------------------------------------------------------- R: round trips
def test_sample_then_count_on_the_device(gpu):
    """R1: forward_sample_codes -> FitPlan.count without a host copy: the counts are np.bincount of the
    restatement's codes, exactly."""
    from pgmpy_amd.estimators._fit import FitPlan
    from pgmpy_amd.sampling import BayesianModelSampling

    m, nodes, order, fams, tables = alarm()
    n = 4 * BLOCK_ROWS + 4
    codes, cols = BayesianModelSampling(m).forward_sample_codes(n, seed=11)
    assert cols == nodes and codes.is_cuda and tuple(codes.shape) == (len(nodes), n)
    col = {v: i for i, v in enumerate(nodes)}
    count_fams = []
    for v in nodes:
        scope = [v] + sorted(m.get_parents(v))
        count_fams.append(([col[u] for u in scope], [len(m.states[u]) for u in scope]))
    got = _host(FitPlan(count_fams).count(codes))
    ref = alarm_ref(n)
    want = []
    for fcols, cards in count_fams:
        idx = np.zeros(n, dtype=np.int64)
        for c, k in zip(fcols, cards):
            idx = idx * k + ref[c]
        want.append(np.bincount(idx, minlength=int(np.prod(cards))))
    assert np.array_equal(got, np.concatenate(want))


def test_fit_then_simulate_uses_the_new_cpds(gpu):
    """R2: fit on a simulated frame leaves the CPDs on the device; simulate draws from them, and from
    the next fit's after that (the sampler's cache follows the model's change counter)."""
    from pgmpy_amd.models import DiscreteBayesianNetwork

    m = S.hand_model()
    data = m.simulate(3000, seed=1)
    learner = DiscreteBayesianNetwork(list(m.edges()))
    seen = []
    for rows in (3000, 400):
        learner.fit(data.iloc[:rows])
        assert all(c._dev is not None for c in learner.cpds)
        got = learner.simulate(257, seed=2)
        nodes, order, fams, tables = S.model_plan(learner)
        want, _, _ = S.sample_ref(fams, tables, 257, seed=2)
        _same_frame(got, S.frame_of(learner, want, nodes))
        seen.append(np.concatenate([t.ravel() for t in tables]))
    assert not np.array_equal(seen[0], seen[1])
    np.testing.assert_allclose(seen[0][:2], [0.6, 0.4], atol=0.05)
