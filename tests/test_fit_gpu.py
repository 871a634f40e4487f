"""Parameter learning on the device: the family-count kernel (G1-G3), the finishing kernel (G4), the
public API against the reference's goldens (G5) and fit -> predict cache invalidation (G6).

The references are tests/fit_cases.py's numpy restatement (which tests/test_fit_cpu.py pins to the
goldens) and the goldens themselves (tests/golden/fit_cases.json, fit_alarm.npz)."""
import numpy as np
import pandas as pd
import pytest

from tests import fit_cases as F

pytestmark = pytest.mark.gpu

TILE, ROWS_PER_BLOCK = 4096, 4096
KCASES = {c["name"]: c for c in F.kernel_cases(TILE, ROWS_PER_BLOCK)}
CASES, ALARM = F.load_golden()
RUNS = F.golden_runs(CASES)
LD = F.LD


def _dev(a):
    from pgmpy_amd import engine as E

    return E.to_device_raw(np.ascontiguousarray(a))


def _host(t):
    from pgmpy_amd.inference.batch import download

    return download(t)


def _plan(families):
    from pgmpy_amd.estimators._fit import FitPlan

    plan = FitPlan(families)
    assert (plan.info.tile_bins, plan.info.rows_per_block) == (TILE, ROWS_PER_BLOCK)  # the cases' geometry
    return plan


# ---------------------------------------------------------------------------- G1
@pytest.mark.parametrize("name", list(KCASES))
def test_counts_exact(gpu, name):
    """G1: the device count tables are the restatement's integers, and two runs give identical tables."""
    c = KCASES[name]
    plan = _plan(c["families"])
    assert (plan.offsets, plan.sizes, plan.strides) == F.layout(c["families"])
    codes = _dev(c["codes"])
    want = F.count_ref(c["codes"], c["families"], row0=c["row0"], n_rows=c["n_rows"])
    got = _host(plan.count(codes, n_rows=c["n_rows"], row0=c["row0"]))
    again = _host(plan.count(codes, n_rows=c["n_rows"], row0=c["row0"]))
    assert got.dtype == np.int64 and np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert np.array_equal(again, got)
    if name in ("tile_plus_1", "tile_plus_1_ld4", "max_parents_global", "one_bin_global"):
        assert max(plan.sizes) > TILE  # these run the global path
    if name == "missing_all":
        assert not got.any()


def test_count_accumulates_over_row_windows(gpu):
    """pgm_fit_count adds to the tables: two windows counted into one buffer equal the whole."""
    c = KCASES[f"rows_{3 * ROWS_PER_BLOCK + 77}"]
    plan, codes = _plan(c["families"]), _dev(c["codes"])
    cut = ROWS_PER_BLOCK + 19
    t = plan.count(codes, n_rows=cut, row0=0)
    t = plan.count(codes, n_rows=c["n_rows"] - cut, row0=cut, tables=t)
    assert np.array_equal(_host(t), F.count_ref(c["codes"], c["families"]))


# ---------------------------------------------------------------------------- G2
@pytest.mark.parametrize("extra", [10, 12], ids=["one_row_kernel", "four_row_kernel"])
@pytest.mark.parametrize("path", ["lds", "global"])
def test_bad_code_is_index_error_and_stays_inside_the_tables(gpu, path, extra):
    """G2: a code equal to the cardinality, in row 0 and in the last row, raises IndexError; the rows
    are skipped for the families that read it and the sentinel-filled memory around the tables is
    untouched."""
    import torch

    rng = np.random.default_rng(3)
    n = ROWS_PER_BLOCK + extra  # + 12: a multiple of 4, the four-rows-per-lane kernel
    if path == "lds":
        fams, bad_col = F.MIXED, 5  # card 6, read by the last family only
        codes = F._random_codes(rng, 6, n, F._col_cards(fams, 6))
        codes[5, 0] = 6
        codes[2, n - 1] = 4  # card 4: read by families 2 and 3
    else:
        fams = [([0, 1], [17, 241]), ([1], [241])]
        codes = F._random_codes(rng, 2, n, [17, 241])
        codes[1, 0] = 241  # 16 * 241 + 241 would be the first bin past the table
        codes[0, 0] = 16
        codes[1, n - 1] = 254
    plan = _plan(fams)
    pad, sentinel = 1024, -0x0123456789ABCDEF
    buf = torch.full((plan.total_bins + 2 * pad,), sentinel, dtype=torch.int64, device=gpu)
    tables = buf[pad:pad + plan.total_bins]
    tables.zero_()
    with pytest.raises(IndexError):
        plan.count(_dev(codes), tables=tables)
    got = _host(buf)
    assert (got[:pad] == sentinel).all() and (got[pad + plan.total_bins:] == sentinel).all()
    assert np.array_equal(got[pad:pad + plan.total_bins], F.count_ref(codes, fams, bad="skip"))
    with pytest.raises(IndexError):
        F.count_ref(codes, fams)
    # the flag is per call: a clean call on the same plan succeeds afterwards
    codes[:, 0] = 0
    codes[:, n - 1] = 0
    assert np.array_equal(_host(plan.count(_dev(codes))), F.count_ref(codes, fams))


# ---------------------------------------------------------------------------- G3
@pytest.mark.parametrize("weights", ["signed", "signed_and_denormal", "denormal_only"])
def test_weighted_counts_within_summation_bound(gpu, weights):
    """G3: per bin |got - ref| <= (n + 2) * 2^-53 * sum |w| against a long-double sum, n the rows
    added to the bin (the any-order summation bound of tests/test_kernel_paths_gpu.py): LDS and global
    families, missing codes, signed and denormal weights.  Sums of denormals alone are exact."""
    rng = np.random.default_rng(17)
    fams = F.MIXED + [([6, 7], [17, 241])]
    n = 2 * ROWS_PER_BLOCK + 100 + (weights == "signed")  # + 1: odd ld, the one-row kernel; else four rows per lane
    codes = F._random_codes(rng, 8, n, F._col_cards(fams, 8), missing=0.05)
    tiny = np.float64(5e-324)
    if weights == "signed":
        w = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    elif weights == "signed_and_denormal":
        w = rng.standard_normal(n)
        sub = rng.random(n) < 0.5
        w[sub] = tiny * rng.integers(-(2 ** 40), 2 ** 40, int(sub.sum()))
    else:
        w = tiny * rng.integers(-(2 ** 30), 2 ** 30, n).astype(np.float64)
    assert weights == "signed" or (np.abs(w[w != 0]) < np.finfo(np.float64).tiny).any()
    plan = _plan(fams)
    got = _host(plan.count(_dev(codes), weights=_dev(w)))
    assert got.dtype == np.float64
    ref, n_add, mag = F.count_ref(codes, fams, weights=w)
    err = np.abs(got.astype(LD) - ref)
    bound = (n_add + 2) * LD(2.0) ** -53 * mag
    ratio = float(np.max(err / np.where(bound > 0, bound, 1), initial=0.0))
    print(f"{weights}: worst |got - ref| / bound = {ratio:.3f} over {int((n_add > 0).sum())} bins")
    assert not (err > bound).any(), f"{int((err > bound).sum())} bins beyond the summation bound (worst {ratio:.3f})"
    assert not got[n_add == 0].any()
    if weights == "denormal_only":
        assert np.array_equal(got, ref.astype(np.float64))


# ---------------------------------------------------------------------------- G4
FINISH_FAMILIES = [([0, 1], [3, 4]), ([2], [1]), ([2, 0], [1, 3]), ([1, 0, 2], [4, 3, 1]), ([3], [254]),
                   ([4, 3], [2, 254])]


def _finish_counts(rng):
    offsets, sizes, _ = F.layout(FINISH_FAMILIES)
    counts = rng.integers(0, 50, offsets[-1] + sizes[-1]).astype(np.int64)
    t = counts[:12].reshape(3, 4)
    t[:, 1] = 0                    # an unseen parent configuration
    t[:, 2] = [2 ** 31, 1, 2 ** 31 - 1]  # counts up to 2^31
    counts[offsets[3]:offsets[3] + 12].reshape(4, 3)[:, 0] = 0
    counts[offsets[5]:offsets[5] + 2 * 254].reshape(2, 254)[:, ::7] = 0
    return counts


@pytest.mark.parametrize("mode", ["mle", "bayes", "bayes_zero_prior", "mle_weighted", "bayes_weighted"])
def test_finish_kernel(gpu, mode):
    """G4: values = normalise(counts + pseudo) equal the restatement: the MLE fill of all-zero columns,
    Bayes 0/0 -> NaN, one-state nodes, pseudo-counts beside counts up to 2^31.  MLE exact, else rtol 1e-12."""
    rng = np.random.default_rng(23)
    counts = _finish_counts(rng)
    plan = _plan(FINISH_FAMILIES)
    bayes = mode.startswith("bayes")
    if mode.endswith("weighted"):
        counts = counts * 0.37
    pseudo = None
    if mode in ("bayes", "bayes_weighted"):
        pseudo = rng.random(counts.size) * 3 + 0.01
    elif mode == "bayes_zero_prior":
        pseudo = np.zeros(counts.size)
    got = _host(plan.finish(_dev(counts), pseudo=None if pseudo is None else _dev(pseudo), bayes=bayes))
    want = F.finish_ref(counts, FINISH_FAMILIES, pseudo=pseudo, bayes=bayes)
    if mode == "mle":
        assert np.array_equal(got, want)
        assert np.array_equal(got[:12].reshape(3, 4)[:, 1], [1 / 3] * 3)  # the fill
        assert (got[12:13] == 1.0).all() and (got[13:16] == 1.0).all()     # one-state nodes
    else:
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
    assert np.isnan(want).any() == (mode == "bayes_zero_prior")
    assert np.array_equal(np.isnan(got), np.isnan(want))


# ---------------------------------------------------------------------------- G5
def _bn(case):
    from pgmpy_amd.models import DiscreteBayesianNetwork

    m = DiscreteBayesianNetwork([tuple(e) for e in case["edges"]])
    m.add_nodes_from(case["nodes"])
    return m


def _check_cpd(cpd, want, exact):
    assert list(cpd.variables) == want["variables"] and cpd.variable == want["variables"][0]
    assert [int(c) for c in cpd.cardinality] == want["cardinality"]
    assert {v: list(cpd.state_names[v]) for v in cpd.variables} == want["state_names"]
    got, ref = np.asarray(cpd.get_values()), np.asarray(want["values"], dtype=np.float64)
    assert got.shape == ref.shape
    if exact:
        assert np.array_equal(got, ref, equal_nan=True), (cpd.variable, got, ref)
    else:
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0, equal_nan=True)


def _check_counts(sc, want, weighted, ordered=True):
    assert list(sc.index) == want["index"] and sc.index.name == want["index_name"]
    assert list(sc.columns.names) == want["column_names"]
    cols = [list(c) if isinstance(c, tuple) else [c] for c in sc.columns.tolist()]
    got = np.asarray(sc, dtype=np.float64)
    ref = np.asarray(want["values"], dtype=np.float64)
    if not ordered:  # reindex=False: the reference's column order is the groupby's
        assert sorted(map(tuple, cols)) == sorted(map(tuple, want["columns"]))
        pick = [cols.index(c) for c in want["columns"]]
        got, cols = got[:, pick], want["columns"]
    assert cols == want["columns"]
    if weighted:
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    else:
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_public_api_matches_golden(gpu, run):
    """G5, cases (a)-(d): fit, get_parameters, estimate_cpd and state_counts give the reference's CPDs
    (variables, parent order, cardinalities, state names, values) and count tables."""
    from pgmpy_amd.estimators import BayesianEstimator, MaximumLikelihoodEstimator

    _, case, key, est, kwargs, state_names, weighted = run
    cls = {"mle": MaximumLikelihoodEstimator, "bayes": BayesianEstimator}[est]
    exact = est == "mle" and not weighted
    df = F.golden_frame(case)
    want = case[key]
    extra = {"weighted": True} if weighted else {}
    sn = {"state_names": state_names} if state_names is not None else {}
    e = cls(_bn(case), df, **sn)
    cpds = e.get_parameters(**kwargs, **extra)
    # one CPD per node, in this model's node order (the reference's list follows its own graph's order)
    assert [c.variable for c in cpds] == list(e.model.nodes()) and sorted(want["node_order"]) == sorted(case["nodes"])
    for c in cpds:
        _check_cpd(c, want["cpds"][c.variable], exact)
    for n in case["nodes"]:
        per = {k: (v[n] if isinstance(v, dict) else v) for k, v in kwargs.items()}
        _check_cpd(e.estimate_cpd(n, **per, **extra), want["cpds"][n], exact)
        _check_counts(e.state_counts(n, **extra), want["counts"][n], weighted)
    m = _bn(case)
    assert m.fit(df, estimator=None if est == "mle" else cls, state_names=state_names or [], n_jobs=2,
                 **kwargs, **extra) is m
    for n in case["nodes"]:
        _check_cpd(m.get_cpds(n), want["cpds"][n], exact)
    if not any(np.isnan(np.ravel(want["cpds"][n]["values"])).any() for n in case["nodes"]):
        assert m.check_model()


def test_fit_update_and_noreindex_match_golden(gpu):
    """G5, case (a): BDeu(5) then fit_update(n_prev_samples=10) gives the reference's CPDs
    (C = [[.2525, .2525, .7475, .5], ...]); also with the current CPD's parents out of sorted order
    (transposed on the device); state_counts(reindex=False) drops the unseen parent column."""
    from pgmpy_amd.estimators import BayesianEstimator, ParameterEstimator
    from pgmpy_amd.factors.discrete import TabularCPD

    a = CASES["a"]
    df = F.golden_frame(a)
    m = _bn(a)
    m.fit(df, estimator=BayesianEstimator, prior_type="BDeu", equivalent_sample_size=5)
    before = np.array(m.get_cpds("C").get_values())
    assert m.fit_update(df, n_prev_samples=10) is None
    for n in a["nodes"]:
        _check_cpd(m.get_cpds(n), a["fit_update10"][n], exact=False)
    np.testing.assert_allclose(m.get_cpds("C").get_values()[0], [.2525, .2525, .7475, .5], atol=5e-5)
    # the same update from a C whose parents are stored as [B, A]
    swapped = before.reshape(2, 2, 2).transpose(0, 2, 1).reshape(2, 4)
    m2 = _bn(a)
    m2.fit(df, estimator=BayesianEstimator, prior_type="BDeu", equivalent_sample_size=5)
    m2.add_cpds(TabularCPD("C", 2, swapped, evidence=["B", "A"], evidence_card=[2, 2],
                           state_names={"C": [0, 1], "A": [0, 1], "B": [0, 1]}))
    m2.fit_update(df, n_prev_samples=10)
    for n in a["nodes"]:
        _check_cpd(m2.get_cpds(n), a["fit_update10"][n], exact=False)
    sc = ParameterEstimator(_bn(a), df).state_counts("C", reindex=False)
    _check_counts(sc, a["counts_C_noreindex"], weighted=False, ordered=False)


def _alarm():
    from pgmpy_amd.models import DiscreteBayesianNetwork
    from pgmpy_amd.utils import get_example_model
    from pgmpy_amd.utils.sampling import codes_to_frame

    src = get_example_model("alarm")
    nodes = sorted(src.nodes())
    m = DiscreteBayesianNetwork(list(src.edges()))
    m.add_nodes_from(src.nodes())
    states = {v: list(src.states[v]) for v in nodes}
    df = codes_to_frame(src, ALARM["codes"], nodes)
    return src, m, nodes, states, df


def _alarm_cpds(src, nodes, states, flat):
    from pgmpy_amd.factors.discrete import TabularCPD

    fams = F.alarm_families(src, nodes)
    offsets, sizes, _ = F.layout(fams)
    out = []
    for f, n in enumerate(nodes):
        ps = sorted(src.get_parents(n))
        out.append(TabularCPD(n, len(states[n]), flat[offsets[f]:offsets[f] + sizes[f]].reshape(len(states[n]), -1),
                              evidence=ps or None, evidence_card=[len(states[p]) for p in ps] or None,
                              state_names={v: states[v] for v in [n] + ps}))
    return out


@pytest.mark.parametrize("name", ["mle", "bdeu5"])
def test_alarm_fit_matches_golden(gpu, name):
    """G5, case (e): all 37 alarm CPDs from the 1,000 recorded rows, through fit on the DataFrame."""
    from pgmpy_amd.estimators import BayesianEstimator

    src, m, nodes, states, df = _alarm()
    if name == "mle":
        m.fit(df, state_names=states)
    else:
        m.fit(df, estimator=BayesianEstimator, state_names=states, prior_type="BDeu", equivalent_sample_size=5)
    fams = F.alarm_families(src, nodes)
    offsets, sizes, _ = F.layout(fams)
    for f, n in enumerate(nodes):
        cpd = m.get_cpds(n)
        assert list(cpd.variables) == [n] + sorted(src.get_parents(n))
        assert [int(c) for c in cpd.cardinality] == fams[f][1]
        assert {v: list(cpd.state_names[v]) for v in cpd.variables} == {v: states[v] for v in cpd.variables}
        got = np.asarray(cpd.get_values()).ravel()
        ref = ALARM[f"{name}_values"][offsets[f]:offsets[f] + sizes[f]]
        if name == "mle":
            assert np.array_equal(got, ref), n
        else:
            np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    assert m.check_model()


# ---------------------------------------------------------------------------- G6
def test_fit_then_predict_sees_the_new_cpds(gpu):
    """G6: predict_probability after fit equals predict_probability of a model built from the golden
    CPDs through add_cpds; after a second fit of the same object on the other half of the rows the
    same call changes and matches the second golden: the plan and value caches were invalidated."""
    src, m, nodes, states, df = _alarm()
    hidden = ["HR", "CVP", "BP"]
    rows = df.iloc[np.r_[0:25, 500:525]].drop(columns=hidden).reset_index(drop=True)

    def golden_model(key):
        from pgmpy_amd.models import DiscreteBayesianNetwork

        g = DiscreteBayesianNetwork(list(src.edges()))
        g.add_nodes_from(src.nodes())
        g.add_cpds(*_alarm_cpds(src, nodes, states, ALARM[key]))
        return g

    def same(a, b):
        assert list(a.columns) == list(b.columns) and len(a) == len(b) == 50
        np.testing.assert_allclose(a.to_numpy(dtype=float), b.to_numpy(dtype=float), rtol=1e-10, atol=1e-15,
                                   equal_nan=True)

    m.fit(df.iloc[:500].reset_index(drop=True), state_names=states)
    first = m.predict_probability(rows)
    same(first, golden_model("mle_first_values").predict_probability(rows))
    m.fit(df.iloc[500:].reset_index(drop=True), state_names=states)
    second = m.predict_probability(rows)
    same(second, golden_model("mle_second_values").predict_probability(rows))
    a, b = first.to_numpy(dtype=float), second.to_numpy(dtype=float)
    both = ~(np.isnan(a) | np.isnan(b))
    assert both.any() and np.abs(a[both] - b[both]).max() > 1e-3
