"""The E-step of the dynamic-network EM on the device (pgmpy_amd/csrc/pgmdbn.hip k_dbn_estep) against the
long-double restatement of tests/dbn_em_cases.py, through both accumulation paths, and the classes above it:
DbnPlan.estep, DBNInference.expected_counts_codes, DynamicBayesianNetwork.fit(estimator="EM") / fit_codes."""
import numpy as np
import pandas as pd
import pytest

from tests import dbn_cases as C
from tests import dbn_em_cases as M

pytestmark = pytest.mark.gpu

PATHS = {"tile": False, "direct": True}


def _device(a):
    from pgmpy_amd import engine as E

    return E.to_device_raw(np.ascontiguousarray(a))


def _host(t):
    from pgmpy_amd.inference.batch import download

    return download(t.contiguous())


def _values(spec):
    return tuple(_device(v) for v in M.flat_values(spec))


def _estep(case, direct, plan=None, **kwargs):
    """(tables0, tables1, loglik, impossible) on the host, and the plan."""
    plan = plan or M.plan_of(case["spec"], case["clamped"])
    v0, v1 = _values(case["spec"])
    out = plan.estep(_device(case["codes"]), v0, v1, direct=direct, **kwargs)
    return tuple(_host(t) for t in out), plan


def _family_sums(spec, terms, table, k):
    """Per family of set k: (the sum of its table, the terms that reached it)."""
    off = M.layout(spec)[k]
    fams = spec["fam1"] if k else spec["fam0"]
    return [(float(table[off[v]:off[v] + tab.size].sum()), int(terms[off[v]:off[v] + tab.size].sum()))
            for v, (_, tab) in enumerate(fams)]


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", sorted(C.kernel_cases()))
def test_tables_match_long_double_restatement(gpu, name, path):
    """Every branch case of the filter, through both paths: the tables within the bound of estep_ref, loglik and
    impossible the bits of DbnPlan.run, every family's table holding one unit per sequence and slice."""
    case = C.kernel_cases()[name]
    (t0, t1, loglik, flags), plan = _estep(case, PATHS[path])
    M.check_tables(case, t0, t1, f" [{path}]")
    _, _, want_ll, want_flags = plan.run(_device(case["codes"]), *_values(case["spec"]))
    assert np.array_equal(loglik.view(np.uint64), _host(want_ll).view(np.uint64))
    assert np.array_equal(flags, _host(want_flags)) and not flags.any()
    ref = M.reference(case)["ld"]
    for k, (table, per) in enumerate(((t0, case["B"]), (t1, case["B"] * case["T"]))):
        for total, n_terms in _family_sums(case["spec"], ref[4 + k], table, k):
            assert abs(total - per) <= n_terms * 2.0 ** -52 * per, (name, path, k, total, per)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_impossible_sequences_add_nothing(gpu, path):
    """Four sequences of the deterministic case contradict a one-hot CPD: they are flagged, get -inf, and the tables
    are those of the batch without them."""
    base = C.kernel_cases()["deterministic"]
    rows = [0, 5, 33, 62]
    case = M.with_impossible(base, rows)
    (t0, t1, loglik, flags), plan = _estep(case, PATHS[path])
    assert sorted(np.nonzero(flags)[0]) == rows and np.isneginf(loglik[rows]).all()
    keep = [b for b in range(case["B"]) if b not in rows]
    assert np.isfinite(loglik[keep]).all()
    rest = dict(case, name=case["name"] + "_rest", ev=case["ev"][keep], codes=C.to_codes(case["ev"][keep]), B=len(keep))
    M.check_tables(rest, t0, t1, f" [{path}, with the impossible rows]")
    (r0, r1, rest_ll, _), _ = _estep(rest, PATHS[path], plan)
    M.check_tables(rest, r0, r1, f" [{path}, without them]")
    assert np.array_equal(rest_ll.view(np.uint64), loglik[keep].view(np.uint64))
    for k, table in enumerate((t0, t1)):
        per = len(keep) * (case["T"] if k else 1)
        for total, n_terms in _family_sums(case["spec"], M.reference(rest)["ld"][4 + k], table, k):
            assert abs(total - per) <= n_terms * 2.0 ** -52 * per


def test_large_table_takes_the_direct_path(gpu):
    """20,655 transition entries cannot tile: the info says direct, and the tables are within the bound."""
    from pgmpy_amd import _native as N

    case = M.large_table_case()
    plan = M.plan_of(case["spec"], case["clamped"])
    assert plan.estep_info().path == N.DBN_ESTEP_DIRECT and not plan.estep_info().tile_fits
    (t0, t1, loglik, flags), _ = _estep(case, False, plan)
    assert not flags.any() and np.isfinite(loglik).all()
    M.check_tables(case, t0, t1)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_observed_batch_gives_exact_integers(gpu, path):
    """Every cell observed (B = 130, T = 4): one (i, x') survives per slice with weight g / g = 1.0, so the tables
    are the integer counts bit for bit, with every node clamped, none, and some."""
    spec = C.make_spec(seed=72, **C.TWO_IFACE)
    ev = C.sample(spec, 4, 130, 600)
    want0, want1 = M.observed_counts(spec, ev)
    for clamped in (spec["names"], [], ["W", "Y"]):
        case = {"spec": spec, "clamped": clamped, "codes": C.to_codes(ev)}
        (t0, t1, _, flags), _ = _estep(case, PATHS[path])
        assert not flags.any()
        assert np.array_equal(t0, want0) and np.array_equal(t1, want1), (path, clamped)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_row_windows_and_split_scratch(gpu, path):
    """Rows [3, 3 + B) of a buffer with ld = B + 8 whose pad rows hold a code that is no state and must not be read;
    and a scratch that holds 7 sequences, which splits the batch by rows.  Both within the bound of the unsplit
    reference; the split run's loglik is the unsplit run's."""
    case = C.kernel_cases()["J15_S3"]
    B = case["B"]
    padded = np.full((case["codes"].shape[0], B + 8), 200, dtype=np.uint8)
    padded[:, 3:3 + B] = case["codes"]
    plan = M.plan_of(case["spec"], case["clamped"])
    v0, v1 = _values(case["spec"])
    t0, t1, loglik, flags = (_host(t) for t in plan.estep(_device(padded), v0, v1, n_rows=B, row0=3, direct=PATHS[path]))
    assert loglik.shape == (B,) and not flags.any()
    M.check_tables(case, t0, t1, f" [{path}, window]")
    small = plan.scratch_bytes(7, case["T"] + 1)
    (s0, s1, split_ll, _), _ = _estep(case, PATHS[path], plan, scratch_bytes=small)
    M.check_tables(case, s0, s1, f" [{path}, split]")
    assert np.array_equal(split_ll.view(np.uint64), loglik.view(np.uint64))


def test_grid_stride_and_partial_last_group(gpu):
    """spw (grid cap + 1) + 1 sequences at T = 1: one workgroup takes two groups, the last group holds one sequence."""
    spec = C.doc_spec()
    plan = M.plan_of(spec, ["X", "Y"])
    cap, spw = int(plan.estep_info().max_blocks), int(plan.info.seq_per_wave)
    B = spw * (cap + 1) + 1
    rng = np.random.default_rng(610)
    ev = rng.integers(0, 2, size=(B, 2, 3)).astype(np.uint8)
    ev[:, :, 2][rng.random((B, 2)) < 0.5] = C.MISSING
    case = {"name": f"doc_grid_stride_B{B}", "spec": spec, "clamped": ["X", "Y"], "T": 1, "B": B, "ev": ev,
            "codes": C.to_codes(ev)}
    M.reference_by_unique_rows(case)
    (t0, t1, loglik, flags), _ = _estep(case, False, plan)
    assert not flags.any() and np.isfinite(loglik).all()
    M.check_tables(case, t0, t1)
    assert abs(t0.sum() - 3 * B) <= 1e-9 * B and abs(t1.sum() - 3 * B) <= 1e-9 * B


@pytest.mark.parametrize("path", sorted(PATHS))
def test_tables_are_added_to(gpu, path):
    """Pre-filled tables come back as prefill + counts.  An add onto an entry that holds prefill + a partial sum
    rounds relative to that, so N adds may cost (N + 8) 2^-52 prefill beside the bound of the counts."""
    import torch

    case = C.kernel_cases()["two_iface"]
    plan = M.plan_of(case["spec"], case["clamped"])
    v0, v1 = _values(case["spec"])
    rng = np.random.default_rng(620)
    fill = [np.where(rng.random(int(n)) < 0.5, 0.0, 2.0) for n in (plan.info.values0, plan.info.values1)]
    got = plan.estep(_device(case["codes"]), v0, v1, tables0=_device(fill[0]), tables1=_device(fill[1]), direct=PATHS[path])
    ref = M.reference(case)
    for k in (0, 1):
        counts = _host(got[k]) - fill[k]
        allowed = M.table_bound(ref["ld"][k], ref["ld"][4 + k], ref["d"], ref["e_max"]) + (ref["ld"][4 + k] + 8) * 2.0 ** -52 * fill[k]
        err = np.abs(counts.astype(M.LD) - ref["ld"][k]).astype(np.float64)
        assert (err <= allowed).all(), (path, k, float((err / allowed).max()))
    assert isinstance(got[0], torch.Tensor) and got[0].is_cuda


# ------------------------------------------------------------------------------------------------ the classes
def _frame(spec, ev, names):
    """The frame of the sequences ev [B, T + 1, n] with (name, t) columns of the nodes `names`."""
    cols = {(name, t): ev[:, t, spec["names"].index(name)].astype(np.int64) for t in range(ev.shape[1]) for name in names}
    frame = pd.DataFrame(cols)
    frame.columns = pd.Index(list(cols), tupleize_cols=False)
    return frame


def _flat_cpds(model):
    from pgmpy_amd.inference import DBNInference
    from pgmpy_amd.inference._dbn import flat_values

    inf = DBNInference(model)
    return flat_values(inf.cpds0), flat_values(inf.cpds1)


def test_expected_counts_codes(gpu):
    """DBNInference's entry point returns the plan's tables, resident."""
    case = C.kernel_cases()["cross_edge"]
    from pgmpy_amd.inference import DBNInference

    inf = DBNInference(C.to_model(case["spec"]))
    t0, t1, loglik, flags = inf.expected_counts_codes(_device(case["codes"]), observed=case["clamped"])
    assert t0.is_cuda and t1.is_cuda and loglik.is_cuda
    M.check_tables(case, _host(t0), _host(t1), " [expected_counts_codes]")
    ll, _ = inf.log_likelihood_codes(_device(case["codes"]), observed=case["clamped"])
    assert np.array_equal(_host(loglik).view(np.uint64), _host(ll).view(np.uint64)) and not _host(flags).any()


def test_fit_em_end_to_end(gpu):
    """The HMM with its chain dropped from the frame, 400 sequences x 6 slices, three iterations from fixed CPDs:
    the CPDs within 16 d3 of em_ref's (d3: the fp64-vs-long-double deviation of em_ref itself after 3 iterations,
    floor 64 * 2^-53), the log-likelihoods those of em_ref and non-decreasing up to rounding, n_iter_ == 3."""
    truth = C.hmm_spec(states=3, n_obs=2)
    start = C.hmm_spec(states=3, n_obs=2, seed=631)
    ev = C.sample(truth, 5, 400, 630)
    observed = truth["names"][1:]
    model = C.to_model(start)
    model.fit(_frame(truth, ev, observed), estimator="EM", max_iter=3, atol=0)
    assert model.n_iter_ == 3 and len(model.log_likelihoods_) == 3
    hidden = ev.copy()
    hidden[:, :, 0] = C.MISSING
    want0, want1, want_ll = M.em_ref(start, observed, hidden, 3)
    f0, f1, _ = M.em_ref(start, observed, hidden, 3, dtype=np.float64)
    d3 = max(float(np.abs(f0 - want0).max()), float(np.abs(f1 - want1).max()))
    tol = 16 * max(d3, 64 * M.U)
    got0, got1 = _flat_cpds(model)
    worst = max(float(np.abs(got0 - want0).max()), float(np.abs(got1 - want1).max()))
    print(f"fit EM, 3 iterations: worst CPD error {worst:.3g}, allowed {tol:.3g} (d3 {d3:.3g})")
    assert worst <= tol
    lls = model.log_likelihoods_
    slack = [M.loglik_slack(start, observed, 400, 6, x) for x in lls]
    for got, want, s in zip(lls, want_ll, slack):
        assert abs(got - float(want)) <= s + 16 * max(d3, 64 * M.U) * 400 * 6, (got, float(want))
    assert all(b >= a - s for a, b, s in zip(lls, lls[1:], slack[1:])) and lls[-1] > lls[0]
    assert len(model.get_cpds()) == 6 and model.check_model()


def test_fit_em_on_complete_data_is_the_counts(gpu):
    """Every cell observed, one iteration, two slices: the transition CPDs are those of fit(estimator="MLE") to
    1e-15 and the slice-0 CPDs the column-normalised counts of slice 0.  (With more than one window "MLE" averages
    normalised CPDs over the windows, as the reference does, and is no maximum-likelihood estimate to compare to.)"""
    from pgmpy_amd.models import DynamicBayesianNetwork

    spec = C.make_spec(seed=72, **C.TWO_IFACE)
    ev = C.sample(spec, 1, 300, 640)
    frame = _frame(spec, ev, spec["names"])
    model = C.to_model(C.make_spec(seed=641, **C.TWO_IFACE))
    model.fit(frame, estimator="EM", max_iter=1)
    assert model.n_iter_ == 1
    counts0, counts1 = M.observed_counts(spec, ev)
    want0, want1 = M.normalise(spec, counts0, counts1)
    got0, got1 = _flat_cpds(model)
    assert float(np.abs(got0 - want0).max()) <= 1e-15 and float(np.abs(got1 - want1).max()) <= 1e-15
    mle = DynamicBayesianNetwork()
    mle.add_nodes_from(spec["names"])
    mle.add_edges_from([tuple(e) for e in model.edges()])
    mle.fit(frame, estimator="MLE")
    for name in spec["names"]:
        ours, theirs = model.get_cpds((name, 1)), mle.get_cpds((name, 1))
        order = sorted(ours.variables)
        arrays = []
        for cpd in (ours, theirs):
            assert sorted(cpd.variables) == order
            a = np.asarray(cpd._values_readonly(), dtype=np.float64).reshape([int(k) for k in cpd.cardinality])
            arrays.append(a.transpose([list(cpd.variables).index(v) for v in order]))
        assert float(np.abs(arrays[0] - arrays[1]).max()) <= 1e-15, name


def test_fit_codes_resident(gpu):
    """simulate_codes -> fit_codes never leaves the device; the data's log-likelihood under the fitted model is not
    below the one under the model it started from."""
    from pgmpy_amd.inference import DBNInference

    truth = C.to_model(C.hmm_spec(states=3, n_obs=2))
    codes = truth.simulate_codes(2000, 6, seed=650).clone()
    n = 3
    codes[0::n] = C.MISSING  # H, the first node in sorted order, in every slice
    observed = ["O0", "O1"]
    model = C.to_model(C.hmm_spec(states=3, n_obs=2, seed=651))
    before = float(_host(DBNInference(model).log_likelihood_codes(codes, observed)[0]).sum())
    model.fit_codes(codes, 6, observed=observed, max_iter=5, init_cpds=None)
    after = float(_host(DBNInference(model).log_likelihood_codes(codes, observed)[0]).sum())
    assert 1 <= model.n_iter_ <= 5 and len(model.log_likelihoods_) == model.n_iter_
    assert abs(model.log_likelihoods_[0] - before) <= M.loglik_slack(C.hmm_spec(states=3, n_obs=2), observed, 2000, 6, before)
    assert after >= before and after >= model.log_likelihoods_[-1] - 1e-9 * abs(after)
    # random starting values for the hidden node's families and its children's: it still improves on its start
    again = C.to_model(C.hmm_spec(states=3, n_obs=2, seed=651))
    again.fit_codes(codes, 6, observed=observed, max_iter=4, init_cpds="random", seed=7)
    assert again.log_likelihoods_[-1] >= again.log_likelihoods_[0]
