"""The dynamic-network filter on the device (pgmpy_amd/csrc/pgmdbn.hip) against the long-double restatement
and the enumeration of tests/dbn_cases.py, and the classes above it: DBNInference's reference and batched
entry points, DynamicBayesianNetwork.fit / simulate / simulate_codes."""
import numpy as np
import pandas as pd
import pytest

from pgmpy_amd.inference import DBNInference  # noqa: F401  (without the feature the module does not import)
from pgmpy_amd.models import DynamicBayesianNetwork, DynamicNode  # noqa: F401
from tests import dbn_cases as C

pytestmark = pytest.mark.gpu


def _inference(spec):
    from pgmpy_amd.inference import DBNInference

    return DBNInference(C.to_model(spec))


def _device(codes):
    from pgmpy_amd import engine as E

    return E.to_device_raw(np.ascontiguousarray(codes))


def _host(t):
    from pgmpy_amd.inference.batch import download

    return download(t.contiguous())


def _run(case, inf=None):
    """(filter, smooth, loglik from the filter call, loglik from the smoother, impossible) on the host."""
    inf = inf or _inference(case["spec"])
    codes = _device(case["codes"])
    f, lf, flags = inf.filter_codes(codes, observed=case["clamped"])
    s, ls, flags2 = inf.smooth_codes(codes, observed=case["clamped"])
    assert np.array_equal(_host(flags), _host(flags2))
    return _host(f), _host(s), _host(lf), _host(ls), _host(flags)


def _assert_path(case, inf):
    """A case of C.path_cases() is the case it claims to be: the plan has the geometry the case was built for."""
    i = inf.plan(case["clamped"]).info
    want = case["expect"]
    got = dict(J=i.n_configs, S=i.n_interface, spw=i.seq_per_wave, lds=i.lds_bytes, n_prev=i.n_prev_families,
               n_cur=i.n_cur_families)
    assert got == want, (case["name"], got, want)
    if case["name"] in ("n255_all_clamped", "J3072_S3072"):
        assert i.lds_bytes > 65536, "this case is there for the launch with more than 64 KiB of dynamic LDS"


def _check_case(case, rows=None):
    dm, dl = C.golden_d(case)
    tol_m, tol_l = C.tolerance(dm), C.tolerance(dl)
    inf = _inference(case["spec"])
    if "expect" in case:
        _assert_path(case, inf)
    f, s, lf, ls, flags = _run(case, inf)
    assert f.shape == s.shape == (case["B"], case["T"] + 1, sum(case["spec"]["card"]))
    assert np.array_equal(lf.view(np.uint64), ls.view(np.uint64)), "the smoother's forward pass is the filter's"
    worst = [0.0, 0.0, 0.0]
    for b in range(case["B"]) if rows is None else rows:
        wf, ws, wl, dead = C.reference(case, b)
        assert not dead and flags[b] == 0
        worst[0] = max(worst[0], float(np.abs(f[b] - wf).max()))
        worst[1] = max(worst[1], float(np.abs(s[b] - ws).max()))
        worst[2] = max(worst[2], float(abs(lf[b] - wl) / max(abs(wl), 1.0)))
    print(f"{case['name']}: filter {worst[0]:.3g} smooth {worst[1]:.3g} (allowed {tol_m:.3g}), "
          f"loglik {worst[2]:.3g} (allowed {tol_l:.3g})")
    # marginals are relative to their largest entry, which is at most 1: the bound is absolute
    assert worst[0] <= tol_m and worst[1] <= tol_m and worst[2] <= tol_l


@pytest.mark.parametrize("name", sorted(C.kernel_cases()) + sorted(C.path_cases()))
def test_device_matches_long_double_recursion(gpu, name):
    """filter, smooth and loglik of every sequence of every branch case and every path case, within
    max(16 d, 64 u); a path case also has the plan geometry it was built for (tests/test_dbn_paths_gpu.py records
    the worst error / allowed of the path cases)."""
    _check_case(C.all_cases()[name])


def test_all_clamped_yields_indicators(gpu):
    case = C.kernel_cases()["all_clamped_J1"]
    f, s, lf, _, _ = _run(case)
    off, _ = C.offsets(case["spec"])
    for v in range(3):
        hot = np.arange(2)[None, None, :] == case["ev"][:, :, v][:, :, None]
        assert np.array_equal(f[:, :, off[v]:off[v] + 2], hot.astype(float))
        assert np.array_equal(s[:, :, off[v]:off[v] + 2], hot.astype(float))
    assert np.isfinite(lf).all()


def test_interface_evidence_is_exact_where_the_reference_is_not(gpu):
    """An interface node observed at t >= 1 and an earlier slice queried: the device equals enumeration and is
    more than 1e-2 from what the reference returns (recorded in tests/golden/dbn_cases.json)."""
    golden = C.load_golden()
    for case in C.interface_evidence_cases():
        inf = _inference(case["spec"])
        got = inf.query([case["query"]], case["evidence"])[case["query"]]
        T = max(t for _, t in list(case["evidence"]) + [case["query"]])
        ev = C.evidence_array(case["spec"], case["evidence"], T)
        _, es, _ = C.enumerate_unrolled(case["spec"], ev, smooth_only=True)
        off, _ = C.offsets(case["spec"])
        v = case["spec"]["names"].index(case["query"][0])
        want = es[case["query"][1], off[v]:off[v] + case["spec"]["card"][v]].astype(np.float64)
        np.testing.assert_allclose(np.asarray(got.values), want, rtol=0, atol=64 * C.U)
        rec = golden["interface_evidence"][case["name"]]
        np.testing.assert_allclose(rec["enumerated"], want, rtol=0, atol=1e-12)
        assert np.abs(np.asarray(got.values) - np.asarray(rec["reference"])).max() > 1e-2


def test_long_sequence(gpu):
    """T = 2,000: the scaling keeps everything finite; loglik within the rule, marginals sum to 1.  This length is
    also what covers a beta update that drops its / c_t: gamma is renormalised, so at T = 2 that error is invisible
    by construction (it is no fault of dbn_cases.FAULTS); over 2,000 slices the unscaled beta leaves fp64's range."""
    spec = C.make_spec(names=["A", "B", "O"], card=[2, 2, 3], intra=[("A", "O"), ("B", "O")],
                       inter=[("A", "A"), ("B", "B"), ("A", "B")], seed=90)
    case = C._case("long_T2000", spec, ["O"], 2000, 4, 91, hide=0.5)
    f, s, lf, ls, flags = _run(case)
    assert not flags.any() and np.isfinite(lf).all()
    off, _ = C.offsets(spec)
    for v in range(3):
        for m in (f, s):
            np.testing.assert_allclose(m[:, :, off[v]:off[v] + spec["card"][v]].sum(axis=2), 1.0, rtol=0, atol=1e-12)
    _check_case(case, rows=[0])


def test_bit_identity_across_batch_positions(gpu):
    """A sequence alone, at row 0 of a batch of 130 and at row 77 gives byte-equal outputs."""
    case = C.kernel_cases()["J15_S3"]
    inf = _inference(case["spec"])
    base = case["codes"]
    seq = base[:, 5:6]
    alone = dict(case, codes=np.ascontiguousarray(seq), B=1)
    batch = base.copy()
    batch[:, 0] = seq[:, 0]
    batch[:, 77] = seq[:, 0]
    a = _run(alone, inf)
    b = _run(dict(case, codes=batch), inf)
    for x, y in zip(a[:4], b[:4]):
        assert x[0].tobytes() == y[0].tobytes() == y[77].tobytes()
    # and a smoother split into row windows by a small scratch gives the same bytes
    s_small, _, _ = inf.smooth_codes(_device(batch), observed=case["clamped"], scratch_bytes=7 * 3 * 4 * 8)
    assert _host(s_small).tobytes() == b[1].tobytes()


def test_impossible_evidence(gpu):
    """One impossible sequence among good ones: its flag, -inf and NaNs; byte-equal neighbours."""
    case = C.kernel_cases()["deterministic"]
    spec = case["spec"]
    inf = _inference(spec)
    good = _run(case, inf)
    # X is a deterministic function of Z: observe Z and the X it excludes at slice 1
    x_of_z = np.argmax(spec["fam1"][0][1], axis=0)  # the X each Z gives
    codes = case["codes"].copy()
    n, b = 3, 31
    codes[:, b] = C.MISSING
    codes[0 * n + 1, b] = case["ev"][b, 0, 1]
    codes[1 * n + 1, b] = case["ev"][b, 1, 1]
    codes[2 * n + 1, b] = case["ev"][b, 2, 1]
    codes[1 * n + 2, b] = 0
    codes[1 * n + 0, b] = 1 - x_of_z[0]
    f, s, lf, ls, flags = _run(dict(case, codes=codes), inf)
    assert flags[b] == 1 and flags.sum() == 1
    assert lf[b] == -np.inf and ls[b] == -np.inf
    assert np.isfinite(f[b, 0]).all() and np.isnan(f[b, 1:]).all() and np.isnan(s[b]).all()
    keep = np.arange(case["B"]) != b
    for x, y in zip((f, s, lf, ls), good[:4]):
        assert x[keep].tobytes() == y[keep].tobytes()


def test_bad_codes_are_refused(gpu):
    case = C.kernel_cases()["doc_J2_T1_B63"]
    inf = _inference(case["spec"])
    for row, col, code in ((7, 0, C.MISSING), (9, 3, 2), (11, 2, 5)):  # a clamped cell missing; codes >= card
        codes = case["codes"].copy()
        codes[col, row] = code
        with pytest.raises(ValueError, match="dbn_run"):
            inf.filter_codes(_device(codes), observed=case["clamped"])
    f, _, _ = inf.filter_codes(_device(case["codes"]), observed=case["clamped"])  # and the handle still works
    assert np.isfinite(_host(f)).all()


def test_reference_api_matches_golden(gpu):
    """forward_inference, backward_inference and query agree with the recorded reference results to 1e-12."""
    golden = C.load_golden()
    from pgmpy_amd.factors.discrete import DiscreteFactor

    for rec in golden["queries"]:
        spec = C.golden_spec(golden, rec["network"])
        inf = _inference(spec)
        ev = {(k[0], int(k[1])): int(s) for k, s in rec["evidence"]}
        variables = [(v[0], int(v[1])) for v in rec["variables"]]
        for method, key in ((inf.forward_inference, "forward"), (inf.backward_inference, "backward"), (inf.query, "backward")):
            got = method(variables, ev)
            assert set(got) == set(variables)
            wants = rec[key]
            if wants is None:  # the reference's backward pass is wrong here: the enumerated values were recorded instead
                faults = {tuple(f["variable"]): f["enumerated"] for f in golden["reference_faults"]
                          if (f["network"], f["pattern"]) == (rec["network"], rec["pattern"])}
                wants = [faults[(var[0], var[1])] for var in variables]
            for var, want in zip(variables, wants):
                fac = got[var]
                assert isinstance(fac, DiscreteFactor) and list(fac.variables) == [var]
                assert fac.state_names[var] == list(range(len(want)))
                np.testing.assert_allclose(np.asarray(fac.values), want, rtol=0, atol=1e-12)
    with pytest.raises(NotImplementedError):
        inf.forward_inference(variables, ev, args="potential")


def test_batched_frames(gpu):
    """filter_batch / smooth_batch / log_likelihood_batch on a frame: NaN and absent columns are unobserved."""
    case = C.kernel_cases()["doc_free_J8_S2"]
    spec, ev = case["spec"], case["ev"]
    inf = _inference(spec)
    cols = {}
    for t in range(case["T"] + 1):
        for v, name in enumerate(spec["names"]):
            if (name, t) == ("Y", 1):
                continue  # an absent column
            cols[(name, t)] = np.where(ev[:, t, v] == C.MISSING, np.nan, ev[:, t, v].astype(float))
    df = pd.DataFrame(cols)
    ev2 = ev.copy()
    ev2[:, 1, 1] = C.MISSING
    res_f, res_s, res_l = inf.filter_batch(df), inf.smooth_batch(df, variables=["Z"]), inf.log_likelihood_batch(df)
    off, _ = C.offsets(spec)
    for b in range(0, case["B"], 9):
        wf, ws, wl, _ = C.recursion(spec, [], ev2[b])
        for v, name in enumerate(spec["names"]):
            np.testing.assert_allclose(res_f.marginal(name)[b], wf[:, off[v]:off[v] + 2].astype(float), rtol=0, atol=64 * C.U)
        np.testing.assert_allclose(res_s.marginal("Z")[b], ws[:, off[2]:off[2] + 2].astype(float), rtol=0, atol=64 * C.U)
        np.testing.assert_allclose(res_l.log_likelihood[b], float(wl), rtol=64 * C.U)
    assert not res_l.impossible.any() and res_f.log_likelihood.shape == (case["B"],)
    with pytest.raises(ValueError):
        res_s.marginal("X")


def test_fit_matches_reference(gpu):
    """DynamicBayesianNetwork.fit gives the reference's CPDs (the tolerance test_fit_gpu uses for fit_update)."""
    golden = C.load_golden()
    from pgmpy_amd.models import DynamicBayesianNetwork

    g = golden["fit"]
    data = C.load_golden_arrays()["fit_data"]
    columns = [(c[0], int(c[1])) for c in g["columns"]]
    df = pd.DataFrame(data, columns=pd.Index(columns, tupleize_cols=False))
    m = DynamicBayesianNetwork([((a[0], int(a[1])), (b[0], int(b[1]))) for a, b in g["edges"]])
    m.fit(df)
    assert len(m.cpds) == len(g["cpds"])
    for want in g["cpds"]:
        var = (want["variables"][0][0], int(want["variables"][0][1]))
        cpd = m.get_cpds(var)
        assert [tuple(v) for v in cpd.variables] == [(v[0], int(v[1])) for v in want["variables"]]
        np.testing.assert_allclose(np.asarray(cpd.get_values()), np.asarray(want["values"]), rtol=1e-12, atol=0)


def test_simulate(gpu):
    """200,000 samples, T = 3: every node's empirical marginal at every slice within 5 sigma of the enumerated
    one; evidence and do columns constant; simulate_codes -> smooth_codes with everything clamped."""
    spec = C.doc_spec()
    m = C.to_model(spec)
    N, T = 200_000, 3
    df = m.simulate(n_samples=N, n_time_slices=T + 1, seed=5)
    assert list(df.columns) == [(name, t) for t in range(T + 1) for name in spec["names"]]
    _, es, _ = C.enumerate_unrolled(spec, np.full((T + 1, 3), C.MISSING, dtype=np.uint8), smooth_only=True)
    off, _ = C.offsets(spec)
    for t in range(T + 1):
        for v, name in enumerate(spec["names"]):
            p = float(es[t, off[v] + 1])
            emp = float((df[(name, t)].astype(int) == 1).mean())
            assert abs(emp - p) <= 5 * np.sqrt(p * (1 - p) / N), (name, t, emp, p)
    small = m.simulate(n_samples=500, n_time_slices=3, evidence={("Y", 1): 1}, do={("Z", 2): 0}, seed=6)
    assert (small[("Y", 1)].astype(int) == 1).all() and (small[("Z", 2)].astype(int) == 0).all()
    codes = m.simulate_codes(1000, T + 1, seed=7)
    assert tuple(codes.shape) == ((T + 1) * 3, 1000) and codes.is_cuda
    from pgmpy_amd.inference import DBNInference

    inf = DBNInference(m)
    s, ll, flags = inf.smooth_codes(codes, observed=spec["names"])
    s, host = _host(s), _host(codes)
    for v in range(3):
        hot = np.arange(2)[None, None, :] == host.T.reshape(1000, T + 1, 3)[:, :, v][:, :, None]
        assert np.array_equal(s[:, :, off[v]:off[v] + 2], hot.astype(float))
    assert np.isfinite(_host(ll)).all() and not _host(flags).any()
