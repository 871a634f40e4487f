"""The linear-Gaussian kernels on wide and deep synthetic plans (tests/lg_cases.py, "wide and deep synthetic plans"):
k_lg_gram / k_lg_gram_reduce at three and four super-tiles and with the automatic and the raised slice, k_lg_affine
past one launch, k_lg_sample / k_lg_logpdf / k_lg_logpdf_sum at up to 4,096 parents, 300-node chains, every order of
a Philox pair and first_row up to INT64_MAX, the public API on a 300-node random model, and k_lgs_lane / k_lgs_wave
reading a Gram matrix of three super-tiles.  Every comparison is against the long-double restatement under a bound
derived in tests/lg_cases.py or tests/lgs_cases.py; tests/test_lg_cpu.py shows for every shape that the bound sees
a structural error.  Each test prints its worst error / bound.

Worst error / bound per family (MI355X, 2026-10-21, one run of this module; the data is seeded, so a run repeats it):
  k_lg_gram, windows of 1 .. 33 rows    0.916 (d = 200, row0 = 0; at n = 1 the bound is three roundings), 0.149 on the
                                        shuffled subset
  k_lg_gram, sliced                     0.025 (automatic, d = 200, 1,025 rows), 0.004 (raised, d = 200, 1,633 rows)
  k_lg_affine                           0.498 (one input), 0.042 with 256 .. 600 inputs
  k_lg_sample                           0.494 (max_parents; 0.33 .. 0.49 over the seven plans)
  k_lg_logpdf, per row                  0.076 (odd_first), 0.001 at 4,096 parents; the 258-partial total below 0.0005
  simulate / log-likelihood / predict   0.470 / below 0.0005 / 0.055 on the 300-node model (fit: check_fit, kappa to 4.5e3)
  k_lgs_lane / k_lgs_wave, d = 150      0.015 (the Gram matrix they read: 0.051)
No bound was exceeded and no derivation changed.
"""
import ctypes

import numpy as np
import pytest

from tests import lg_cases as LC
from tests import lgs_cases as LGS
from tests.test_lg_gpu import _assert_distribution, _dev

pytestmark = pytest.mark.gpu

LD = np.longdouble


def _report(capsys, what, ratio):
    with capsys.disabled():
        print(f"\n{what}: worst error / bound {ratio:.3f}")


def _run_gram(host, cols, shift, row0, n_rows, slice_rows=None, expect=None):
    """(device G as ndarray, G long double, bound, plan): expect = (rows per slice, slices, 16-byte loads) or None."""
    from pgmpy_amd.models._lg import GramPlan

    plan = GramPlan(cols)
    if slice_rows:
        plan.set_slice(slice_rows)
    X = _dev(host)
    if expect is not None:
        assert plan.gram_info(n_rows, X.data_ptr(), host.shape[1], row0) == expect
    got = plan.gram(X, _dev(shift), n_rows, row0).cpu().numpy()
    want, A = LC.gram_ld(host[:, row0:row0 + n_rows], cols, shift)
    return got, want, LC.gram_bound(A, n_rows), plan


def _check_gram(got, want, bound, what):
    """As test_lg_gpu._assert_gram; returns the worst error / bound."""
    d = got.shape[0] - 1
    assert np.array_equal(got, got.T), what
    assert got[d, d] == float(want[d, d]), what
    ratio = LC.worst_ratio(got, want, bound)
    assert ratio <= 1.0, (what, ratio)
    return ratio


# ---------------------------------------------------------------------- 1. Gram at three and four super-tiles
@pytest.mark.parametrize("row0", [0, 1])
@pytest.mark.parametrize("d", LC.GRAM_WIDE_D)
def test_gram_wide(gpu, capsys, d, row0):
    """Six and ten groups: the I-major group list, waves with both sides off the first super-tile, the partials'
    [slice][group] stride and the reduce kernel's (I, J) to (row, col) map.  Rows outside the window and the columns
    the plan does not name hold NaN."""
    worst = 0.0
    for name, dd, r0, n_rows, kw in LC.gram_wide_shapes():
        if (dd, r0) != (d, row0) or "n_cols" in kw:
            continue
        host, cols, shift = LC.gram_window(d, row0, n_rows, **kw)
        assert np.isnan(host[d // 2]).all() and d // 2 not in cols
        got, want, bound, plan = _run_gram(host, cols, shift, row0, n_rows, expect=(LC.SLICE_MIN, 1, row0 % 2 == 0))
        assert plan.info.n_super == (d + 1 + 63) // 64 >= 3 and plan.info.n_groups in (6, 10)
        worst = max(worst, _check_gram(got, want, bound, name))
    _report(capsys, f"k_lg_gram d = {d} row0 = {row0}", worst)


def test_gram_wide_permuted_subset(gpu, capsys):
    """140 of 150 columns in shuffled order: a tile's columns are not contiguous in X, the other ten are NaN."""
    (name, d, row0, n_rows, kw), = [s for s in LC.gram_wide_shapes() if "n_cols" in s[4]]
    host, cols, shift = LC.gram_window(d, row0, n_rows, **kw)
    assert sorted(cols) != cols and np.isnan(host[[c for c in range(150) if c not in cols]]).all()
    got, want, bound, _ = _run_gram(host, cols, shift, row0, n_rows)
    _report(capsys, "k_lg_gram 140 of 150 columns, shuffled", _check_gram(got, want, bound, name))


# ---------------------------------------------------------------------- 2. slices on the device
@pytest.mark.parametrize("d", [3, 200])
@pytest.mark.parametrize("kind", ["auto", "raised"])
def test_gram_slices(gpu, capsys, kind, d):
    """The two outcomes of lg_slice_rows no Gram had run with: the automatic split above PGM_LG_SLICE_MIN rows and a
    forced slice of one step raised until the handle's partials hold the slices."""
    from pgmpy_amd.models._lg import GramPlan

    max_slices = int(GramPlan(list(range(d))).info.max_slices)
    assert max_slices == {3: 1024, 200: 102}[d]
    n_rows = LC.slice_rows_of(kind, max_slices)
    host, cols, shift = LC.gram_window(d, 2, n_rows, seed=d + n_rows, ld=n_rows + 7)  # an even ld: 16-byte loads
    if kind == "auto":
        expect = (LC.SLICE_MIN, 2, True)
    else:
        expect = (2 * LC.STEP, (n_rows + 2 * LC.STEP - 1) // (2 * LC.STEP), True)
        assert expect[1] <= max_slices < (n_rows + LC.STEP - 1) // LC.STEP
    got, want, bound, _ = _run_gram(host, cols, shift, 2, n_rows, slice_rows=1 if kind == "raised" else None, expect=expect)
    _report(capsys, f"k_lg_gram {kind} slices d = {d} n_rows = {n_rows}", _check_gram(got, want, bound, (kind, d)))


# ---------------------------------------------------------------------- 3. bit-identity across widths
def test_gram_wide_bit_identity(gpu):
    """Three columns standing in super-tiles 0, 1 and 3 of a 200-column handle: their block (diagonal groups and the
    groups (0, 1), (0, 3), (1, 3)) and their entries against the ones column carry the bits a three-column handle
    gives at the same forced slice, and a second run carries the same bits."""
    from pgmpy_amd.models._lg import GramPlan

    n_rows = 200
    host = LC.wide_data(200, n_rows, seed=31)
    X = _dev(host)
    narrow = [17, 101, 150]
    rest = [c for c in range(200) if c not in narrow]
    wide = rest[:5] + [17] + rest[5:69] + [101] + rest[69:193] + [150] + rest[193:]
    pos = [wide.index(c) for c in narrow]
    assert len(wide) == 200 and [p // 64 for p in pos] == [0, 1, 3]
    shift = LC.colmean(host, list(range(200)))
    out = {}
    for name, cols in (("narrow", narrow), ("wide", wide)):
        p = GramPlan(cols)
        p.set_slice(64)
        assert p.gram_info(n_rows)[:2] == (64, 4)
        out[name] = p.gram(X, _dev(shift[cols]), n_rows).cpu().numpy()
        assert np.array_equal(out[name], p.gram(X, _dev(shift[cols]), n_rows).cpu().numpy())
    ix = pos + [200]
    assert np.array_equal(out["narrow"], out["wide"][np.ix_(ix, ix)])
    assert len({out["narrow"][a, b] for a in range(3) for b in range(a, 4)}) == 9  # every entry is its own number


# ---------------------------------------------------------------------- 4. the affine map
@pytest.mark.parametrize("n_in", LC.AFFINE_N_IN)
def test_affine_every_launch_count(gpu, capsys, n_in):
    """No input column (the constants alone), one launch, two and three: a later launch starts from the output of
    the one before and takes W from its first column on."""
    from pgmpy_amd.models._lg import affine

    worst = 0.0
    for n_out in LC.AFFINE_N_OUT:
        for n_rows in LC.AFFINE_ROWS:
            for row0 in (0, 3):
                W, c, in_cols, host = LC.affine_case(n_in, n_out, n_rows, row0)
                got = affine(W, c, in_cols, _dev(host), n_rows, row0).cpu().numpy()
                want, bound = LC.affine_ld(W, c, in_cols, host[:, row0:row0 + n_rows])
                assert got.shape == (n_out, n_rows)
                ratio = LC.worst_ratio(got, want, bound)
                assert ratio <= 1.0, (n_in, n_out, n_rows, row0, ratio)
                worst = max(worst, ratio)
    _report(capsys, f"k_lg_affine n_in = {n_in}", worst)


def test_affine_later_launches_read_back(gpu):
    """600 inputs whose columns from 256 on have weight 0 give the bits of the 256-input call: the second and third
    launch add zeros to what the first one wrote."""
    from pgmpy_amd.models._lg import affine

    W, c, in_cols, host = LC.affine_case(600, 5, 257, 3)
    W[:, 256:] = 0.0
    X = _dev(host)
    full = affine(W, c, in_cols, X, 257, 3).cpu().numpy()
    head = affine(W[:, :256], c, in_cols[:256], X, 257, 3).cpu().numpy()
    assert np.isfinite(full).all() and np.array_equal(full, head)


def test_affine_writes_its_window_only(gpu):
    """ld_out > n_rows through the ABI: nothing outside [j ld_out, j ld_out + n_rows) is written."""
    import torch

    from pgmpy_amd import _native as N

    n_in, n_out, n_rows, row0, ld_out = 257, 5, 257, 3, 300
    W, c, in_cols, host = LC.affine_case(n_in, n_out, n_rows, row0)
    X = _dev(host)
    out = torch.full((n_out + 1, ld_out), -7.0, dtype=torch.float64, device="cuda")
    cols = (ctypes.c_int32 * n_in)(*in_cols)
    dW, dc = _dev(W.reshape(-1)), _dev(c)
    N.check(N.lib().pgm_lg_affine(N.ptr(dW), N.ptr(dc), cols, n_in, n_out, N.ptr(X), host.shape[0],
                                  host.shape[1], row0, n_rows, N.ptr(out), ld_out, N.stream_handle()), "lg_affine")
    got = out.cpu().numpy()
    want, bound = LC.affine_ld(W, c, in_cols, host[:, row0:row0 + n_rows])
    assert LC.worst_ratio(got[:n_out, :n_rows], want, bound) <= 1.0
    assert (got[:n_out, n_rows:] == -7.0).all() and (got[n_out] == -7.0).all()


# ---------------------------------------------------------------------- 5. the net kernels on synthetic plans
NET = {c["name"]: c for c in LC.net_cases()}
SEED = 77


def _net_coef(case):
    from pgmpy_amd.models._lg import NetPlan

    plan = NetPlan(case["families"])
    return plan, _dev(plan.coef(case["betas"], case["stds"]))


@pytest.mark.parametrize("name", list(NET))
def test_net_sample(gpu, capsys, name):
    """n = 1 and n_big rows, at row0 0 and 3 of a NaN-filled buffer, from stream rows 0, 2^33 + 5 and the last the
    ABI takes: against sample_ld under its bound with the recorded U_Z_DEVICE.  Rows outside the window and columns
    no family names keep their NaN."""
    import torch

    case = NET[name]
    plan, coef = _net_coef(case)
    assert plan.info.max_parents == max(len(f) - 1 for f in case["families"])
    named = sorted({c for f in case["families"] for c in f})
    blank = [c for c in range(case["n_cols"]) if c not in named]
    assert (name == "gaps") == bool(blank) and (name != "gaps" or blank == [4, 5, 10, 11])
    worst = 0.0
    for n in (1, case["n_big"]):
        for first_row in LC.net_first_rows(n):
            want, bound = LC.net_sample(case, n, first_row, SEED)
            for row0 in (0, 3):
                X = torch.full((case["n_cols"], case["ld"]), float("nan"), dtype=torch.float64, device="cuda")
                plan.sample(coef, X, n, row0, first_row, SEED)
                got = X.cpu().numpy()
                assert np.isnan(got[:, :row0]).all() and np.isnan(got[:, row0 + n:]).all() and np.isnan(got[blank]).all()
                ratio = LC.worst_ratio(got[named, row0:row0 + n], want[named], bound[named])
                assert ratio <= 1.0, (name, n, first_row, row0, ratio)
                worst = max(worst, ratio)
    _report(capsys, f"k_lg_sample {name}", worst)


@pytest.mark.parametrize("name", list(NET))
def test_net_logpdf(gpu, capsys, name):
    """The density of the fp64 rounding of the restated sample: per row under logpdf_ld's bound, the total within
    the row-sum term, and a window at row0 = 1 bit-identical to the same rows of the full call."""
    case = NET[name]
    plan, coef = _net_coef(case)
    host, lp, bound = LC.net_logpdf(case)
    n = host.shape[1]
    stds = np.array(case["stds"])
    konst = _dev(-np.log(stds) - 0.5 * np.log(2 * np.pi))
    X = _dev(host)
    logp, total = plan.logpdf(coef, konst, X)
    full = logp.cpu().numpy()
    ratio = LC.worst_ratio(full, lp, bound)
    assert ratio <= 1.0, (name, ratio)
    tol = bound.sum() + n * LC.U * float(np.abs(lp).sum(dtype=LD))
    assert abs(float(total.cpu()[0]) - float(lp.sum(dtype=LD))) <= tol
    for n_rows in (1, n - 1):
        part, tot = plan.logpdf(coef, konst, X, n_rows, 1)
        assert np.array_equal(part.cpu().numpy(), full[1:1 + n_rows])
        want = lp[1:1 + n_rows].sum(dtype=LD)
        tol = bound[1:1 + n_rows].sum() + n_rows * LC.U * float(np.abs(lp[1:1 + n_rows]).sum(dtype=LD))
        assert abs(float(tot.cpu()[0]) - float(want)) <= tol
    _report(capsys, f"k_lg_logpdf {name}", ratio)


def test_logpdf_sum_strided_loop(gpu, capsys):
    """65,537 + 300 rows are 258 workgroup partials: work-items 0 and 1 of k_lg_logpdf_sum take their loop twice."""
    from pgmpy_amd import _native as N
    from pgmpy_amd.models._lg import NetPlan

    n = 65537 + 300
    assert N.LG_BLOCK < (n + N.LG_BLOCK - 1) // N.LG_BLOCK < 2 * N.LG_BLOCK
    fams, betas, stds = [[0], [1, 0]], [np.array([1.5]), np.array([-2.0, 0.75])], [2.0, 0.5]
    host = LC.sample_ld(fams, betas, stds, n, 9)[0].astype(np.float64)
    lp, bound = LC.logpdf_ld(host, fams, betas, stds)
    plan = NetPlan(fams)
    konst = _dev(-np.log(np.array(stds)) - 0.5 * np.log(2 * np.pi))
    logp, total = plan.logpdf(_dev(plan.coef(betas, stds)), konst, _dev(host))
    ratio = LC.worst_ratio(logp.cpu().numpy(), lp, bound)
    assert ratio <= 1.0
    tol = bound.sum() + n * LC.U * float(np.abs(lp).sum(dtype=LD))
    err = abs(float(total.cpu()[0]) - float(lp.sum(dtype=LD)))
    assert err <= tol
    # the bound is loose by its factor n: it must still see the last two partials missing
    assert abs(float(lp[256 * N.LG_BLOCK:].sum(dtype=LD))) > tol
    _report(capsys, "k_lg_logpdf_sum 258 partials (total)", err / tol)


# ---------------------------------------------------------------------- 6. the public API at width
FIT_ROWS = 512


@pytest.fixture(scope="module")
def wide():
    """(model, nodes, X device [300, FIT_ROWS] of simulate_values, its download)."""
    m = LC.wide_model()
    X = m.simulate_values(FIT_ROWS, seed=41)
    return m, list(m.nodes()), X, X.cpu().numpy()


def test_wide_simulate_and_fit(gpu, capsys, wide):
    m, nodes, X, host = wide
    _, fams, betas, stds = LC.model_families(m, nodes)
    want, bound = LC.sample_ld(fams, betas, stds, FIT_ROWS, 41, n_cols=len(nodes))
    ratio = LC.worst_ratio(host, want, bound)
    assert ratio <= 1.0
    idx = list(range(len(nodes)))
    shift = LC.colmean(host, idx)
    Gm, _ = LC.gram_ld(host, idx, shift)
    fitted = LC.build_model({"nodes": nodes, "edges": list(m.edges())})
    ref, cond = [], {}
    for v in nodes:
        P = [nodes.index(u) for u in fitted.get_parents(v)]
        beta, std = LC.finish_ld(Gm, shift, nodes.index(v), P, "unbiased")
        ref.append({"variable": v, "evidence": fitted.get_parents(v), "beta": beta.astype(np.float64), "std": float(std)})
        cond[v] = {"kappa": LC.family_condition(Gm, shift, nodes.index(v), P)[0]}  # from the long-double Gram, not the result
    fitted.fit_values(X, nodes)
    LC.check_fit(fitted.cpds, ref, host, nodes, "unbiased", cond)
    _report(capsys, "simulate_values, 300 nodes (fit_values passed check_fit at kappa up to "
            f"{max(c['kappa'] for c in cond.values()):.3g})", ratio)


def test_wide_log_likelihood(gpu, capsys, wide):
    m, nodes, X, host = wide
    _, fams, betas, stds = LC.model_families(m, nodes)
    lp, bound = LC.logpdf_ld(host, fams, betas, stds)
    logp, total = m.log_likelihood_values(X, nodes)
    ratio = LC.worst_ratio(logp.cpu().numpy(), lp, bound)
    assert ratio <= 1.0
    assert abs(total - float(lp.sum(dtype=LD))) <= bound.sum() + FIT_ROWS * LC.U * float(np.abs(lp).sum(dtype=LD))
    _report(capsys, "log_likelihood_values, 300 nodes", ratio)


def test_wide_predict(gpu, capsys, wide):
    """280 observed columns are two affine launches; the 20 columns of the missing variables hold NaN."""
    import networkx as nx

    m, nodes, X, host = wide
    rng = np.random.default_rng(5)
    seen = set(int(i) for i in rng.permutation(len(nodes))[:280])
    columns = [v if i in seen else f"unnamed {i}" for i, v in enumerate(nodes)]
    host = host.copy()
    host[[i for i in range(len(nodes)) if i not in seen]] = np.nan
    missing, mu, cov_cond = m.predict_values(_dev(host), columns)
    mv, ov, W, c, _ = m._conditional([v for v in columns if v in m.nodes()])
    assert missing == mv and len(ov) == 280 and mu.shape == (20, FIT_ROWS)
    want, bound = LC.affine_ld(W, c, [columns.index(v) for v in ov], host)
    ratio = LC.worst_ratio(mu.cpu().numpy(), want, bound)
    assert ratio <= 1.0
    _, cov = m.to_joint_gaussian()
    order = list(nx.topological_sort(m))
    a, b = [order.index(v) for v in mv], [order.index(v) for v in ov]
    kappa = np.linalg.cond(cov)
    assert np.allclose(W @ cov[np.ix_(b, b)], cov[np.ix_(a, b)], rtol=64 * LC.U * kappa, atol=64 * LC.U * kappa)
    _report(capsys, "predict_values, 280 observed columns", ratio)


def test_wide_simulate_with_evidence(gpu, wide):
    """One variable observed: the other 299 are drawn as a dense chain, the last node on 298 parents."""
    m, nodes, _, _ = wide
    mean, cov = m.to_joint_gaussian()
    import networkx as nx

    order = list(nx.topological_sort(m))
    v = order[150]
    val = float(mean[150] + np.sqrt(cov[150, 150]))
    drawn, _, W, c, cov_cond = m._conditional([v])
    n = 65536
    df = m.simulate(n, evidence={v: val}, seed=1234)
    assert sorted(df.columns) == sorted(order) and (df[v] == val).all() and len(drawn) == 299
    _assert_distribution(df[drawn].to_numpy().T, c + W @ np.array([val]), cov_cond)


# ---------------------------------------------------------------------- 7. Schur jobs over a wide G
def _wide_jobs():
    """(pcorr jobs with an intercept, pcorr jobs without, score jobs) over d = 150: K and the targets take positions from
    the three super-tiles [0, 64), [64, 128), [128, 150]; |K| counts the ones column (position d) where K holds it."""
    d = 150
    pool = [140, 3, 70, 129, 66, 149, 10, 127, 128, 64, 63, 0, 135, 100, 20, 145, 90, 40, 131, 77]
    with_icpt, without, scores = [], [], []
    for k in (1, 7, 8, 20):  # |K| with the ones column: lane path up to 7, wave path from 8
        Z = pool[:k - 1]
        with_icpt.append(LGS.pcorr_job(Z, 130, 65, d, True))
        with_icpt.append(LGS.pcorr_job(Z, 5, 148, d, True))
        scores.append(LGS.score_job(Z, 148, d))
        scores.append(LGS.score_job(Z, 65, d))
    for k in (0, 7, 8):  # no ones column in K: |K| = 0 exists in this form only
        without.append(LGS.pcorr_job(pool[:k], 130, 65, d))
        without.append(LGS.pcorr_job(pool[:k], 5, 148, d))
    return with_icpt, without, scores


def test_schur_jobs_over_wide_gram(gpu, capsys):
    """G is what k_lg_gram_reduce wrote for six groups.  One pcorr batch with an intercept and one bic batch at
    |K| = 1, 7, 8, 20; |K| = 0 cannot hold the ones column, so it runs (with 7 and 8) in a batch without an intercept,
    where position d is the third target.  kappa comes from job_condition on the host data."""
    from tests.test_lgs_gpu import _moments, _run

    d = 150
    X = LGS.dense_data(d, seed=150)
    shift = LGS.shift_of(X)
    G, dshift = _moments(X)
    got, want, A = G.cpu().numpy(), *LC.gram_ld(X, list(range(d)), shift)
    worst_g = _check_gram(got, want, LC.gram_bound(A, X.shape[1]), "d150")
    with_icpt, without, scores = _wide_jobs()
    worst = 0.0
    for jobs, kind, icpt in ((with_icpt, None, True), (without, None, False), (scores, "bic", None)):
        out0, out1, rank = _run(d, jobs, G, dshift, kind, icpt)
        for i, (K, T) in enumerate(jobs):
            kappa = LGS.job_condition(X, shift, K)
            if kind is None:
                ref, tol = LGS.pcorr_ld(X, K, T), LGS.pcorr_bound(X, shift, K, T, kappa)
            else:
                ref, tol = LGS.score_ld(X, K, T, kind)[:2], LGS.score_bound(X, shift, K, T, kappa)
            assert rank[i] == len(K)
            r = max(abs(out0[i] - ref[0]) / tol[0], abs(out1[i] - ref[1]) / tol[1])
            assert r <= 1.0, (K, T, kind, r)
            worst = max(worst, r)
    _report(capsys, f"k_lgs_lane / k_lgs_wave over G of d = 150 (G itself {worst_g:.3f})", worst)
