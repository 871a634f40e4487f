"""Linear-Gaussian networks without a GPU: the long-double restatement and the package's own host arithmetic
against the goldens of the reference, CPD strings and random CPDs, the container's errors and graph surgery,
the evidence conversion, and the validation and geometry of the two plan handles through ctypes (no device
call)."""
import ctypes
from types import SimpleNamespace

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import lg_cases as LC

G, _NPZ = LC.golden()
MODELS = sorted(G["models"])
LD = np.longdouble


def _matrix(df):
    return np.ascontiguousarray(df.to_numpy(dtype=np.float64).T)


def _restated_cpds(spec_nodes, spec_edges, df, est):
    """The fit of the restatement: long-double Gram at the column means, normal equations in long double."""
    cols = list(df.columns)
    X = _matrix(df)
    idx = list(range(len(cols)))
    shift = LC.colmean(X, idx)
    Gm, _ = LC.gram_ld(X, idx, shift)
    parents = {v: [u for u, w in spec_edges if w == v] for v in spec_nodes}
    out = []
    for v in spec_nodes:
        beta, std = LC.finish_ld(Gm, shift, cols.index(v), [cols.index(u) for u in parents[v]], est)
        out.append(SimpleNamespace(variable=v, beta=beta.astype(np.float64), std=float(std), evidence=parents[v]))
    return out, Gm, shift


def _package_cpds(spec, df, est, Gm, shift):
    """The package's host finish (models/_lg.py) on the fp64 rounding of the restated Gram matrix."""
    m = LC.build_model({"nodes": spec["nodes"], "edges": spec["edges"]})
    cols = list(df.columns)
    nodes = list(m.nodes())
    sel = [cols.index(v) for v in nodes] + [len(cols)]
    return m._finish_fit(nodes, Gm[np.ix_(sel, sel)].astype(np.float64), shift[[cols.index(v) for v in nodes]], est)


# ---------------------------------------------------------------------- goldens
@pytest.mark.parametrize("est", ["unbiased", "mle"])
@pytest.mark.parametrize("name", MODELS)
def test_fit_matches_reference(name, est):
    case = G["models"][name]
    df = LC.frame(name)
    restated, Gm, shift = _restated_cpds(case["nodes"], case["edges"], df, est)
    LC.check_fit(restated, case["fit"][est], _matrix(df), list(df.columns), est, case["fit"]["condition"])
    LC.check_fit(_package_cpds(case, df, est, Gm, shift), case["fit"][est], _matrix(df), list(df.columns), est,
                 case["fit"]["condition"])


@pytest.mark.parametrize("est", ["unbiased", "mle"])
def test_fit_shifted(est):
    df = LC.derived_frame("shifted")
    spec = G["models"]["chain3"]
    restated, Gm, shift = _restated_cpds(spec["nodes"], spec["edges"], df, est)
    LC.check_fit(restated, G["shifted"][est], _matrix(df), list(df.columns), est, G["shifted"]["condition"])
    LC.check_fit(_package_cpds(spec, df, est, Gm, shift), G["shifted"][est], _matrix(df), list(df.columns), est,
                 G["shifted"]["condition"])


def test_raw_moments_lose_the_shifted_case():
    """The case keeps its teeth: an fp64 raw-moment Gram of the shifted frame does NOT reproduce S_x2x2."""
    df = LC.derived_frame("shifted")
    X = _matrix(df)
    n = X.shape[1]
    j = list(df.columns).index("x2")
    raw = float(X[j] @ X[j]) - float(X[j].sum()) ** 2 / n
    Gm, A = LC.gram_ld(X, [j], LC.colmean(X, [j]))
    _, _, S = LC.moments_ld(Gm, LC.colmean(X, [j]))
    assert abs(raw - float(S[0, 0])) > 1e4 * float(LC.gram_bound(A, n)[0, 0])


def check_twins(cpds, est):
    ref = {c["variable"]: c for c in G["twins"]["fit"][est]}
    got = {c.variable: c for c in cpds}
    r2, g2 = ref["x2"], got["x2"]
    assert list(g2.evidence) == r2["evidence"]
    n = G["n_rows"]
    tol = LC.coef_rtol(n, 2, 1.0) + 256 * LC.U
    total = r2["beta"][1] + r2["beta"][2]
    assert abs(g2.beta[1] + g2.beta[2] - total) <= tol * abs(total)
    for i in (1, 2):  # the minimum-norm split: equal halves
        assert abs(g2.beta[i] - r2["beta"][i]) <= tol * abs(total)
    assert abs(g2.beta[0] - r2["beta"][0]) <= tol * (abs(r2["beta"][0]) + abs(total) * 8)
    assert abs(g2.std - r2["std"]) <= 4 * tol * r2["std"]
    for v in ("x1", "x1b"):
        assert abs(got[v].std - ref[v]["std"]) <= 4 * tol * ref[v]["std"]


@pytest.mark.parametrize("est", ["unbiased", "mle"])
def test_fit_twins_min_norm(est):
    df = LC.derived_frame("twins")
    spec = G["twins"]["spec"]
    cols = list(df.columns)
    X = _matrix(df)
    idx = list(range(len(cols)))
    shift = LC.colmean(X, idx)
    Gm, _ = LC.gram_ld(X, idx, shift)
    check_twins(_package_cpds(spec, df, est, Gm, shift), est)


@pytest.mark.parametrize("est", ["unbiased", "mle"])
def test_fit_two_rows_and_one_row(est):
    df = LC.derived_frame("tworows")
    spec = G["models"]["chain3"]
    restated, Gm, shift = _restated_cpds(spec["nodes"], spec["edges"], df, est)
    LC.check_fit(_package_cpds(spec, df, est, Gm, shift), G["tworows"][est], _matrix(df), list(df.columns), est)
    one = LC.derived_frame("onerow")
    _, Gm, shift = _restated_cpds(["x1"], [], one, est)
    cpds = _package_cpds(G["onerow"]["spec"], one, est, Gm, shift)
    ref = G["onerow"]["fit"][est][0]
    assert cpds[0].beta[0] == ref["beta"][0]
    assert (np.isnan(cpds[0].std) and np.isnan(ref["std"])) or cpds[0].std == ref["std"]
    if est == "unbiased":
        assert np.isnan(ref["std"])  # ddof 1 on one row, as pandas


@pytest.mark.parametrize("name", MODELS)
def test_to_joint_gaussian(name):
    case = G["models"][name]
    m = LC.build_model(case)
    assert list(m.nodes()) == case["nodes"]
    assert list(nx.topological_sort(m)) == case["order"]
    mean, cov = m.to_joint_gaussian()
    assert np.array_equal(mean, np.array(case["mean"])) and np.array_equal(cov, np.array(case["cov"]))


@pytest.mark.parametrize("name", MODELS)
def test_predict_formulas(name):
    """The host part of predict (W, c, cov_cond) and the long-double affine map against the reference."""
    case = G["models"][name]
    m = LC.build_model(case)
    df = LC.frame(name).iloc[:8]
    for rec in case["predict"]:
        part = df.drop(columns=rec["missing"])
        mv, ov, W, c, cov_cond = m._conditional(part.columns)
        assert mv == rec["variables"]
        mu, bound = LC.affine_ld(W, c, list(range(len(ov))), _matrix(part[ov]))
        ref = np.array(rec["mu"]).T
        kappa = np.linalg.cond(np.array(case["cov"]))
        assert (np.abs(mu.astype(np.float64) - ref) <= bound + 64 * LC.U * kappa * (np.abs(ref) + 1)).all()
        assert np.allclose(cov_cond, np.array(rec["cov"]), rtol=64 * LC.U * kappa, atol=64 * LC.U * kappa)


@pytest.mark.parametrize("name", MODELS)
def test_log_likelihood_restatement(name):
    """The factorised long-double density equals the reference's joint logpdf within the host bound:
    scipy's eigendecomposition of cov costs d kappa(cov) u relative to the sum of the rows' |terms|."""
    case = G["models"][name]
    m = LC.build_model(case)
    df = LC.frame(name)
    cols = list(df.columns)
    _, fams, betas, stds = LC.model_families(m, cols)
    lp, _ = LC.logpdf_ld(_matrix(df), fams, betas, stds)
    total = float(lp.sum(dtype=LD))
    assert abs(total - case["log_likelihood"]) <= host_ll_bound(case, lp)


def host_ll_bound(case, lp):
    d = len(case["nodes"])
    return 4 * d * case["kappa_cov"] * LC.U * float(np.abs(lp).sum(dtype=LD))


# ---------------------------------------------------------------------- CPDs
def test_cpd_strings_and_accessors():
    from pgmpy_amd.factors.continuous import LinearGaussianCPD

    for rec in G["strings"]:
        c = rec["cpd"]
        cpd = LinearGaussianCPD(c["variable"], c["beta"], c["std"], c["evidence"])
        assert str(cpd) == rec["str"]
        assert repr(cpd).startswith(f"<LinearGaussianCPD: {rec['str']} at 0x")
        k = cpd.copy()
        assert k is not cpd and k.variable == cpd.variable and k.evidence == cpd.evidence and k.evidence is not cpd.evidence
        assert np.array_equal(k.beta, cpd.beta) and k.std == cpd.std and k.variables == [c["variable"]] + c["evidence"]
    with pytest.raises(ValueError, match="must be hashable"):
        LinearGaussianCPD(["x"], [1], 1)


def test_get_random_values():
    from pgmpy_amd.factors import LinearGaussianCPD
    from pgmpy_amd.models import LinearGaussianBayesianNetwork

    r = G["cpd_get_random"]
    c = LinearGaussianCPD.get_random(r["variable"], r["evidence"], loc=r["loc"], scale=r["scale"], seed=r["seed"])
    assert c.beta.tolist() == r["beta"] and c.std == r["std"] and c.evidence == r["evidence"]
    # the reference's graph is drawn without the seed; its CPDs are a function of (graph, seed)
    rec = G["get_random"]
    m = LinearGaussianBayesianNetwork()
    m.add_nodes_from(rec["nodes"])
    m.add_edges_from(map(tuple, rec["edges"]))
    for got, ref in zip(m.get_random_cpds(seed=rec["seed"]), rec["cpds"]):
        assert got.variable == ref["variable"] and got.evidence == ref["evidence"]
        assert got.beta.tolist() == ref["beta"] and got.std == ref["std"]
    rnd = LinearGaussianBayesianNetwork.get_random(n_nodes=5, seed=rec["seed"])
    assert len(rnd.nodes()) == 5 and rnd.check_model() and len(rnd.cpds) == 5
    for i, v in enumerate(rnd.nodes()):
        ref = LinearGaussianCPD.get_random(v, rnd.get_parents(v), seed=rec["seed"] + i)
        assert np.array_equal(rnd.get_cpds(v).beta, ref.beta) and rnd.get_cpds(v).std == ref.std
    assert rnd.get_random_cpds(inplace=True) is None


# ---------------------------------------------------------------------- container
def _chain():
    return LC.build_model(G["models"]["chain3"])


def test_container_errors():
    from pgmpy_amd.factors.continuous import LinearGaussianCPD
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.models import LinearGaussianBayesianNetwork

    m = _chain()
    with pytest.raises(ValueError, match="Only LinearGaussianCPD can be added."):
        m.add_cpds(TabularCPD("x1", 2, [[0.5], [0.5]]))
    with pytest.raises(ValueError, match="CPD defined on variable not in the model"):
        m.add_cpds(LinearGaussianCPD("q", [0], 1))
    with pytest.raises(ValueError, match="Node not present in the Directed Graph"):
        m.get_cpds("q")
    with pytest.raises(ValueError, match="Cardinality is not defined for continuous variables."):
        m.get_cardinality("x1")
    with pytest.raises(NotImplementedError):
        m.to_markov_model()
    with pytest.raises(NotImplementedError):
        m.is_imap(None)
    bad = LinearGaussianBayesianNetwork([("x1", "x2")])
    bad.add_cpds(LinearGaussianCPD("x1", [0], 1), LinearGaussianCPD("x2", [0], 1))
    with pytest.raises(ValueError, match="CPD associated with x2 doesn't have proper parents associated with it."):
        bad.check_model()
    with pytest.raises(ValueError, match="can't be in both do and evidence: x2"):
        m.simulate(3, do={"x2": 0.0}, evidence={"x2": 1.0})
    with pytest.raises(ValueError, match="do-nodes are not present in the model: {'q'}"):
        m.simulate(3, do={"q": 0.0})
    with pytest.raises(ValueError, match="evidence-nodes are not present in the model: {'q'}"):
        m.simulate(3, evidence={"q": 0.0})
    with pytest.raises(ValueError, match="Virtual intervention provided for variable which is not in the model: q"):
        m.simulate(3, virtual_intervention=[LinearGaussianCPD("q", [0], 1)])
    with pytest.raises(ValueError, match="No missing variables in the data"):
        m.predict(pd.DataFrame({"x1": [0.0], "x2": [0.0], "x3": [0.0]}))
    with pytest.raises(ValueError, match="Following variables are missing in the data: {'x3'}"):
        m.fit(pd.DataFrame({"x1": [0.0], "x2": [0.0]}))
    full = pd.DataFrame({"x1": [0.0], "x2": [0.0], "x3": [0.0]})
    with pytest.raises(ValueError, match="estimator must be one of"):
        m.fit(full, estimator="bayes")
    with pytest.raises(ValueError, match="std_estimator must be one of"):
        m.fit(full, std_estimator="x")
    with pytest.raises(ValueError, match="Missing required columns in DataFrame: {'x3'}"):
        m.log_likelihood(pd.DataFrame({"x1": [0.0], "x2": [0.0]}))


def test_container_methods():
    m = _chain()
    assert [c.variable for c in m.get_cpds()] == ["x1", "x2", "x3"] and m.get_cpds("x2").evidence == ["x1"]
    k = m.copy()
    assert list(k.nodes()) == list(m.nodes()) and list(k.edges()) == list(m.edges()) and len(k.cpds) == 3
    assert k.cpds[0] is not m.cpds[0] and k.latents == m.latents
    m.remove_cpds("x3", m.get_cpds("x2"))
    assert [c.variable for c in m.cpds] == ["x1"] and len(k.cpds) == 3
    from pgmpy_amd.factors.continuous import LinearGaussianCPD

    m.add_cpds(LinearGaussianCPD("x1", [7], 2))
    assert len(m.cpds) == 1 and m.get_cpds("x1").beta[0] == 7
    with pytest.raises(ValueError, match="Loops are not allowed"):
        k.add_edge("x3", "x1")


def test_graph_surgery():
    from pgmpy_amd.factors.continuous import LinearGaussianCPD

    m = _chain()
    d = m._intervened({"x2": 2.0}, [])
    assert sorted(d.nodes()) == ["x1", "x3"] and not list(d.edges())
    c3 = d.get_cpds("x3")
    assert c3.evidence == [] and c3.beta.tolist() == [4 + (-1) * 2.0] and c3.std == 3
    assert len(m.get_cpds("x3").beta) == 2  # the model itself is untouched
    v = m._intervened({}, [LinearGaussianCPD("x2", [9], 0.5)])
    assert list(v.edges()) == [("x2", "x3")] and v.get_cpds("x2").beta.tolist() == [9] and v.check_model()
    mean, cov = v.to_joint_gaussian()
    assert dict(zip(nx.topological_sort(v), mean)) == {"x1": 1.0, "x2": 9.0, "x3": -5.0}
    m5 = LC.build_model(G["models"]["collider5"])
    d5 = m5._intervened({"c": 1.0}, [])
    assert d5.get_cpds("e").evidence == ["b"] and d5.get_cpds("e").beta.tolist() == [-0.5 + (-1) * 1.0, 0.5]
    assert d5.get_cpds("d").beta.tolist() == [3.0] and d5.check_model()


@pytest.mark.parametrize("name", MODELS)
def test_evidence_chain_reproduces_the_conditional(name):
    case = G["models"][name]
    m = LC.build_model(case)
    ev = case["evidence"]
    drawn, chain = m._evidence_chain(ev["evidence"])
    assert drawn == ev["variables"] and list(chain.nodes()) == drawn and chain.check_model()
    assert list(nx.topological_sort(chain)) == drawn
    mean, cov = chain.to_joint_gaussian()
    ref_m, ref_c = np.array(ev["mean"]), np.array(ev["cov"])
    assert np.abs(mean - ref_m).max() <= 1e-12 * np.abs(ref_m).max()
    assert np.abs(cov - ref_c).max() <= 1e-12 * np.abs(ref_c).max()


# ---------------------------------------------------------------------- the C-ABI without a device
@pytest.fixture(scope="module")
def lib():
    from pgmpy_amd import _native as N

    return N.load_library()


def test_symbols_and_structs(lib):
    from pgmpy_amd import _native as N

    assert lib.pgm_version() == 25
    names = ["pgm_lg_gram_plan_create", "pgm_lg_gram_plan_destroy", "pgm_lg_gram_plan_info", "pgm_lg_gram_plan_set_slice",
             "pgm_lg_gram_info", "pgm_lg_colsum", "pgm_lg_gram", "pgm_lg_net_create", "pgm_lg_net_destroy", "pgm_lg_net_info",
             "pgm_lg_sample", "pgm_lg_logpdf", "pgm_lg_affine"]
    for name in names:
        assert name in N.EXPORTED and getattr(lib, name).argtypes is not None
    assert ctypes.sizeof(N.LgGramInfo) == 64 and ctypes.sizeof(N.LgNetInfo) == 24
    assert (N.LG_TILE, N.LG_SUPER, N.LG_ROWS_PER_LANE, N.LG_STEP) == (16, 4, 4, 16)
    assert N.LG_STEP == 4 * N.LG_ROWS_PER_LANE


@pytest.mark.parametrize("d1,tiles,supers,groups,single", [(1, 1, 1, 1, 1), (16, 1, 1, 1, 1), (17, 2, 1, 1, 1), (64, 4, 1, 1, 1),
                                                            (65, 5, 2, 3, 0), (130, 9, 3, 6, 0)])
def test_gram_geometry(d1, tiles, supers, groups, single):
    from pgmpy_amd import _native as N
    from pgmpy_amd.models._lg import GramPlan

    p = GramPlan(list(range(d1 - 1)))
    i = p.info
    assert (i.d, i.n_cols, i.n_tiles, i.n_super, i.n_groups, i.single_wave) == (d1 - 1, d1 - 1, tiles, supers, groups, single)
    assert i.n_tile_pairs == tiles * (tiles + 1) // 2 and i.out_size == d1 * d1
    assert p.groups() == [(I, J) for I in range(supers) for J in range(I, supers)]
    assert i.max_slices == max(4, N.LG_TARGET_BLOCKS // groups)
    # the automatic slice: one slice up to LG_SLICE_MIN rows, then about LG_TARGET_BLOCKS waves
    assert p.gram_info(1) == (N.LG_SLICE_MIN, 1, True) and p.gram_info(N.LG_SLICE_MIN + 1)[:2] == (N.LG_SLICE_MIN, 2)
    want = max(1, N.LG_TARGET_BLOCKS // groups)
    s, k, _ = p.gram_info(10_000_000)
    assert s % N.LG_STEP == 0 and k <= want and (k - 1) * s < 10_000_000 <= k * s
    # forced: rounded up to a step, and raised when the handle's partials would not hold the slices
    p.set_slice(1)
    assert p.info.slice_rows == 1 and p.gram_info(33)[:2] == (16, 3)
    s, k, _ = p.gram_info(16 * int(i.max_slices) + 1)
    assert s == 32 and k <= i.max_slices
    p.set_slice(0)
    assert p.gram_info(1)[0] == N.LG_SLICE_MIN


def test_gram_vec16_flag():
    from pgmpy_amd.models._lg import GramPlan

    p = GramPlan([0, 1])
    assert p.gram_info(100, x_ptr=4096, ld=128, row0=0)[2] is True
    assert p.gram_info(100, x_ptr=4096, ld=128, row0=2)[2] is True
    assert p.gram_info(100, x_ptr=4096, ld=128, row0=1)[2] is False
    assert p.gram_info(100, x_ptr=4096, ld=127, row0=0)[2] is False
    assert p.gram_info(100, x_ptr=4096 + 8, ld=128, row0=0)[2] is False


def test_plan_refusals(lib):
    from pgmpy_amd import _native as N
    from pgmpy_amd.models._lg import GramPlan, NetPlan

    with pytest.raises(ValueError, match="column 3 is listed twice"):
        GramPlan([3, 1, 3])
    with pytest.raises(ValueError, match="column -1"):
        GramPlan([0, -1])
    h = ctypes.c_void_p()
    assert lib.pgm_lg_gram_plan_create(None, 2, ctypes.byref(h)) == N.PGM_EINVAL
    assert lib.pgm_lg_gram_plan_create(None, 0, None) == N.PGM_EINVAL
    assert lib.pgm_lg_gram_plan_info(None, None, None) == N.PGM_EINVAL
    assert lib.pgm_lg_gram_plan_destroy(None) == N.PGM_OK and lib.pgm_lg_net_destroy(None) == N.PGM_OK
    with pytest.raises(ValueError, match="rows"):
        GramPlan([0]).set_slice(-1)

    NetPlan([[0], [1, 0], [2, 1, 0]])
    with pytest.raises(ValueError, match="parent column 1 is not the node of an earlier family"):
        NetPlan([[0, 1], [1]])  # a child before its parent (every cycle has one)
    with pytest.raises(ValueError, match="family 0 lists column 0 twice"):
        NetPlan([[0, 0]])  # its own parent
    with pytest.raises(ValueError, match="parent column 2 is not the node of an earlier family"):
        NetPlan([[0], [1, 2], [2, 1]])  # 1 -> 2 -> 1
    with pytest.raises(ValueError, match="column 0 is the node of families 0 and 1"):
        NetPlan([[0], [0]])
    with pytest.raises(ValueError, match="lists column 0 twice"):
        NetPlan([[0], [1, 0, 0]])
    many = N.LG_MAX_PARENTS + 1
    NetPlan([[c] for c in range(many - 1)] + [[many - 1] + list(range(many - 1))])
    with pytest.raises(ValueError, match=f"has {many} parents"):
        NetPlan([[c] for c in range(many)] + [[many] + list(range(many))])
    assert lib.pgm_lg_net_create(None, None, 1, ctypes.byref(h)) == N.PGM_EINVAL
    with pytest.raises(ValueError, match="0 families"):
        NetPlan([])
    p = NetPlan([[2], [0, 2], [1, 0, 2]])
    assert (p.info.n_families, p.info.n_cols, p.info.max_parents, p.n_coef) == (3, 3, 2, 9) and p.coef_off == [0, 2, 5]
    assert p.coef([[1], [2, 3], [4, 5, 6]], [7, 8, 9]).tolist() == [1, 7, 2, 3, 8, 4, 5, 6, 9]


def test_launch_argument_checks(lib):
    """Every launch entry point refuses bad arguments, and accepts n_rows == 0, before any HIP call."""
    from pgmpy_amd import _native as N
    from pgmpy_amd.models._lg import GramPlan, NetPlan

    g, net = GramPlan([0, 2]), NetPlan([[0], [2, 0]])
    buf = np.zeros(64)
    x = ctypes.c_void_p(buf.ctypes.data)  # never dereferenced: the checks come first
    ib = (ctypes.c_int32 * 2)(0, 2)
    E = N.PGM_EINVAL

    def colsum(X=x, n_cols=3, ld=10, row0=0, n=0, sums=x, counts=x, plan=g._h):
        return lib.pgm_lg_colsum(plan, X, n_cols, ld, row0, n, sums, counts, None)

    def gram(X=x, n_cols=3, ld=10, row0=0, n=0, shift=x, out=x, plan=g._h):
        return lib.pgm_lg_gram(plan, X, n_cols, ld, row0, n, shift, out, None)

    def sample(X=x, n_cols=3, ld=10, row0=0, n=0, coef=x, first=0, plan=net._h):
        return lib.pgm_lg_sample(plan, coef, X, n_cols, ld, row0, n, first, 0, None)

    def logpdf(X=x, n_cols=3, ld=10, row0=0, n=0, coef=x, konst=x, logp=x, total=x, plan=net._h):
        return lib.pgm_lg_logpdf(plan, coef, konst, X, n_cols, ld, row0, n, logp, total, None)

    def affine(X=x, n_cols=3, ld=10, row0=0, n=0, W=x, c=x, cols=ib, n_in=2, n_out=1, out=x, ld_out=10):
        return lib.pgm_lg_affine(W, c, cols, n_in, n_out, X, n_cols, ld, row0, n, out, ld_out, None)

    for fn in (colsum, gram, sample, logpdf, affine):
        assert fn() == N.PGM_OK  # n_rows == 0: nothing is launched
        assert fn(X=None) == E
        assert fn(n=-1) == E and fn(row0=-1) == E
        assert fn(row0=8, n=3) == E and fn(row0=11) == E  # the window leaves ld
        assert fn(n_cols=2) == E  # the plan names column 2
    assert colsum(plan=None) == E and colsum(sums=None) == E and colsum(counts=None) == E
    assert gram(plan=None) == E and gram(shift=None) == E and gram(out=None) == E
    assert sample(plan=None) == E and sample(coef=None) == E and sample(first=-1) == E
    assert logpdf(plan=None) == E and logpdf(coef=None) == E and logpdf(konst=None) == E and logpdf(logp=None, total=None) == E
    assert logpdf(logp=None) == N.PGM_OK and logpdf(total=None) == N.PGM_OK
    assert logpdf(ld=1 << 40, n=N.LG_BLOCK * N.LG_MAX_BLOCKS + 1) == E
    assert affine(W=None) == E and affine(c=None) == E and affine(out=None) == E and affine(cols=None) == E
    assert affine(n_out=0) == E and affine(n_out=65536) == E and affine(ld_out=-1) == E
    assert affine(cols=(ctypes.c_int32 * 2)(0, -1)) == E
    assert "lg_affine" in N.last_error()


# ---------------------------------------------------------------------- the wide plans: host side and negative controls
@pytest.mark.parametrize("case", LC.net_cases(), ids=lambda c: c["name"])
def test_net_case_plans(case):
    """The handle's view of every synthetic plan of tests/test_lg_wide_gpu.py."""
    from pgmpy_amd import _native as N
    from pgmpy_amd.models._lg import NetPlan

    fams = case["families"]
    p = NetPlan(fams)
    assert p.info.n_families == len(fams) and p.info.n_cols == 1 + max(c for f in fams for c in f) <= case["n_cols"]
    assert p.info.max_parents == max(len(f) - 1 for f in fams) <= N.LG_MAX_PARENTS
    assert p.n_coef == sum(len(f) + 1 for f in fams)
    assert p.coef_off == [sum(len(g) + 1 for g in fams[:f]) for f in range(len(fams))]
    coef = p.coef(case["betas"], case["stds"])
    for f, fam in enumerate(fams):
        o = p.coef_off[f]
        assert np.array_equal(coef[o:o + len(fam)], case["betas"][f]) and coef[o + len(fam)] == case["stds"][f]
    assert {"max_parents": N.LG_MAX_PARENTS, "star_300": 300, "chain_300": 1, "dense_40": 39}.get(case["name"], p.info.max_parents) \
        == p.info.max_parents
    assert case["ld"] >= 3 + case["n_big"] + 1


def _exceeds(wrong, want, bound):
    return LC.worst_ratio(wrong.astype(np.float64), want, bound) > 1.0


def _gram_control(d, row0, n_rows, slice_rows, **kw):
    host, cols, shift = LC.gram_window(d, row0, n_rows, **kw)
    win = host[:, row0:row0 + n_rows]
    want, A = LC.gram_ld(win, cols, shift)
    bound = LC.gram_bound(A, n_rows)
    wrong = LC.gram_structural_errors(win, cols, shift, slice_rows)
    assert ("columns_16_apart_exchanged" in wrong) == (d >= 17)
    for name, E in wrong.items():
        assert _exceeds(E, want, bound), (name, d, row0, n_rows)


def test_gram_bound_sees_structural_errors():
    """The bounds carry a factor n: at every Gram shape of the wide tests a row left out, two columns of neighbouring
    tiles exchanged on one side, and a slice's partial dropped each lie outside gram_bound."""
    from pgmpy_amd import _native as N
    from pgmpy_amd.models._lg import GramPlan

    assert (LC.SLICE_MIN, LC.STEP) == (N.LG_SLICE_MIN, N.LG_STEP)
    for _, d, row0, n_rows, kw in LC.gram_wide_shapes():
        _gram_control(d, row0, n_rows, LC.SLICE_MIN, **kw)
    for d in (3, 200):
        p = GramPlan(list(range(d)))
        for kind, forced in (("auto", None), ("raised", 1)):
            n_rows = LC.slice_rows_of(kind, p.info.max_slices)
            p.set_slice(forced or 0)
            slice_rows, n_slices, _ = p.gram_info(n_rows)
            assert n_slices >= 2
            _gram_control(d, 2, n_rows, slice_rows, seed=d + n_rows, ld=n_rows + 7)


def test_affine_bound_sees_a_dropped_input():
    """Input 256, the first of the second launch, left out: outside affine_ld's bound wherever it exists."""
    for n_in in (n for n in LC.AFFINE_N_IN if n > 256):
        for n_out in LC.AFFINE_N_OUT:
            for n_rows in LC.AFFINE_ROWS:
                for row0 in (0, 3):
                    W, c, in_cols, host = LC.affine_case(n_in, n_out, n_rows, row0)
                    win = host[:, row0:row0 + n_rows]
                    want, bound = LC.affine_ld(W, c, in_cols, win)
                    wrong = want - np.outer(W[:, 256].astype(LD), win[in_cols[256]].astype(LD))
                    assert _exceeds(wrong, want, bound), (n_in, n_out, n_rows, row0)


@pytest.mark.parametrize("case", LC.net_cases(), ids=lambda c: c["name"])
def test_net_bounds_see_structural_errors(case):
    """The cosine where the sine belongs (every odd column, at every n and first_row of the GPU test) and one parent's
    term missing from the density: outside the bounds of sample_ld and logpdf_ld."""
    odd = sorted({f[0] for f in case["families"] if f[0] & 1})
    assert odd
    for n in (1, case["n_big"]):
        for first_row in LC.net_first_rows(n):
            want, bound = LC.net_sample(case, n, first_row)
            wrong, _ = LC.net_sample(case, n, first_row, wrong_trig=True)
            for c in odd:
                assert _exceeds(wrong[c], want[c], bound[c]), (case["name"], n, first_row, c)
    _, lp, bound = LC.net_logpdf(case)
    _, wrong, _ = LC.net_logpdf(case, drop_parent=True)
    assert (np.abs(wrong - lp).astype(np.float64) > bound).all()  # every row
