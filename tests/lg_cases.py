"""Linear-Gaussian networks restated in np.longdouble, independently of the C++ (pgmpy_amd/csrc/pgmlg.hip)
and of pgmpy_amd/models/_lg.py, the error bounds of the comparisons, and the fixtures the CPU and GPU tests
share (tests/golden/lg_cases.json + lg_cases.npz, made by tests/golden/make_golden_lg.py from the reference).

A value matrix is an fp64 ndarray X[n_cols, n_rows] (column-major like the device's).  u = 2^-53.

Gram.  The device forms a = fl(x - c) and b = fl(y - c') (one rounding each) and accumulates the products
in fp64 in some order (the MFMA's k slots, the row slices).  Against G_xy = sum_k (x_k - c)(y_k - c') in
long double, any order of n additions of once-rounded products of once-rounded factors gives
    |G^_xy - G_xy| <= (n + 2) u sum_k |a_k b_k|        (gram_bound; higher orders in u are below 1 %).
The ones column is exact, so an entry against it carries one factor rounding less (the bound still holds).

Coefficients.  S = G - g g' / n is formed in long double from the device's G.  Scale the parents to unit
diagonal: by Cauchy-Schwarz sum|a_k b_k| <= sqrt(G_xx G_yy), so every entry of the scaled S_pp and s_pv moves by at
most eps1 = 2 (n + 2) u (the factor 2: the correction term, whose g entries are bounded the same way), and the
p x p matrix by eps = p eps1 in norm.  With kappa the condition number of the scaled S_pp (RECORDED in the
golden from the reference's own frame, not recomputed from the result) the solution moves by
    ||db|| / ||b|| <= 2 eps kappa / (1 - eps kappa)  +  p u kappa                          (coef_rtol)
the second term being the host solve's own (fp64 eigendecomposition, refined once in long double).  It bounds the
scaled coefficient vector D b (D = sqrt(diag S_pp)) in norm; check_fit compares D_i |b_i - ref_i| against
r ||D b_ref||.  The intercept mean_v - b . mean_p is bounded in absolute terms: r ||D b|| sum_i |mean_i| / D_i for the
coefficients' share plus (p + 2) roundings of its own terms.  The variance rss / dof, with rss = S_vv - 2 b.s +
b'Sb, carries the perturbation of S_vv (eps1 S_vv) and a SECOND-order term in db (rss is minimal at b):
    |d var| <= ((eps1 + r^2) S_vv + r^2 rss) / dof,
an absolute bound that also covers an exact fit (rss = 0: the golden case tworows), where a relative one has no
meaning; S_vv / rss, recorded in the golden, is the factor by which this exceeds a relative bound on the std.
The reference's own numbers come from scikit-learn's fp64 lstsq on the frame it centres in fp64 and from residuals
it forms in fp64: its coefficients carry about sqrt(kappa) u and both carry u |mean| / sd when the data sits far from
0 (the case `shifted`); check_fit adds host = 64 u sqrt(kappa) (1 + max_j |mean_j| / sd_j) over the family for it.

logpdf.  Per node, with r = x_v - m, m = beta_0 + sum_i beta_i x_i, t = r / sigma and M = |x_v| + |beta_0| +
sum_i |beta_i x_i| the magnitude r is cancelled from: m costs at most 2 p roundings of terms within M (fused or
not), so |dr| <= 2 p u M + u |r|; the division, the square and the subtraction from k_v add 2.5 u more, and the
halving is exact: |d(t^2 / 2)| <= (2 p + 4) u t^2 (1 + M / |r|).  Adding the n_nodes terms in order costs
n_nodes u sum_v (|k_v| + t_v^2 / 2).  Both are below
    (2 p_max + 8 + n_nodes) u sum_v (|k_v| + t_v^2 (1 + M_v / |r_v|))                      (logpdf_ld's bound, per row);
a residual that is exactly 0 contributes (M_v / sigma_v)^2 in place of the undefined quotient.  The total adds
n u sum_rows |lp|.

Affine.  (n_in + 1) u (|c_j| + sum_i |W_ji x_i|).

Sampler.  z = rho cospi(2 u1) or rho sinpi(2 u1), rho = sqrt(-2 log(1 - u0)); 1 - u0 and 2 u1 are exact.
The device's error in z is U_Z ulps of z: log, sqrt, sincospi and two products.  It can only be observed as a
whole through the ABI (a root with beta_0 = 0, sigma = 1 writes z itself), so it is recorded as one figure:
U_Z_MEASURED = 3.245 ulp of z, the largest of 2^20 stream rows x 2 columns x 3 seeds on an MI355X (2026-10-20; the
mean is 0.61), and U_Z_DEVICE is its double because other seeds reach other arguments (as score_cases.U_DEVICE is
doubled).  The long-double side must itself be exact next to the zeros of the cosine and sine: sincospi_ld.
A node's value then carries
    dx_v <= sum_i |beta_i| dx_{p_i} + (p + 2) u (|beta_0| + sum_i |beta_i x_i| + |sigma z|) + U_Z u |sigma z|.

Wide plans.  The second half of this module builds the shapes of tests/test_lg_wide_gpu.py: Gram handles of three and
four super-tiles, the two sliced launches, affine maps of up to three launches, the net plans of net_cases (300-node
chain and star, 4,096 parents, every visiting order of a Philox pair, unnamed columns, a dense 40-node net) and a
300-node random model.  The bounds above are used as they stand: each scales with its own n, d or p, and at 4,096
parents no further term appeared (the worst error / bound of every family is recorded in that module's docstring).
Because the bounds carry a factor n they are loose on rounding; what the wide tests are for is structure, so every
shape has NEGATIVE CONTROLS on the CPU (tests/test_lg_cpu.py): the long-double result with one structural error (a row
left out, two columns 16 apart exchanged on one side, a slice's partial dropped; affine input 256 dropped; the cosine
where the sine belongs; one parent's term missing) must lie outside the bound of that shape.  The data carries offset
means and a shift that is not the window's own mean so that this holds down to a one-row window.
"""
import json
import os

import numpy as np

from tests import sample_cases as SC

LD = np.longdouble
U = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# measured (module docstring, Sampler); tests/test_lg_gpu.py::test_sampler_ulp prints the figure of its own run
U_Z_MEASURED = 3.245
U_Z_DEVICE = 2 * U_Z_MEASURED
PI_LD = LD("3.14159265358979323846264338327950288")


# ---------------------------------------------------------------------- fixtures
_CACHE = {}


def golden():
    if "json" not in _CACHE:
        with open(os.path.join(GOLDEN, "lg_cases.json")) as f:
            _CACHE["json"] = json.load(f)
        _CACHE["npz"] = dict(np.load(os.path.join(GOLDEN, "lg_cases.npz")))
    return _CACHE["json"], _CACHE["npz"]


def frame(name):
    """The recorded frame of a case as a DataFrame (columns in the recorded order)."""
    import pandas as pd

    g, z = golden()
    return pd.DataFrame(z[f"{name}_frame"], columns=g["frames"][name])


def derived_frame(name):
    """shifted / twins / tworows / onerow: built from chain3's frame exactly as make_golden_lg.py builds them."""
    df = frame("chain3")
    if name == "shifted":
        df = df.copy()
        df["x2"] = df["x2"] + 1e8
        return df
    if name == "twins":
        df = df[["x1", "x2"]].copy()
        df["x1b"] = df["x1"]
        return df
    if name == "tworows":
        return df.iloc[:2].copy()
    if name == "onerow":
        return df.iloc[:1][["x1"]].copy()
    raise KeyError(name)


def build_model(spec):
    """A pgmpy_amd LinearGaussianBayesianNetwork from a recorded {"nodes", "edges", "cpds"} (cpds optional)."""
    from pgmpy_amd.factors.continuous import LinearGaussianCPD
    from pgmpy_amd.models import LinearGaussianBayesianNetwork

    m = LinearGaussianBayesianNetwork()
    m.add_nodes_from(spec["nodes"])
    m.add_edges_from([tuple(e) for e in spec["edges"]])
    for c in spec.get("cpds", []):
        m.add_cpds(LinearGaussianCPD(c["variable"], c["beta"], c["std"], list(c["evidence"])))
    return m


# ---------------------------------------------------------------------- Gram
def gram_ld(X, cols, shift):
    """(G, A) [d + 1, d + 1] long double: G the Gram matrix of the columns x - c with the ones column last,
    A the same sums of |a_k b_k|."""
    X = np.asarray(X, dtype=np.float64)
    d, n = len(cols), X.shape[1]
    Z = np.ones((d + 1, n), dtype=LD)
    for j, c in enumerate(cols):
        Z[j] = X[c].astype(LD) - LD(shift[j])
    G = np.empty((d + 1, d + 1), dtype=LD)
    A = np.empty((d + 1, d + 1), dtype=LD)
    absZ = np.abs(Z)
    for j in range(d + 1):
        G[j] = (Z * Z[j][None, :]).sum(axis=1, dtype=LD)
        A[j] = (absZ * absZ[j][None, :]).sum(axis=1, dtype=LD)
    return G, A


def gram_bound(A, n):
    return (n + 2) * U * np.asarray(A, dtype=np.float64) * 1.01


def colmean(X, cols):
    """The fp64 shift a caller would use: the column means to within rounding."""
    return np.array([float(np.asarray(X[c], dtype=LD).sum(dtype=LD) / LD(X.shape[1])) for c in cols])


# ---------------------------------------------------------------------- the finish
def solve_ld(A, b):
    """Gaussian elimination with partial pivoting in long double."""
    A, b = np.array(A, dtype=LD), np.array(b, dtype=LD)
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            A[i, k:] -= f * A[k, k:]
            b[i] -= f * b[k]
    x = np.zeros(n, dtype=LD)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def moments_ld(G, shift):
    G = np.asarray(G, dtype=LD)
    d = G.shape[0] - 1
    n, g = G[d, d], G[:d, d]
    return n, np.asarray(shift, dtype=LD) + g / n, G[:d, :d] - np.outer(g, g) / n


def finish_ld(G, shift, v, parents, std_estimator):
    """(beta LD [1 + p], std LD) of node index v on `parents` by the normal equations in long double (parents
    must not be collinear)."""
    n, mean, S = moments_ld(G, shift)
    p = len(parents)
    b = solve_ld(S[np.ix_(parents, parents)], S[parents, v]) if p else np.zeros(0, dtype=LD)
    rss = S[v, v] - (b @ S[parents, v] if p else LD(0))
    dof = n - (0 if std_estimator == "mle" else 1 + p)
    std = np.sqrt(rss / dof) if dof > 0 else LD("nan")
    return np.concatenate([[mean[v] - (b @ mean[parents] if p else LD(0))], b]), std


def family_condition(G, shift, v, parents):
    """(kappa of the correlation-scaled centred parent Gram matrix, S_vv / rss) in fp64."""
    n, mean, S = moments_ld(G, shift)
    if not parents:
        return 1.0, 1.0
    Spp = S[np.ix_(parents, parents)].astype(np.float64)
    dg = np.sqrt(np.diag(Spp))
    w = np.linalg.eigvalsh(Spp / np.outer(dg, dg))
    b = solve_ld(S[np.ix_(parents, parents)], S[parents, v])
    rss = S[v, v] - b @ S[parents, v]
    return float(w[-1] / w[0]), float(S[v, v] / rss)


def coef_rtol(n, p, kappa):
    """The device path's share (module docstring, Coefficients)."""
    eps = p * 2 * (n + 2) * U
    return 2 * eps * kappa / (1 - eps * kappa) + p * U * kappa


def check_fit(cpds, ref_cpds, X, cols, std_estimator, cond=None):
    """Assert that `cpds` (objects with variable / beta / std / evidence) match the reference's recorded fit of
    the frame X[len(cols), n] within the bounds of the module docstring.  cond: the golden's recorded
    {variable: {kappa, svv_over_rss}}; the kappa recorded there is used, not one recomputed from the result."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[1]
    idx = list(range(len(cols)))
    shift = colmean(X, idx)
    G, _ = gram_ld(X, idx, shift)
    _, mean, S = moments_ld(G, shift)
    mean, S = mean.astype(np.float64), S.astype(np.float64)
    sd = np.sqrt(np.diag(S) / n)
    by_var = {c.variable: c for c in cpds}
    assert len(by_var) == len(ref_cpds)
    for ref in ref_cpds:
        got = by_var[ref["variable"]]
        assert list(got.evidence) == ref["evidence"], (got.evidence, ref["evidence"])
        v, P = cols.index(ref["variable"]), [cols.index(u) for u in ref["evidence"]]
        p = len(P)
        kappa = cond[ref["variable"]]["kappa"] if cond else 1.0
        assert np.isfinite(kappa)
        with np.errstate(divide="ignore", invalid="ignore"):
            off_centre = max(abs(mean[j]) / sd[j] if sd[j] > 0 else 0.0 for j in [v] + P)
        host = 64 * U * np.sqrt(kappa) * (1 + off_centre)
        r = coef_rtol(n, p, kappa) + host if p else host
        beta, beta_ref = np.asarray(got.beta, dtype=np.float64), np.asarray(ref["beta"], dtype=np.float64)
        assert beta.shape == beta_ref.shape
        D = np.sqrt(np.diag(S)[P])
        scale = float(np.linalg.norm(D * beta_ref[1:])) if p else 0.0
        if p:
            err = np.abs(beta[1:] - beta_ref[1:]) * D
            assert (err <= r * scale + 1e-300).all(), (ref["variable"], err / max(scale, 1e-300), r)
        mag = abs(mean[v]) + float(np.abs(beta_ref[1:] * mean[P]).sum())
        tol0 = r * scale * float((np.abs(mean[P]) / D).sum()) + (4 * (p + 2) * U + host) * max(mag, sd[v])
        assert abs(beta[0] - beta_ref[0]) <= tol0, (ref["variable"], abs(beta[0] - beta_ref[0]), tol0)
        dof = n - (0 if std_estimator == "mle" else 1 + p)
        if dof <= 0 or np.isnan(ref["std"]):
            assert np.isnan(got.std) and np.isnan(ref["std"]), (ref["variable"], got.std, ref["std"])
            continue
        var_ref = ref["std"] ** 2
        eps1 = 2 * (n + 2) * U
        tol = ((eps1 + r * r) * S[v, v] + r * r * var_ref * dof) / dof + (8 * U + host) * (var_ref + S[v, v] / dof * host)
        assert abs(got.std ** 2 - var_ref) <= tol, (ref["variable"], got.std, ref["std"], tol)


# ---------------------------------------------------------------------- log-density
def logpdf_ld(X, families, betas, stds):
    """(lp LD [n], bound fp64 [n]): families [[node col, parent cols ...]] in topological order."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[1]
    lp, mag = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    p_max = max(len(f) - 1 for f in families)
    for fam, beta, std in zip(families, betas, stds):
        beta = np.asarray(beta, dtype=np.float64).astype(LD)
        m = np.full(n, beta[0], dtype=LD)
        M = np.full(n, abs(beta[0]), dtype=LD) + np.abs(X[fam[0]]).astype(LD)
        for i, c in enumerate(fam[1:]):
            m = m + beta[1 + i] * X[c].astype(LD)
            M = M + np.abs(beta[1 + i] * X[c].astype(LD))
        r = X[fam[0]].astype(LD) - m
        t = r / LD(std)
        k = -np.log(LD(std)) - LD(0.5) * np.log(2 * PI_LD)
        lp = lp + (k - LD(0.5) * t * t)
        with np.errstate(divide="ignore", invalid="ignore"):
            amp = np.where(r != 0, t * t * (1 + M / np.abs(r)), (M / LD(std)) ** 2)
        mag = mag + abs(k) + amp
    return lp, ((2 * p_max + 8 + len(families)) * U * mag).astype(np.float64)


# ---------------------------------------------------------------------- affine
def affine_ld(W, c, in_cols, X):
    W, c = np.asarray(W, dtype=np.float64).astype(LD), np.asarray(c, dtype=np.float64).astype(LD)
    Xi = np.asarray(X, dtype=np.float64)[list(in_cols)].astype(LD)
    out = c[:, None] + W @ Xi
    mag = np.abs(c)[:, None] + np.abs(W) @ np.abs(Xi)
    return out, ((len(in_cols) + 1) * U * mag).astype(np.float64)


# ---------------------------------------------------------------------- the sampler
def normals_ld(seed, rows, col):
    """z of stream rows `rows` and column `col` in long double: Philox (sample_cases), then Box-Muller."""
    rows = np.asarray(rows, dtype=np.uint64)
    pair = int(col) & ~1
    u0 = SC.uniform_bits(seed, rows, pair).astype(LD) * LD(2.0 ** -53)
    u1 = SC.uniform_bits(seed, rows, pair + 1).astype(LD) * LD(2.0 ** -53)
    rho = np.sqrt(LD(-2) * np.log(LD(1) - u0))
    sn, cs = sincospi_ld(LD(2) * u1)
    return rho * (sn if int(col) & 1 else cs)


def sincospi_ld(t):
    """(sin(pi t), cos(pi t)) for long-double t in [0, 2] to long-double RELATIVE accuracy: t = q / 2 + r with
    |r| <= 1 / 4 exactly, so the rounding of pi only scales the small angle pi r and a result next to a zero
    of the function keeps all its digits (cos(2 pi u1) evaluated directly loses them there)."""
    t = np.asarray(t, dtype=LD)
    q = np.rint(2 * t)
    r = t - q / 2
    s, c = np.sin(PI_LD * r), np.cos(PI_LD * r)
    q = q.astype(np.int64) % 4
    return (np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s]))


def sample_ld(families, betas, stds, n, seed, first_row=0, n_cols=None, u_z=U_Z_DEVICE, normals=None):
    """(X LD [n_cols, n], bound fp64 [n_cols, n]) of the forward sampler; the normal index is the column.
    normals: normals_ld, or a negative control's stand-in for it."""
    normals = normals_ld if normals is None else normals
    n_cols = 1 + max(c for f in families for c in f) if n_cols is None else n_cols
    X = np.zeros((n_cols, n), dtype=LD)
    B = np.zeros((n_cols, n), dtype=LD)
    rows = np.uint64(first_row) + np.arange(n, dtype=np.uint64)
    for fam, beta, std in zip(families, betas, stds):
        beta = np.asarray(beta, dtype=np.float64).astype(LD)
        p = len(fam) - 1
        z = normals(seed, rows, fam[0])
        x = np.full(n, beta[0], dtype=LD)
        mag = np.full(n, abs(beta[0]), dtype=LD)
        err = np.zeros(n, dtype=LD)
        for i, c in enumerate(fam[1:]):
            x = x + beta[1 + i] * X[c]
            mag = mag + np.abs(beta[1 + i] * X[c])
            err = err + np.abs(beta[1 + i]) * B[c]
        sz = LD(std) * z
        X[fam[0]] = x + sz
        B[fam[0]] = err + (p + 2) * U * (mag + np.abs(sz)) + u_z * U * np.abs(sz)
    return X, B.astype(np.float64)


def model_families(model, columns):
    """(order, families, betas, stds) of a model over the column names `columns`, topological order."""
    import networkx as nx

    col = {v: i for i, v in enumerate(columns)}
    order = list(nx.topological_sort(model))
    cpds = [model.get_cpds(v) for v in order]
    return (order, [[col[c.variable]] + [col[u] for u in c.evidence] for c in cpds], [np.asarray(c.beta, dtype=np.float64) for c in cpds],
            [float(c.std) for c in cpds])


# ---------------------------------------------------------------------- wide and deep synthetic plans
# The shapes of tests/test_lg_wide_gpu.py and of the negative controls in tests/test_lg_cpu.py (module docstring,
# "Wide plans").  Everything below is seeded: the CPU controls see the data the device sees.
GRAM_WIDE_D = (128, 191, 200)        # d + 1 = 129: the third super-tile is the ones column alone; 12 full tiles; 13 tiles, 10 groups
GRAM_WIDE_ROWS = (1, 15, 16, 17, 33)  # below, at and past one step; two steps and one row
AFFINE_N_IN = (0, 1, 255, 256, 257, 600)  # PGM_LG_AFFINE_CHUNK = 256: no input, one launch, two, three
AFFINE_N_OUT = (1, 5)
AFFINE_ROWS = (1, 255, 256, 257)
SLICE_MIN, STEP = 1024, 16           # PGM_LG_SLICE_MIN, PGM_LG_STEP (tests/test_lg_cpu.py asserts the binding's)


def wide_data(n_cols, ld, seed):
    """Dependent columns with different means and scales: every entry of the Gram matrix is its own number."""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(3, ld))
    mix = rng.normal(size=(n_cols, 3))
    return mix @ base + rng.normal(size=(n_cols, ld)) * rng.uniform(0.5, 2.0, (n_cols, 1)) + rng.normal(size=(n_cols, 1)) * 10


def gram_window(d, row0, n_rows, seed, ld=40, n_cols=None, shuffled=False):
    """(host [n_cols, ld], cols [d], shift [d]) of one Gram case: NaN in every row outside the window and in every
    column the plan does not name (column d // 2 among them).  The shift is the mean of the column over ALL ld rows of
    the data before the blanking, not the window's own: a one-row window at its own mean is the zero matrix, on which
    no structural error shows."""
    n_cols = d + 2 if n_cols is None else n_cols
    assert ld > n_rows + row0 and n_cols > d
    full = wide_data(n_cols, ld, seed)
    if shuffled:
        cols = [int(c) for c in np.random.default_rng(seed + 1).permutation(n_cols)[:d]]
    else:
        cols = [c for c in range(n_cols) if c != d // 2][:d]
    shift = colmean(full, cols)
    host = np.full_like(full, np.nan)
    host[cols, row0:row0 + n_rows] = full[cols, row0:row0 + n_rows]
    return host, cols, shift


def gram_wide_shapes():
    """[(name, d, row0, n_rows, kwargs of gram_window)]: every Gram shape of the wide tests but the two kinds of sliced
    launch, whose row count comes from the handle (slice_rows_of)."""
    out = []
    for d in GRAM_WIDE_D:
        for row0 in (0, 1):
            for n in GRAM_WIDE_ROWS:
                out.append((f"d{d}-row{row0}-n{n}", d, row0, n, {"seed": 1000 * d + 10 * n + row0}))
    out.append(("subset140of150", 140, 0, 33, {"seed": 140, "n_cols": 150, "shuffled": True}))
    return out


def slice_rows_of(kind, max_slices):
    """n_rows of a sliced case: 'auto' is the first size the automatic choice splits, 'raised' the first at which a
    forced slice of one step would need more partials than the handle keeps."""
    return SLICE_MIN + 1 if kind == "auto" else STEP * int(max_slices) + 1


def gram_structural_errors(win, cols, shift, slice_rows):
    """{name: G' long double} for the window `win` [n_cols, n_rows]: the long-double Gram matrix with ONE structural
    error each. The sums are linear in the rows, so a matrix without some rows is G minus the Gram matrix of those rows."""
    n = win.shape[1]
    d = len(cols)
    G, _ = gram_ld(win, cols, shift)
    out = {"last_row_left_out": G - gram_ld(win[:, n - 1:], cols, shift)[0]}
    if d >= 17:  # two columns 16 apart (the same lane of neighbouring tiles) exchanged on the A side only
        j = d - 17
        E = G.copy()
        E[[j, j + 16]] = E[[j + 16, j]]
        out["columns_16_apart_exchanged"] = E
    k = ((n + slice_rows - 1) // slice_rows) // 2  # the middle slice; the only one of an unsliced launch
    out["slice_partial_dropped"] = G - gram_ld(win[:, k * slice_rows:(k + 1) * slice_rows], cols, shift)[0]
    return out


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the entries (a zero bound with a zero error counts as 0)."""
    err = np.abs(np.asarray(got).astype(LD) - want).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def affine_case(n_in, n_out, n_rows, row0, seed=0):
    """(W [n_out, n_in], c [n_out], in_cols [n_in], host X [n_in + 7, row0 + n_rows + 2]): the inputs are a permutation
    drawn from the wider X, whose other columns, and whose rows outside the window, hold NaN."""
    rng = np.random.default_rng([seed, n_in, n_out, n_rows, row0])
    n_cols = n_in + 7
    in_cols = [int(c) for c in rng.permutation(n_cols)[:n_in]]
    X = np.full((n_cols, row0 + n_rows + 2), np.nan)
    X[in_cols, row0:row0 + n_rows] = rng.normal(size=(n_in, n_rows)) + 3 * rng.normal(size=(n_in, 1))
    W = rng.normal(size=(n_out, n_in)) / np.sqrt(max(n_in, 1))
    return W, 5 * rng.normal(size=n_out), in_cols, X


def net_cases():
    """The synthetic plans of the net kernels: {name, families, betas, stds, n_cols, ld, n_big}.  |beta_i| <= 1 on chains
    and sum_i |beta_i| <= 1 on wide families keep every value O(10).  ld is the rows of the device buffer the GPU test
    samples into (row0 3 and n_big rows fit with a sentinel row after them)."""
    if "net" in _CACHE:
        return _CACHE["net"]
    rng = np.random.default_rng(20261021)
    out = []

    def add(name, families, n_cols=None, n_big=257, ld=None):
        betas, stds = [], []
        for fam in families:
            p = len(fam) - 1
            w = rng.uniform(-1, 1, p)
            if p > 1:
                w = w / np.abs(w).sum()
            betas.append(np.concatenate([[3 * rng.normal()], w]))
            stds.append(float(rng.uniform(0.5, 2.0)))
        out.append({"name": name, "families": [list(f) for f in families], "betas": betas, "stds": stds,
                    "n_cols": 1 + max(c for f in families for c in f) if n_cols is None else n_cols,
                    "n_big": n_big, "ld": n_big + 6 if ld is None else ld})

    add("chain_300", [[0]] + [[i, i - 1] for i in range(1, 300)])
    add("star_300", [[c] for c in range(300)] + [[300] + list(range(300))])
    add("max_parents", [[c] for c in range(4096)] + [[4096] + list(range(4096))], n_big=64, ld=70)
    add("odd_first", [[1], [0, 1], [3, 0, 1], [2, 3]])
    add("interleaved", [[0], [2, 0], [1, 2, 0], [3, 1]])
    add("gaps", [[0], [1, 0], [2, 1], [3, 2, 0], [6, 3], [7, 6, 1], [8, 7], [9, 8, 6, 0]], n_cols=12)
    add("dense_40", [[i] + list(range(i)) for i in range(40)])
    _CACHE["net"] = out
    return out


def net_first_rows(n):
    return (0, (1 << 33) + 5, (1 << 63) - 1 - n)


def net_sample(case, n, first_row, seed=77, wrong_trig=False):
    """sample_ld of a net case, cached; wrong_trig: the structural error of the negative control, an odd column
    taking the cosine of its pair where the sine belongs."""
    key = ("net_sample", case["name"], n, first_row, seed, wrong_trig)
    if key not in _CACHE and n < case["n_big"] and first_row + case["n_big"] < 1 << 63:
        X, B = net_sample(case, case["n_big"], first_row, seed, wrong_trig)  # a row depends on its stream row alone
        _CACHE[key] = (X[:, :n], B[:, :n])
    if key not in _CACHE:
        normals =(lambda s, rows, col: normals_ld(s, rows, int(col) & ~1)) if wrong_trig else normals_ld
        _CACHE[key] = sample_ld(case["families"], case["betas"], case["stds"], n, seed, first_row, n_cols=case["n_cols"],
                                normals=normals)
    return _CACHE[key]


def net_logpdf(case, drop_parent=False):
    """(X fp64 [n_cols, n_big] the rounding of the restated sample with NaN in the columns no family names, lp, bound)
    of a net case, cached; drop_parent: the structural error, the last family with a parent scored without its last one."""
    key = ("net_logpdf", case["name"], drop_parent)
    if key not in _CACHE:
        X = net_sample(case, case["n_big"], 0)[0].astype(np.float64)
        named = sorted({c for f in case["families"] for c in f})
        blank = [c for c in range(case["n_cols"]) if c not in named]
        X[blank] = np.nan
        fams, betas = [list(f) for f in case["families"]], [np.array(b) for b in case["betas"]]
        if drop_parent:
            f = max(i for i, fam in enumerate(fams) if len(fam) > 1)
            fams[f], betas[f] = fams[f][:-1], betas[f][:-1]
        _CACHE[key] = (X,) + logpdf_ld(np.nan_to_num(X), fams, betas, case["stds"])
    return _CACHE[key]


WIDE_MODEL = {"n_nodes": 300, "edge_prob": 0.03, "seed": 300, "graph_seed": 20261021}


def wide_model():
    """LinearGaussianBayesianNetwork.get_random(300 nodes, edge_prob 0.03).  The call draws its graph from numpy's UNSEEDED
    generator (as the reference's does), so for this one call the unseeded default_rng is pinned to graph_seed: the
    model, and with it every condition number the checks use, is the same in every run."""
    if "wide_model" not in _CACHE:
        from pgmpy_amd.models import LinearGaussianBayesianNetwork

        real = np.random.default_rng
        np.random.default_rng = lambda seed=None: real(WIDE_MODEL["graph_seed"] if seed is None else seed)
        try:
            _CACHE["wide_model"] = LinearGaussianBayesianNetwork.get_random(
                n_nodes=WIDE_MODEL["n_nodes"], edge_prob=WIDE_MODEL["edge_prob"], seed=WIDE_MODEL["seed"])
        finally:
            np.random.default_rng = real
    return _CACHE["wide_model"]
