"""Binding of the pgm_lg_* entry points (include/pgmhip.h "linear-Gaussian networks", pgmpy_amd/csrc/pgmlg.hip)
and the host arithmetic that goes with them.

The data is a resident fp64 value matrix: a contiguous ``torch.float64`` device tensor ``X[n_cols, ld]``
(column-major like the codes: ``X[col, row]``); a call works on the rows ``[row0, row0 + n_rows)``.

``GramPlan`` (columns) gives the column sums and the shifted Gram matrix of pgm_lg_colsum / pgm_lg_gram;
``SchurJobs`` runs batches of partial correlations and Gaussian family scores on that matrix where it lies
(pgm_lgs_pcorr / pgm_lgs_score, pgmpy_amd/csrc/pgmlgs.hip);
``moments`` turns the downloaded matrix into (n, mean, S) in np.longdouble and ``ols`` into one node's
regression.  ``NetPlan`` (families in topological order) samples and scores; ``affine`` is predict's row map.
The host functions take numpy arrays only: the restatement of the tests calls them with its own Gram matrix.
"""
import ctypes

import numpy as np

from .. import _native as N
from .._plan import MASK64, Plan, flat_tensor

LD = np.longdouble
# An eigenvalue of the correlation-scaled parent Gram matrix below RCOND times the largest counts as zero:
# parents that collinear get the minimum-norm coefficients, as scikit-learn's lstsq gives them.
RCOND = 1e-11


def values_window(X, n, row0):
    """(n_cols, ld, n) of a launch over the rows [row0, row0 + n) of `X`; n None: up to the last row."""
    import torch

    if not isinstance(X, torch.Tensor) or X.dtype != torch.float64 or X.dim() != 2 or not X.is_contiguous():
        raise ValueError("X must be a contiguous [n_cols, ld] float64 device tensor")
    n_cols, ld = int(X.shape[0]), int(X.shape[1])
    return n_cols, ld, (ld - row0 if n is None else int(n))


def _i32(vals):
    return (ctypes.c_int32 * max(len(vals), 1))(*[int(v) for v in vals])


class GramPlan(Plan):
    _destroy = "pgm_lg_gram_plan_destroy"

    def __init__(self, columns):
        L = N.load_library()  # building and inspecting a plan needs no device
        self.columns = [int(c) for c in columns]
        self.d = len(self.columns)
        self._h = ctypes.c_void_p()
        N.check(L.pgm_lg_gram_plan_create(_i32(self.columns), self.d, ctypes.byref(self._h)), "lg_gram_plan_create")
        self.info = N.LgGramInfo()
        N.check(L.pgm_lg_gram_plan_info(self._h, ctypes.byref(self.info), None), "lg_gram_plan_info")

    def groups(self):
        """[(I, J)] of the super-tile pairs a Gram launch runs (grid.x)."""
        g = (ctypes.c_int32 * max(2 * int(self.info.n_groups), 1))()
        N.check(N.load_library().pgm_lg_gram_plan_info(self._h, ctypes.byref(self.info), g), "lg_gram_plan_info")
        return [(g[2 * i], g[2 * i + 1]) for i in range(int(self.info.n_groups))]

    def set_slice(self, rows):
        """Force the rows per slice of the Gram launches (0: the automatic choice)."""
        N.check(N.load_library().pgm_lg_gram_plan_set_slice(self._h, int(rows)), "lg_gram_plan_set_slice")
        N.check(N.load_library().pgm_lg_gram_plan_info(self._h, ctypes.byref(self.info), None), "lg_gram_plan_info")

    def gram_info(self, n_rows, x_ptr=0, ld=0, row0=0):
        """(rows per slice, slices, whether the 16-byte loads apply) of a Gram over such a window."""
        s, k, v = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        N.check(N.load_library().pgm_lg_gram_info(self._h, ctypes.c_void_p(x_ptr), int(ld), int(row0), int(n_rows),
                                                  ctypes.byref(s), ctypes.byref(k), ctypes.byref(v)), "lg_gram_info")
        return int(s.value), int(k.value), bool(v.value)

    def colsum(self, X, n_rows=None, row0=0):
        """(sums fp64 [d], counts int64 [d]) device tensors of the window's columns (pgm_lg_colsum)."""
        import torch

        L = N.lib()
        n_cols, ld, n_rows = values_window(X, n_rows, row0)
        sums = torch.zeros(max(self.d, 1), dtype=torch.float64, device=X.device)
        counts = torch.zeros(max(self.d, 1), dtype=torch.int64, device=X.device)
        N.check(L.pgm_lg_colsum(self._h, N.ptr(X), n_cols, ld, int(row0), n_rows, N.ptr(sums), N.ptr(counts),
                                N.stream_handle()), "lg_colsum")
        return sums[:self.d], counts[:self.d]

    def gram(self, X, shift, n_rows=None, row0=0, out=None):
        """The (d + 1) x (d + 1) fp64 device matrix of the shifted columns and the ones column (pgm_lg_gram)."""
        import torch

        L = N.lib()
        n_cols, ld, n_rows = values_window(X, n_rows, row0)
        flat_tensor("shift", shift, self.d)
        d1 = self.d + 1
        if out is None:
            out = torch.zeros((d1, d1), dtype=torch.float64, device=X.device)
        else:
            flat_tensor("out", out, d1 * d1)
        if self.d == 0:  # the kernel takes the pointer
            shift = torch.zeros(1, dtype=torch.float64, device=X.device)
        N.check(L.pgm_lg_gram(self._h, N.ptr(X), n_cols, ld, int(row0), n_rows, N.ptr(shift), N.ptr(out), N.stream_handle()),
                "lg_gram")
        return out

    def moments_device(self, X, n_rows=None, row0=0):
        """One colsum, one Gram, nothing downloaded: (G [d + 1, d + 1], shift [d]) as fp64 device tensors."""
        import torch

        n_cols, ld, n_rows = values_window(X, n_rows, row0)
        if n_rows <= 0:
            raise ValueError("no rows")
        sums, counts = self.colsum(X, n_rows, row0)
        shift = (sums / counts.to(torch.float64)).contiguous()
        return self.gram(X, shift, n_rows, row0), shift

    def moments_on_device(self, X, n_rows=None, row0=0):
        """One colsum, one Gram, ONE download: (G [d + 1, d + 1], shift [d]) as fp64 ndarrays."""
        import torch

        G, shift = self.moments_device(X, n_rows, row0)
        host = torch.cat([G.reshape(-1), shift]).cpu().numpy()
        d1 = self.d + 1
        return host[:d1 * d1].reshape(d1, d1), host[d1 * d1:]


class SchurJobs(Plan):
    """A job batch of pgm_lgs_pcorr / pgm_lgs_score over a Gram plan's matrix: jobs are (K, targets) pairs of
    positions 0 .. d in the plan's columns, d being the ones column.  Built and validated on the host."""
    _destroy = "pgm_lgs_jobs_destroy"
    KINDS = {"ll": N.LGS_LL, "bic": N.LGS_BIC, "aic": N.LGS_AIC}

    def __init__(self, gram_plan, jobs):
        L = N.load_library()
        self.d = int(gram_plan.d if hasattr(gram_plan, "d") else gram_plan)
        self.jobs = [([int(c) for c in K], [int(c) for c in T]) for K, T in jobs]
        self.n = len(self.jobs)
        off, flat = [0], []
        for K, T in self.jobs:
            flat.extend(K)
            flat.extend(T)
            off.append(len(flat))
        self._h = ctypes.c_void_p()
        N.check(L.pgm_lgs_jobs_create(_i32(off), _i32(flat), _i32([len(T) for _, T in self.jobs]), self.n, self.d,
                                      ctypes.byref(self._h)), "lgs_jobs_create")
        self.info = N.LgsInfo()
        N.check(L.pgm_lgs_jobs_info(self._h, ctypes.byref(self.info), None, None), "lgs_jobs_info")

    def buckets(self):
        """([(|K|, targets, first, count)], order): the launches of a call and the jobs bucket by bucket."""
        b = (ctypes.c_int32 * max(4 * int(self.info.n_buckets), 1))()
        o = (ctypes.c_int32 * max(self.n, 1))()
        N.check(N.load_library().pgm_lgs_jobs_info(self._h, ctypes.byref(self.info), b, o), "lgs_jobs_info")
        return [tuple(b[4 * i:4 * i + 4]) for i in range(int(self.info.n_buckets))], list(o)[:self.n]

    def _outputs(self, G):
        import torch

        flat_tensor("G", G, (self.d + 1) * (self.d + 1))
        out = torch.empty((2, max(self.n, 1)), dtype=torch.float64, device=G.device)
        rank = torch.empty(max(self.n, 1), dtype=torch.int32, device=G.device)
        return out, rank

    def _shift(self, G, shift):
        import torch

        if self.d == 0:  # the kernel takes the pointer
            return torch.zeros(1, dtype=torch.float64, device=G.device)
        flat_tensor("shift", shift, self.d)
        return shift

    def pcorr(self, G, shift, intercept=False):
        """(coef, pvalue fp64 [n], rank int32 [n]) device tensors of the batch's partial correlations."""
        L = N.lib()
        out, rank = self._outputs(G)
        shift = self._shift(G, shift)
        N.check(L.pgm_lgs_pcorr(self._h, N.ptr(G), N.ptr(shift), self.d, 1 if intercept else 0, N.ptr(out[0]), N.ptr(out[1]),
                                N.ptr(rank), N.stream_handle()), "lgs_pcorr")
        return out[0, :self.n], out[1, :self.n], rank[:self.n]

    def score(self, G, shift, kind):
        """(score, rss fp64 [n], rank int32 [n]) device tensors of the batch's families; kind 'll', 'bic', 'aic'."""
        if kind not in self.KINDS:
            raise ValueError(f"kind must be one of {sorted(self.KINDS)}, got {kind!r}")
        L = N.lib()
        out, rank = self._outputs(G)
        shift = self._shift(G, shift)
        N.check(L.pgm_lgs_score(self._h, N.ptr(G), N.ptr(shift), self.d, self.KINDS[kind], N.ptr(out[0]), N.ptr(out[1]),
                                N.ptr(rank), N.stream_handle()), "lgs_score")
        return out[0, :self.n], out[1, :self.n], rank[:self.n]


class NetPlan(Plan):
    _destroy = "pgm_lg_net_destroy"

    def __init__(self, families):
        """families: [node column, parent columns ...] per node, in a topological order."""
        L = N.load_library()
        self.families = [[int(c) for c in fam] for fam in families]
        off = [0]
        for fam in self.families:
            off.append(off[-1] + len(fam))
        flat = [c for fam in self.families for c in fam]
        self._h = ctypes.c_void_p()
        N.check(L.pgm_lg_net_create(_i32(off), _i32(flat), len(self.families), ctypes.byref(self._h)), "lg_net_create")
        self.info = N.LgNetInfo()
        co = (ctypes.c_int64 * max(len(self.families), 1))()
        N.check(L.pgm_lg_net_info(self._h, ctypes.byref(self.info), co), "lg_net_info")
        self.coef_off = list(co)[:len(self.families)]
        self.n_coef = int(self.info.n_coef)

    def coef(self, betas, stds):
        """The flat fp64 coefficient array of a call: per family beta_0, beta_1 .. beta_p, sigma."""
        out = np.zeros(self.n_coef, dtype=np.float64)
        for f, (fam, beta, std) in enumerate(zip(self.families, betas, stds)):
            beta = np.asarray(beta, dtype=np.float64).reshape(-1)
            if beta.size != len(fam):
                raise ValueError(f"family {f}: {beta.size} coefficients for {len(fam) - 1} parents")
            o = self.coef_off[f]
            out[o:o + len(fam)] = beta
            out[o + len(fam)] = float(std)
        return out

    def sample(self, coef, X, n_rows=None, row0=0, first_row=0, seed=0):
        L = N.lib()
        n_cols, ld, n_rows = values_window(X, n_rows, row0)
        flat_tensor("coef", coef, self.n_coef)
        N.check(L.pgm_lg_sample(self._h, N.ptr(coef), N.ptr(X), n_cols, ld, int(row0), n_rows, int(first_row),
                                int(seed) & MASK64, N.stream_handle()), "lg_sample")
        return X

    def logpdf(self, coef, konst, X, n_rows=None, row0=0, total=True):
        """(logp fp64 [n_rows], total fp64 [1] or None) device tensors; windows longer than one call's limit
        are scored piece by piece and their totals added in order."""
        import torch

        L = N.lib()
        n_cols, ld, n_rows = values_window(X, n_rows, row0)
        flat_tensor("coef", coef, self.n_coef)
        flat_tensor("konst", konst, len(self.families))
        logp = torch.empty(max(n_rows, 1), dtype=torch.float64, device=X.device)[:n_rows]
        step = N.LG_BLOCK * N.LG_MAX_BLOCKS
        tot = torch.zeros(1, dtype=torch.float64, device=X.device) if total else None
        piece = torch.zeros(1, dtype=torch.float64, device=X.device) if total else None
        for r in range(0, n_rows, step):
            n = min(step, n_rows - r)
            N.check(L.pgm_lg_logpdf(self._h, N.ptr(coef), N.ptr(konst), N.ptr(X), n_cols, ld, int(row0) + r, n,
                                    ctypes.c_void_p(logp.data_ptr() + 8 * r), N.ptr(piece), N.stream_handle()), "lg_logpdf")
            if total:
                tot = tot + piece if r else piece.clone()
        return logp, tot


def affine(W, c, in_cols, X, n_rows=None, row0=0):
    """out[j, r] = c[j] + sum_i W[j, i] X[in_cols[i], row0 + r]: an fp64 device tensor [n_out, n_rows]."""
    import torch

    L = N.lib()
    n_cols, ld, n_rows = values_window(X, n_rows, row0)
    W = np.ascontiguousarray(W, dtype=np.float64)
    c = np.ascontiguousarray(c, dtype=np.float64).reshape(-1)
    n_out, n_in = int(W.shape[0]), int(W.shape[1])
    if len(in_cols) != n_in or c.size != n_out:
        raise ValueError(f"W is {n_out} x {n_in}, {len(in_cols)} input columns, {c.size} constants")
    dW = torch.from_numpy(W.reshape(-1) if W.size else np.zeros(1)).to(X.device)
    dc = torch.from_numpy(c).to(X.device)
    out = torch.empty((n_out, max(n_rows, 1)), dtype=torch.float64, device=X.device)
    N.check(L.pgm_lg_affine(N.ptr(dW), N.ptr(dc), _i32(in_cols), n_in, n_out, N.ptr(X), n_cols, ld, int(row0), n_rows,
                            N.ptr(out), int(out.shape[1]), N.stream_handle()), "lg_affine")
    return out[:, :n_rows]


# ---------------------------------------------------------------------- host arithmetic
def moments(G, shift):
    """(n, mean [d], S [d, d]) in np.longdouble from the shifted Gram matrix G [d + 1, d + 1] (ones column last)
    and its shift: mean = c + G_x1 / n, S_xy = G_xy - G_x1 G_y1 / n.  The correction is exact algebra for
    any c and loses nothing when c is within rounding of the mean."""
    G = np.asarray(G, dtype=LD)
    d = G.shape[0] - 1
    n = G[d, d]
    g1 = G[:d, d]
    return n, np.asarray(shift, dtype=LD) + g1 / n, G[:d, :d] - np.outer(g1, g1) / n


def min_norm_solve(A, s):
    """The minimum-norm least-squares solution b of A b = s for a symmetric positive semi-definite A (fp64
    eigendecomposition of the correlation-scaled matrix, then one refinement step in np.longdouble when A
    has full rank)."""
    A64, s64 = np.asarray(A, dtype=np.float64), np.asarray(s, dtype=np.float64)
    p = len(s64)
    dg = np.sqrt(np.clip(np.diag(A64), 0.0, None))
    live = dg > 0  # a constant parent has a zero column: coefficient 0
    b = np.zeros(p, dtype=LD)
    if not live.any():
        return b
    idx = np.nonzero(live)[0]
    D = dg[idx]
    C = A64[np.ix_(idx, idx)] / np.outer(D, D)
    w, V = np.linalg.eigh(C)
    keep = w > RCOND * w.max()
    Vk = V[:, keep]
    y = Vk @ ((Vk.T @ (s64[idx] / D)) / w[keep])
    if keep.all():
        AL, sL = np.asarray(A, dtype=LD)[np.ix_(idx, idx)], np.asarray(s, dtype=LD)[idx]
        x = (y / D).astype(LD)
        r = (sL - AL @ x).astype(np.float64)
        x = x + ((Vk @ ((Vk.T @ (r / D)) / w)) / D).astype(LD)
        b[idx] = x
        return b
    x = y / D
    Nn = V[:, ~keep] / D[:, None]  # null space of A in the unscaled coordinates
    x = x - Nn @ np.linalg.lstsq(Nn, x, rcond=None)[0]
    b[idx] = x.astype(LD)
    return b


def ols(n, mean, S, v, parents, std_estimator="unbiased"):
    """(beta fp64 [1 + p], std float) of node index v on parent indices `parents` from the moments:
    b = lstsq(S_pp, s_pv), intercept mean_v - b . mean_p, std = sqrt(rss / (n - ddof)) with rss the residual
    sum of squares S_vv - 2 b . s_pv + b' S_pp b and ddof 0 ('mle') or 1 + p ('unbiased'); NaN when
    n <= ddof, as pandas."""
    p = len(parents)
    ddof = 0 if std_estimator == "mle" else 1 + p
    if p == 0:
        b = np.zeros(0, dtype=LD)
        rss = S[v, v]
    else:
        P = list(parents)
        Spp, spv = S[np.ix_(P, P)], S[P, v]
        b = min_norm_solve(Spp, spv)
        rss = S[v, v] - 2 * (b @ spv) + b @ (Spp @ b)
    b0 = mean[v] - (b @ mean[list(parents)] if p else LD(0))
    dof = n - ddof
    std = float(np.sqrt(max(rss, LD(0)) / dof)) if dof > 0 else float("nan")
    return np.concatenate([[b0], b]).astype(np.float64), std


def condition(mu, cov, a_idx, b_idx):
    """(W, cov_cond) of x_a | x_b for the joint N(mu, cov): W = cov_ab cov_bb^-1, cov_cond = cov_aa - W cov_ba."""
    cov_aa, cov_ab = cov[np.ix_(a_idx, a_idx)], cov[np.ix_(a_idx, b_idx)]
    if not len(b_idx):
        return np.zeros((len(a_idx), 0)), cov_aa
    W = np.linalg.solve(cov[np.ix_(b_idx, b_idx)], cov_ab.T).T
    return W, cov_aa - W @ cov_ab.T


def dense_chain(m, C):
    """[(beta [1 + j], std)] for j = 0 .. k - 1: the regressions x_j | x_0 .. x_{j-1} of N(m, C), from its
    Cholesky factor L: x = m + L z, so x_j - m_j = L[j, :j] L[:j, :j]^-1 (x_<j - m_<j) + L[j, j] z_j."""
    m, C = np.asarray(m, dtype=np.float64), np.asarray(C, dtype=np.float64)
    try:
        L = np.linalg.cholesky((C + C.T) / 2)
    except np.linalg.LinAlgError:
        raise ValueError("the conditional covariance is not positive definite") from None
    out = []
    for j in range(len(m)):
        w = np.linalg.solve(L[:j, :j].T, L[j, :j]) if j else np.zeros(0)
        out.append((np.concatenate([[m[j] - w @ m[:j]], w]), float(L[j, j])))
    return out
