"""Binding of the pgm_fit_* entry points (include/pgmhip.h, pgmpy_amd/csrc/pgmfit.hip): the state counts
of a set of families in one launch and every CPD's values in one more.

A family is ``(columns, cardinalities)``: the code column and cardinality of the node, then of each
parent in the CPD's order.  The count tables, the pseudo-counts and the values share one flat layout:
family f occupies ``[offsets[f], offsets[f] + sizes[f])``, shaped ``[node_card, prod(parent_card)]`` in
C order.
"""
import ctypes

from .. import _native as N
from .._plan import Plan, codes_window, family_array, flat_tensor


class FitPlan(Plan):
    _destroy = "pgm_fit_plan_destroy"

    def __init__(self, families):
        L = N.load_library()  # building and inspecting a plan needs no device
        families, fams = family_array(families)
        self._h = ctypes.c_void_p()
        N.check(L.pgm_fit_plan_create(fams, len(families), ctypes.byref(self._h)), "fit_plan_create")
        n = len(families)
        self.families = families
        self.info = N.FitInfo()
        off, size = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
        strides, groups = (ctypes.c_int32 * (n * N.PGM_MAX_DIMS))(), (ctypes.c_int32 * n)()
        N.check(L.pgm_fit_plan_info(self._h, ctypes.byref(self.info), off, size, strides, groups), "fit_plan_info")
        self.offsets, self.sizes, self.groups = list(off), list(size), list(groups)
        self.strides = [list(strides[f * N.PGM_MAX_DIMS:f * N.PGM_MAX_DIMS + len(families[f][0])]) for f in range(n)]
        self.total_bins = int(self.info.total_bins)

    def _int64_counts(self, counts, note=""):
        import torch

        flat_tensor("counts", counts, self.total_bins, torch.int64, "int64", f"of {self.total_bins} entries{note}")

    def count(self, codes, n_rows=None, row0=0, weights=None, tables=None):
        """Add the rows [row0, row0 + n_rows) of the device codes [n_cols, ld] (uint8) to `tables` (a
        zeroed flat buffer when None): int64 counts, or fp64 sums of `weights` (a device fp64 tensor of
        ld entries).  Raises IndexError when a code is neither 255 nor a state."""
        import torch

        L = N.lib()
        n_cols, ld, n_rows = codes_window(codes, n_rows, row0)
        dtype = torch.int64 if weights is None else torch.float64
        if weights is not None:
            flat_tensor("weights", weights, ld, entries="with one entry per row of codes")
        if tables is None:
            tables = torch.zeros(self.total_bins, dtype=dtype, device=codes.device)
        else:
            flat_tensor("tables", tables, self.total_bins, dtype, str(dtype))
        N.check(L.pgm_fit_count(self._h, N.ptr(codes), n_cols, ld, int(row0), n_rows, N.ptr(weights), N.ptr(tables),
                                N.stream_handle()), "fit_count")
        return tables

    @staticmethod
    def _latent_array(latent_cols):
        cols = [int(c) for c in latent_cols]
        return (ctypes.c_int32 * max(len(cols), 1))(*cols), len(cols)

    def estep_info(self, latent_cols):
        """pgm_em_info_t of an E-step over this plan with the code columns `latent_cols` latent: the number
        of latent configurations, the family split and the LDS bytes of the launch.  Needs no device."""
        L = N.load_library()
        arr, n = self._latent_array(latent_cols)
        info = N.EmInfo()
        N.check(L.pgm_fit_estep_info(self._h, arr, n, ctypes.byref(info)), "fit_estep_info")
        return info

    def estep(self, latent_cols, values, codes, n_rows=None, row0=0, tables=None, want_loglik=False):
        """The E-step of expectation maximisation (pgm_fit_estep) over the rows [row0, row0 + n_rows) of
        the device codes [n_cols, ld] (uint8): under the CPD `values` (a flat fp64 device tensor) each row
        adds its posterior over the configurations of the latent code columns `latent_cols` (virtual:
        never read) to the fp64 `tables` (a zeroed flat buffer when None) of the families with a latent,
        and 1.0 to the others.  A row with 255 in an observed column of any family is not counted.
        Returns the tables, and with want_loglik the fp64 device tensor [ld] of the rows' log-likelihoods
        beside them.  Raises IndexError when a code is neither 255 nor a state."""
        import torch

        L = N.lib()
        n_cols, ld, n_rows = codes_window(codes, n_rows, row0)
        flat_tensor("values", values, self.total_bins)
        if tables is None:
            tables = torch.zeros(self.total_bins, dtype=torch.float64, device=codes.device)
        else:
            flat_tensor("tables", tables, self.total_bins, label="torch.float64")
        arr, n = self._latent_array(latent_cols)
        loglik = torch.zeros(ld, dtype=torch.float64, device=codes.device) if want_loglik else None
        N.check(L.pgm_fit_estep(self._h, arr, n, N.ptr(values), N.ptr(codes), n_cols, ld, int(row0), n_rows,
                                N.ptr(tables), N.ptr(loglik), N.stream_handle()), "fit_estep")
        return (tables, loglik) if want_loglik else tables

    def finish(self, counts, pseudo=None, bayes=False, out=None):
        """Every CPD's values from the count tables (+ fp64 pseudo-counts of the same layout): each
        column divided by its sum; MLE (bayes=False) fills an all-zero column uniformly, Bayes keeps
        0/0 = NaN.  Returns the flat fp64 device buffer."""
        import torch

        L = N.lib()
        if counts.dtype not in (torch.int64, torch.float64) or counts.numel() < self.total_bins:
            raise ValueError(f"counts must be an int64 or fp64 device tensor of {self.total_bins} entries")
        mode = (N.FIT_BAYES if bayes else N.FIT_MLE) | (N.FIT_WEIGHTED if counts.dtype == torch.float64 else 0)
        if pseudo is not None and (pseudo.dtype != torch.float64 or pseudo.numel() < self.total_bins):
            raise ValueError(f"pseudo-counts must be an fp64 device tensor of {self.total_bins} entries")
        if out is None:
            out = torch.empty(self.total_bins, dtype=torch.float64, device=counts.device)
        N.check(L.pgm_fit_finish(self._h, N.ptr(counts), N.ptr(pseudo), mode, N.ptr(out), N.stream_handle()),
                "fit_finish")
        return out

    def logprob_info(self, codes_ptr, ld, row0=0, n_rows=None):
        """pgm_logp_info_t of a logprob call over the rows [row0, row0 + n_rows) of codes at address
        `codes_ptr` with `ld` rows per column: block, rows per block, whether the launch takes the
        four-rows-per-lane path, and the number of block partials.  Needs no device."""
        L = N.load_library()
        info = N.LogpInfo()
        n_rows = int(ld) - int(row0) if n_rows is None else int(n_rows)
        N.check(L.pgm_fit_logprob_info(self._h, ctypes.c_void_p(codes_ptr), int(ld), int(row0), n_rows,
                                       ctypes.byref(info)), "fit_logprob_info")
        return info

    def log_values(self, values, out=None):
        """log(values) over the flat layout in one launch (pgm_fit_log_values): 0 gives -inf; `out` may be
        `values` itself.  Raises ValueError when a value is negative or NaN."""
        import torch

        L = N.lib()
        flat_tensor("values", values, self.total_bins)
        if out is None:
            out = torch.empty(self.total_bins, dtype=torch.float64, device=values.device)
        else:
            flat_tensor("out", out, self.total_bins)
        N.check(L.pgm_fit_log_values(self._h, N.ptr(values), N.ptr(out), N.stream_handle()), "fit_log_values")
        return out

    def logprob(self, logv, codes, n_rows=None, row0=0, logp=None, total=False):
        """The log-probability of the rows [row0, row0 + n_rows) of the device codes [n_cols, ld] (uint8)
        under the log tables `logv` (log_values' flat fp64 device tensor), one family per node
        (pgm_fit_logprob).  Returns (logp, total, n_skipped): `logp` the fp64 device tensor [ld] indexed by
        buffer row (a new one filled with NaN when None; rows outside the window are not touched), `total`
        a one-element fp64 device tensor with the sum over the rows that are not skipped (None unless
        asked for), n_skipped the number of rows that hold 255 in a column a family reads (their logp is
        NaN), downloaded with the status.  Raises IndexError when a code is neither 255 nor a state."""
        import torch

        L = N.lib()
        n_cols, ld, n_rows = codes_window(codes, n_rows, row0)
        flat_tensor("logv", logv, self.total_bins)
        if logp is None:
            logp = torch.full((ld,), float("nan"), dtype=torch.float64, device=codes.device)
        else:
            flat_tensor("logp", logp, ld, entries="with one entry per row of codes")
        tot = torch.empty(1, dtype=torch.float64, device=codes.device) if total else None
        skipped = torch.empty(1, dtype=torch.int64, device=codes.device)
        N.check(L.pgm_fit_logprob(self._h, N.ptr(logv), N.ptr(codes), n_cols, ld, int(row0), n_rows, N.ptr(logp),
                                  N.ptr(tot), N.ptr(skipped), N.stream_handle()), "fit_logprob")
        return logp, tot, int(skipped.item())

    def score(self, counts, mode, alpha=None, beta=None, want_observed=False):
        """The data-dependent sum of a structure score per family (pgm_fit_score) from the int64 count
        tables: `mode` is N.SCORE_BD (alpha, beta: fp64 device tensors, one entry per family) or
        N.SCORE_LL, | N.SCORE_SKIP_EMPTY.  Returns the fp64 device scores [n_families], and with
        want_observed the int64 device counts of observed columns beside them."""
        import torch

        L = N.lib()
        n = len(self.families)
        self._int64_counts(counts, " (weighted tables have no structure score)")
        for name, t in (("alpha", alpha), ("beta", beta)):
            if t is not None:
                flat_tensor(name, t, n, entries="with one entry per family")
        scores = torch.empty(n, dtype=torch.float64, device=counts.device)
        observed = torch.empty(n, dtype=torch.int64, device=counts.device) if want_observed else None
        N.check(L.pgm_fit_score(self._h, N.ptr(counts), int(mode), N.ptr(alpha), N.ptr(beta), N.ptr(scores),
                                N.ptr(observed), N.stream_handle()), "fit_score")
        return (scores, observed) if want_observed else scores

    def citest(self, counts, lambda_, yates=True):
        """The power-divergence test of X _|_ Y | Z for every family read as (X, Y, Z...) from its int64
        count table (pgm_fit_citest): the device tensors (stat fp64, dof int64, pvalue fp64), one entry
        per family.  `yates`: chi2_contingency's continuity correction in strata with one degree of freedom."""
        import torch

        L = N.lib()
        n = len(self.families)
        self._int64_counts(counts, " (weighted tables have no CI test)")
        stat = torch.empty(n, dtype=torch.float64, device=counts.device)
        dof = torch.empty(n, dtype=torch.int64, device=counts.device)
        pvalue = torch.empty(n, dtype=torch.float64, device=counts.device)
        N.check(L.pgm_fit_citest(self._h, N.ptr(counts), float(lambda_), N.CI_YATES if yates else 0, N.ptr(stat),
                                 N.ptr(dof), N.ptr(pvalue), N.stream_handle()), "fit_citest")
        return stat, dof, pvalue

    def states_observed(self, counts):
        """Per family the number of the node's states that hold a count in any column
        (pgm_fit_states_observed): an int64 device tensor [n_families]."""
        import torch

        L = N.lib()
        self._int64_counts(counts)
        out = torch.empty(len(self.families), dtype=torch.int64, device=counts.device)
        N.check(L.pgm_fit_states_observed(self._h, N.ptr(counts), N.ptr(out), N.stream_handle()), "fit_states_observed")
        return out
