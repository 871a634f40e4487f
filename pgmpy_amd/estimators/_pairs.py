"""Binding of the pgm_pair_* entry points (include/pgmhip.h "pairwise counts", pgmpy_amd/csrc/pgmpair.hip):
the contingency table of every pair of columns in one int8 MFMA launch, optionally per state of a stratum
column, and the pair statistics (mutual information, entropies, expected mutual information) in one
launch each.

The states of all variables are laid end to end (``offsets``), ``S`` of them, ``Sp`` = S rounded up to 16.
The counts are an int64 device tensor ``[n_strata, Sp, Sp]``; for u < v the block
``[c, offsets[u]:offsets[u] + cards[u], offsets[v]:offsets[v] + cards[v]]`` is the table of (u, v) in
stratum c.  Nothing else of the tensor is specified.  A pair's statistics sit at ``[c, pair_index(u, v)]``,
pairs in the order (0, 1), (0, 2), ..., (1, 2), ...

``pair_weights`` turns the downloaded statistics into the edge weights of the tree learners on the host
(numpy): it is shared by the device path and by the numpy restatement of the tests.
"""
import ctypes

import numpy as np

from .. import _native as N
from .._plan import Plan, codes_window, flat_tensor

KINDS = ("mutual_info", "adjusted_mutual_info", "normalized_mutual_info")
COUNT_BUDGET = 1 << 31  # bytes of one count tensor [n_strata, Sp, Sp] a PairPlan allocates


class PairPlan(Plan):
    _destroy = "pgm_pair_plan_destroy"

    def __init__(self, columns, cards, budget=COUNT_BUDGET):
        L = N.load_library()  # building and inspecting a plan needs no device
        self.columns, self.cards = [int(c) for c in columns], [int(k) for k in cards]
        if len(self.columns) != len(self.cards):
            raise ValueError(f"{len(self.columns)} columns, {len(self.cards)} cardinalities")
        n = len(self.columns)
        cols, crd = (ctypes.c_int32 * max(n, 1))(*self.columns), (ctypes.c_int32 * max(n, 1))(*self.cards)
        self._h = ctypes.c_void_p()
        N.check(L.pgm_pair_plan_create(cols, crd, n, ctypes.byref(self._h)), "pair_plan_create")
        self.info = N.PairInfo()
        off = (ctypes.c_int64 * (n + 1))()
        N.check(L.pgm_pair_plan_info(self._h, ctypes.byref(self.info), off, None, None), "pair_plan_info")
        self.offsets = list(off)
        self.n_vars, self.S, self.Sp, self.n_pairs = n, int(self.info.S), int(self.info.Sp), int(self.info.n_pairs)
        self.budget = int(budget)

    # ------------------------------------------------------------------ host-only queries
    def tile_pairs(self):
        """[(ti, tj)] of the 16 x 16 tile pairs that touch a block of two variables."""
        t = (ctypes.c_int32 * max(2 * int(self.info.n_tile_pairs), 1))()
        N.check(N.load_library().pgm_pair_plan_info(self._h, None, None, t, None), "pair_plan_info")
        return [(t[2 * i], t[2 * i + 1]) for i in range(int(self.info.n_tile_pairs))]

    def groups(self):
        """[(I, J, check)] of the 64 x 64 super-tile pairs a count launch runs (grid.x)."""
        g = (ctypes.c_int32 * max(3 * int(self.info.n_groups), 1))()
        N.check(N.load_library().pgm_pair_plan_info(self._h, None, None, None, g), "pair_plan_info")
        return [(g[3 * i], g[3 * i + 1], g[3 * i + 2]) for i in range(int(self.info.n_groups))]

    def set_slice(self, rows):
        """Force the rows per slice of the count launches (0: the automatic choice).  Changes no count."""
        N.check(N.load_library().pgm_pair_plan_set_slice(self._h, int(rows)), "pair_plan_set_slice")

    def count_info(self, n_rows, n_strata=1, codes_ptr=0, ld=0, row0=0):
        """(rows per slice, slices, whether the 16-byte loads apply) of a count over such a window."""
        s, k, v = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        N.check(N.load_library().pgm_pair_count_info(self._h, ctypes.c_void_p(codes_ptr), int(ld), int(row0), int(n_rows),
                                                     int(n_strata), ctypes.byref(s), ctypes.byref(k), ctypes.byref(v)),
                "pair_count_info")
        return int(s.value), int(k.value), bool(v.value)

    def pair_index(self, u, v):
        if not 0 <= u < v < self.n_vars:
            raise ValueError(f"pair ({u}, {v}): need 0 <= u < v < {self.n_vars}")
        return u * self.n_vars - u * (u + 1) // 2 + (v - u - 1)

    def count_bytes(self, n_strata=1):
        return int(n_strata) * self.Sp * self.Sp * 8

    def _check_budget(self, n_strata):
        if self.count_bytes(n_strata) > self.budget:
            raise ValueError(f"pairwise counts of {n_strata} strata x {self.Sp} x {self.Sp} int64 take "
                             f"{self.count_bytes(n_strata)} bytes, above the budget of {self.budget} "
                             f"(fewer variables, or a larger `budget`)")

    # ------------------------------------------------------------------ launches
    def count(self, codes, stratum=None, n_strata=1, n_rows=None, row0=0, counts=None):
        """Add the rows [row0, row0 + n_rows) of the device codes [n_cols, ld] (uint8) to `counts` (a zeroed
        int64 tensor [n_strata, Sp, Sp] when None).  `stratum`: the code column whose state c < n_strata
        selects the stratum of a row (any other code there: counted nowhere).  Raises IndexError when a
        code is neither 255 nor a state."""
        import torch

        L = N.lib()
        n_cols, ld, n_rows = codes_window(codes, n_rows, row0)
        n_strata = int(n_strata)
        if stratum is None and n_strata != 1:
            raise ValueError("n_strata needs a stratum column")
        if counts is None:
            self._check_budget(max(n_strata, 1))
            counts = torch.zeros((max(n_strata, 1), self.Sp, self.Sp), dtype=torch.int64, device=codes.device)
        else:
            flat_tensor("counts", counts, n_strata * self.Sp * self.Sp, torch.int64, "int64")
        N.check(L.pgm_pair_count(self._h, N.ptr(codes), n_cols, ld, int(row0), n_rows,
                                 -1 if stratum is None else int(stratum), n_strata, N.ptr(counts), N.stream_handle()),
                "pair_count")
        return counts

    def _strata(self, counts):
        import torch

        if counts.dtype != torch.int64 or not counts.is_contiguous() or counts.numel() % (self.Sp * self.Sp) or \
                counts.numel() == 0:
            raise ValueError(f"counts must be a contiguous int64 device tensor [n_strata, {self.Sp}, {self.Sp}]")
        return counts.numel() // (self.Sp * self.Sp)

    def mi(self, counts):
        """(mi, hu, hv fp64; n int64), device tensors [n_strata, n_pairs], from the count tensor (pgm_pair_mi)."""
        import torch

        L = N.lib()
        ns = self._strata(counts)
        shape = (ns, self.n_pairs)
        mi, hu, hv = (torch.empty(shape, dtype=torch.float64, device=counts.device) for _ in range(3))
        n = torch.empty(shape, dtype=torch.int64, device=counts.device)
        N.check(L.pgm_pair_mi(self._h, N.ptr(counts), ns, N.ptr(mi), N.ptr(hu), N.ptr(hv), N.ptr(n), N.stream_handle()),
                "pair_mi")
        return mi, hu, hv, n

    def emi(self, counts):
        """The expected mutual information of every (stratum, pair): an fp64 device tensor (pgm_pair_emi)."""
        import torch

        L = N.lib()
        ns = self._strata(counts)
        emi = torch.empty((ns, self.n_pairs), dtype=torch.float64, device=counts.device)
        N.check(L.pgm_pair_emi(self._h, N.ptr(counts), ns, N.ptr(emi), N.stream_handle()), "pair_emi")
        return emi

    def block(self, counts, u, v, c=0):
        """The [cards[u], cards[v]] table of the pair u < v in stratum c: a view of `counts`."""
        self.pair_index(u, v)
        ou, ov = self.offsets[u], self.offsets[v]
        return counts.reshape(-1, self.Sp, self.Sp)[c, ou:ou + self.cards[u], ov:ov + self.cards[v]]


# ---------------------------------------------------------------------- host: statistics to edge weights
EPS = float(np.finfo(np.float64).eps)


def pair_weights(kind, mi, hu, hv, n, emi=None):
    """Edge weights from the pair statistics (numpy arrays of one shape, strata first when there are any):
    `mutual_info`, `normalized_mutual_info` (MI over the arithmetic mean of the entropies) or
    `adjusted_mutual_info` ((MI - EMI) / (mean H - EMI)), with scikit-learn's special cases: a side with
    one observed state has entropy exactly 0; MI is 0 when either side has; NMI and AMI are 1.0 when both
    have, AMI is 0.0 when one has, NMI is 0.0 when MI is; AMI's numerator and denominator are kept at
    least eps away from 0, sign preserved.  A table without rows (n = 0) weighs 0."""
    mi, hu, hv = (np.asarray(a, dtype=np.float64) for a in (mi, hu, hv))
    n = np.asarray(n)
    one_u, one_v = hu == 0.0, hv == 0.0
    mi = np.where(one_u | one_v, 0.0, mi)
    if kind == "mutual_info":
        w = mi
    elif kind == "normalized_mutual_info":
        mean = 0.5 * (hu + hv)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(mi == 0.0, 0.0, mi / mean)
        w = np.where(one_u & one_v, 1.0, w)
    elif kind == "adjusted_mutual_info":
        if emi is None:
            raise ValueError("adjusted_mutual_info needs the expected mutual information")
        emi = np.asarray(emi, dtype=np.float64)
        den = 0.5 * (hu + hv) - emi
        den = np.where(den < 0, np.minimum(den, -EPS), np.maximum(den, EPS))
        num = mi - emi
        num = np.where(num < 0, np.minimum(num, -EPS), np.maximum(num, EPS))
        w = np.where(one_u | one_v, 0.0, num / den)
        w = np.where(one_u & one_v, 1.0, w)
    else:
        raise ValueError(f"edge_weights_fn should either be 'mutual_info', 'adjusted_mutual_info', "
                         f"'normalized_mutual_info'or a function of form fun(array, array). Got: f{kind}")
    return np.where(n == 0, 0.0, w)


def stratified_weight(w, n):
    """sum_c p_c w_c per pair, p_c = n_c / sum_c n_c (the share of stratum c among the rows complete in the
    pair and the stratum column), the strata added in state order.  w, n: [n_strata, n_pairs]."""
    n = np.asarray(n, dtype=np.float64)
    total = n.sum(axis=0)
    out = np.zeros(w.shape[1])
    for c in range(w.shape[0]):
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(total > 0, n[c] / total, 0.0)
        out += p * w[c]
    return out


def weight_matrix(n_vars, values):
    """The symmetric [n_vars, n_vars] matrix of per-pair values (pair order of PairPlan), zero diagonal."""
    weights = np.zeros((n_vars, n_vars))
    indices = np.triu_indices(n_vars, k=1)
    weights[indices] = values
    weights.T[indices] = values
    return weights
