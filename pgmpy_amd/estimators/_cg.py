"""Binding of the pgm_cg_* entry points (include/pgmhip.h "conditional-Gaussian scores", pgmpy_amd/csrc/pgmcg.hip)
and the mixed data behind LogLikelihoodCondGauss, BICCondGauss and AICCondGauss: the discrete columns as the
estimator's resident uint8 code matrix, the continuous ones as a resident fp64 value matrix, both uploaded once.

A column is continuous when its pandas dtype is numeric (integers and bools included) and discrete when it
is object or categorical, as the reference's preprocess_data decides it.
"""
import ctypes

import numpy as np

from .. import _native as N
from .._plan import Plan, codes_window, flat_tensor
from . import _rounds as R
from .base import BaseEstimator


class CgPlan(Plan):
    """families: (code columns, cardinalities, value columns, variable is discrete) with the variable first
    among the code columns when it is discrete and last among the value columns when it is continuous."""
    _destroy = "pgm_cg_plan_destroy"

    def __init__(self, families):
        L = N.load_library()  # building and inspecting a plan needs no device
        self.families = [([int(c) for c in dc], [int(k) for k in cards], [int(c) for c in cc], bool(disc))
                         for dc, cards, cc, disc in families]
        n = len(self.families)
        fams = (N.CgFamily * max(n, 1))()
        for f, (dc, cards, cc, disc) in enumerate(self.families):
            if len(dc) != len(cards):
                raise ValueError(f"family {f}: {len(dc)} discrete columns, {len(cards)} cardinalities")
            fams[f].n_disc, fams[f].n_cont, fams[f].var_discrete = len(dc), len(cc), int(disc)
            for i, (c, k) in enumerate(list(zip(dc, cards))[:N.PGM_MAX_DIMS]):  # the library refuses a longer list by its length
                fams[f].dcol[i], fams[f].card[i] = c, k
            for i, c in enumerate(cc[:N.CG_MAX_CONT + 1]):
                fams[f].ccol[i] = c
        self._h = ctypes.c_void_p()
        N.check(L.pgm_cg_plan_create(fams, n, ctypes.byref(self._h)), "cg_plan_create")
        self.info = N.CgInfo()
        lay = (ctypes.c_int64 * (N.CG_LAYOUT * n))()
        N.check(L.pgm_cg_plan_info(self._h, ctypes.byref(self.info), lay), "cg_plan_info")
        keys = ("mp", "Q", "operand_rows", "tiles", "mom_off", "jobs")
        self.layout = [dict(zip(keys, lay[N.CG_LAYOUT * f:N.CG_LAYOUT * (f + 1)])) for f in range(n)]
        self.moments_size = int(self.info.moments_size)

    def set_slice(self, rows):
        """Force the rows per slice of the moments launches (0: the automatic choice)."""
        N.check(N.load_library().pgm_cg_plan_set_slice(self._h, int(rows)), "cg_plan_set_slice")

    def moments_info(self, n_rows, x_ptr=0, ld_x=0, row0=0):
        """(rows per slice, slices, passes, whether the 16-byte loads apply) of a moments call over such a window."""
        s, k, p, v = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        N.check(N.load_library().pgm_cg_moments_info(self._h, ctypes.c_void_p(x_ptr), int(ld_x), int(row0), int(n_rows),
                                                     ctypes.byref(s), ctypes.byref(k), ctypes.byref(p), ctypes.byref(v)),
                "cg_moments_info")
        return int(s.value), int(k.value), int(p.value), bool(v.value)

    def moments(self, codes, X, shift, n_rows, row0=0):
        """The flat fp64 device buffer of every family's [Q, mp, mp] grouped moments over the rows
        [row0, row0 + n_rows) of the device codes [n_code_cols, ld] (uint8; None without discrete columns) and
        values X [n_value_cols, ld] (fp64; None without continuous ones), shift one entry per value column.
        Raises IndexError when a code is neither 255 nor a state."""
        import torch

        from ..models import _lg

        L = N.lib()
        n_code_cols, ld_codes = (0, int(row0) + int(n_rows)) if codes is None else codes_window(codes, n_rows, row0)[:2]
        n_value_cols, ld_x = (0, int(row0) + int(n_rows)) if X is None else _lg.values_window(X, n_rows, row0)[:2]
        if X is not None:
            flat_tensor("shift", shift, n_value_cols, entries="with one entry per value column")
        device = (codes if codes is not None else X).device
        out = torch.empty(max(self.moments_size, 1), dtype=torch.float64, device=device)
        N.check(L.pgm_cg_moments(self._h, N.ptr(codes), n_code_cols, ld_codes, N.ptr(X), n_value_cols, ld_x, int(row0),
                                 int(n_rows), N.ptr(shift) if X is not None else None, N.ptr(out), N.stream_handle()), "cg_moments")
        return out

    def family_moments(self, flat, f):
        """Family f's [Q, mp, mp] view of a moments buffer (device tensor or ndarray)."""
        lay = self.layout[f]
        return flat[lay["mom_off"]:lay["mom_off"] + lay["Q"] * lay["mp"] ** 2].reshape(lay["Q"], lay["mp"], lay["mp"])

    def score(self, moments):
        """(ll fp64, n_complete, n_observed, n_dropped int64) device tensors, one entry per family."""
        import torch

        L = N.lib()
        flat_tensor("moments", moments, self.moments_size)
        n = len(self.families)
        ll = torch.empty(n, dtype=torch.float64, device=moments.device)
        counts = torch.empty((3, n), dtype=torch.int64, device=moments.device)
        N.check(L.pgm_cg_score(self._h, N.ptr(moments), None, N.ptr(ll), N.ptr(counts[0]), N.ptr(counts[1]), N.ptr(counts[2]),
                               N.stream_handle()), "cg_score")
        return ll, counts[0], counts[1], counts[2]


def is_continuous(dtype):
    import pandas as pd

    return pd.api.types.is_numeric_dtype(dtype) and not isinstance(dtype, pd.CategoricalDtype)


class CondGaussData:
    def __init__(self, data, state_names=None):
        import pandas as pd

        if not isinstance(data, pd.DataFrame):
            raise ValueError(f"Variable data. Expected type: pandas.DataFrame. Got type: {type(data)}")
        self.data, self.variables = data, list(data.columns.values)
        self.value_variables = [v for v in self.variables if is_continuous(data[v].dtype)]
        self.code_variables = [v for v in self.variables if v not in set(self.value_variables)]
        # the discrete columns go through the estimators' own state names and encoder
        self._discrete = BaseEstimator(data.loc[:, self.code_variables], state_names=state_names)
        self.state_names = self._discrete.state_names
        self.cardinalities = [len(self.state_names[v]) for v in self.code_variables]
        self._n_rows, self._resident, self._ready = len(data), None, None
        self._index()

    @classmethod
    def from_columns(cls, codes, code_variables, cardinalities, X, value_variables, n_rows=None):
        """Over resident data, nothing uploaded: the uint8 code matrix codes[len(code_variables), ld] with its
        cardinalities and the fp64 value matrix X[len(value_variables), ld] (either may be None with an empty
        list); the first n_rows rows (all when None)."""
        self = cls.__new__(cls)
        self.data, self._discrete, self.state_names = None, None, None
        self.code_variables, self.value_variables = list(code_variables), list(value_variables)
        self.variables = self.code_variables + self.value_variables
        self.cardinalities = [int(k) for k in cardinalities]
        if len(self.cardinalities) != len(self.code_variables):
            raise ValueError(f"{len(self.code_variables)} discrete variables, {len(self.cardinalities)} cardinalities")
        lds = [int(t.shape[1]) for t in (codes, X) if t is not None]
        if not lds or (n_rows is None and len(set(lds)) > 1):
            raise ValueError("codes and X must be given (one may be None) with the same number of rows, or n_rows")
        self._n_rows = min(lds) if n_rows is None else int(n_rows)
        self._resident, self._ready = (codes if self.code_variables else None, X if self.value_variables else None), None
        self._index()
        return self

    def _index(self):
        self._code_of = {v: j for j, v in enumerate(self.code_variables)}
        self._value_of = {v: j for j, v in enumerate(self.value_variables)}

    @property
    def n_rows(self):
        return self._n_rows

    def resident(self):
        """(codes, X, shift, observed states per code column): uploaded and computed by the first call."""
        if self._ready is not None:
            return self._ready
        import torch

        from ..inference.batch import download
        from ..models import _lg
        from ..models.LinearGaussianBayesianNetwork import LinearGaussianBayesianNetwork as LG

        if self._resident is None:
            codes = self._discrete._codes()[0] if self.code_variables else None
            X = LG._upload(self.data, self.value_variables) if self.value_variables else None
            self._resident = (codes, X)
        codes, X = self._resident
        n, shift, seen = self._n_rows, None, []
        if X is not None:
            d = len(self.value_variables)
            sums, counts = _lg.GramPlan(range(d)).colsum(X, n, 0)
            shift = sums / counts.to(torch.float64)
            gaps = ~torch.isfinite(shift)  # a column with a missing cell: the mean of the cells it has
            if bool(gaps.any()):
                shift = torch.where(gaps, torch.nan_to_num(torch.nanmean(X[:d, :n], dim=1), nan=0.0, posinf=0.0, neginf=0.0), shift)
            shift = shift.contiguous()
        if codes is not None:  # the observed states of every discrete column (nunique), for the penalties
            per_col = [torch.bincount(codes[c, :n].to(torch.int64), minlength=256)[:N.PGM_EV_MISSING] > 0
                       for c in range(len(self.code_variables))]
            seen = [int(x) for x in download(torch.stack(per_col).sum(dim=1).contiguous())]
        self._ready = (codes, X, shift, seen)
        return self._ready

    def family(self, variable, parents):
        """(CgPlan family, (variable is discrete, code positions of the discrete parents, continuous parents))."""
        code_of, value_of = self._code_of, self._value_of
        parents = list(parents)
        for v in [variable] + parents:
            if v not in code_of and v not in value_of:
                raise KeyError(v)
        if len(set(parents)) != len(parents) or variable in parents:
            raise ValueError(f"a family names a variable twice: {variable}, {parents}")
        disc = variable in code_of
        D = [code_of[p] for p in parents if p in code_of]
        C = [value_of[p] for p in parents if p in value_of]
        dcols = ([code_of[variable]] if disc else []) + D
        ccols = C + ([] if disc else [value_of[variable]])
        return (dcols, [self.cardinalities[c] for c in dcols], ccols, disc), (disc, code_of.get(variable), D, len(C))

    def n_parameters(self, shape, seen):
        """The reference's _get_num_parameters: q the product of the observed state counts above 1 of the discrete
        parents; q (|C| + 2) for a continuous variable, q (r - 1) for a discrete one without continuous parents,
        q (r - 1) (|C| + 2) with."""
        disc, v, D, n_cont = shape
        q = 1
        for c in D:
            q *= seen[c] if seen[c] > 1 else 1
        if not disc:
            return q * (n_cont + 2)
        return q * (seen[v] - 1) * (n_cont + 2 if n_cont else 1)

    def run(self, families):
        """[(ll, n_complete, n_observed, n_dropped, parameters)] per (variable, parents): per round one plan, one
        moments launch, one score launch and one download."""
        import torch

        from ..inference.batch import download

        fams = [self.family(v, ps) for v, ps in families]
        if not fams:
            return []
        codes, X, shift, seen = self.resident()
        sizes = []
        for (dc, cards, cc, _), _ in fams:
            mp = 1
            while mp < len(cc) + 1:
                mp *= 2
            sizes.append(int(np.prod(cards, dtype=object)) * mp * mp)
        out = [None] * len(fams)
        for idx in R.rounds(sizes, R.SCORE_BIN_BUDGET):
            plan = CgPlan([fams[i][0] for i in idx])
            ll, n, obs, drop = plan.score(plan.moments(codes, X, shift, self._n_rows))
            host = download(torch.stack([ll.view(torch.int64), n, obs, drop]).contiguous())  # one copy: raw 64-bit words
            for k, i in enumerate(idx):
                out[i] = (float(host[0].view(np.float64)[k]), int(host[1][k]), int(host[2][k]), int(host[3][k]),
                          self.n_parameters(fams[i][1], seen))
        return out
