"""The continuous data behind GaussCITester and the Gaussian structure scores: a resident fp64 value matrix and
its moment matrix, computed once by the Gram kernel (pgm_lg_colsum, pgm_lg_gram) and left on the device.
BaseEstimator's state names (a sorted unique() per column) have no meaning for float data and are not
collected."""
from .. import _native as N
from . import _rounds as R

# most job columns (|K| + targets per job) one round of a batch keeps on the device
ROUND_COLUMNS = 1 << 24


class GaussData:
    def __init__(self, data):
        import pandas as pd

        if not isinstance(data, pd.DataFrame):
            raise ValueError(f"Variable data. Expected type: pandas.DataFrame. Got type: {type(data)}")
        self.data, self.variables = data, list(data.columns.values)
        self._values, self._n_rows, self._moments = None, len(data), None

    @classmethod
    def from_values(cls, X, variables, n_rows=None):
        """Over a resident fp64 value matrix X[len(variables), ld] (column c holds variables[c]), as
        LinearGaussianBayesianNetwork.simulate_values leaves it: nothing is uploaded."""
        from ..models import _lg

        self = cls.__new__(cls)
        self.data, self.variables = None, list(variables)
        n_cols, _, n = _lg.values_window(X, n_rows, 0)
        if n_cols < len(self.variables):
            raise ValueError(f"X has {n_cols} columns for {len(self.variables)} variables")
        self._values, self._n_rows, self._moments = X, n, None
        return self

    @property
    def d(self):
        return len(self.variables)

    @property
    def n_rows(self):
        return self._n_rows

    def gram(self):
        """(G [d + 1, d + 1], shift [d]) device tensors of all the columns; the first call computes them."""
        if self._moments is None:
            from ..models import _lg
            from ..models.LinearGaussianBayesianNetwork import LinearGaussianBayesianNetwork as LG

            if self._values is None:
                self._values = LG._upload(self.data, self.variables)
            self._plan = _lg.GramPlan(range(self.d))
            self._moments = self._plan.moments_device(self._values, self._n_rows, 0)
        return self._moments

    def columns(self, names):
        """Column positions of variable names (KeyError for an unknown one)."""
        col = self.__dict__.get("_col")
        if col is None:
            col = self._col = {v: j for j, v in enumerate(self.variables)}
        for v in names:
            if v not in col:
                raise KeyError(v)
        return [col[v] for v in names]

    def run(self, jobs, call):
        """The [2, len(jobs)] fp64 host array of `call(batch, G, shift)`'s first two outputs, round by round:
        one launch per distinct (|K|, targets) and one download per round."""
        import numpy as np
        import torch

        from ..inference.batch import download
        from ..models import _lg

        out = np.empty((2, len(jobs)), dtype=np.float64)
        if not jobs:
            return out
        G, shift = self.gram()
        for idx in R.rounds([len(K) + len(T) for K, T in jobs], ROUND_COLUMNS):
            batch = _lg.SchurJobs(self.d, [jobs[i] for i in idx])
            a, b, _ = call(batch, G, shift)
            out[:, idx] = download(torch.stack([a, b]).contiguous())
        return out


def cap_error(what, count, room):
    return ValueError(f"{count} {what}: one job takes at most {room} (PGM_LGS_MAX_COND = {N.LGS_MAX_COND} "
                      f"conditioning columns, the intercept's among them)")
