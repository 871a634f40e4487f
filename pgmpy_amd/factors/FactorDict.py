"""FactorDict (mirror of pgmpy/factors/FactorDict.py): a dict of clique -> DiscreteFactor with the vector-space
operations MarginalEstimator's host API needs (`+`, `-`, scalar `*`, `dot`), `product` and the empirical marginals of
a data frame.

Everything here is off the hot path (MirrorDescentEstimator's optimisation runs in one launch of k_md on flat
tables) and works on the factors' host values, so it needs no device.  Two factors of one key may order their
variables differently; the result keeps the left one's order.

Deviation: `from_dataframe` takes an optional `state_names`.  The reference sizes every table by `nunique` of the
column, so a state that does not occur loses its cell and the table no longer lines up with the clique's; with
`state_names` the table has one cell per named state, zero where nothing was observed.
"""
from numbers import Number

import numpy as np

from .base import factor_product
from .discrete import DiscreteFactor


def _like(f, values):
    return DiscreteFactor(list(f.variables), [int(c) for c in f.cardinality], values,
                          state_names={v: list(f.state_names[v]) for v in f.variables})


def _aligned(f, g):
    """g's host values in f's variable order."""
    if set(g.variables) != set(f.variables):
        raise ValueError(f"the factors of one key differ in scope: {f.variables} and {g.variables}")
    return np.transpose(np.asarray(g.values), [g.variables.index(v) for v in f.variables])


class FactorDict(dict):
    @classmethod
    def from_dataframe(cls, df, marginals, state_names=None):
        """{marginal: the contingency table of its columns}, counted on the host (one np.bincount per marginal)."""
        if df.isnull().values.any():
            raise ValueError("df cannot contain None or np.nan values.")
        out = cls({})
        for marginal in marginals:
            names, codes = {}, []
            for v in marginal:
                col = df[v].to_numpy()
                names[v] = list(state_names[v]) if state_names and v in state_names else sorted(set(col.tolist()))
                to_no = {s: i for i, s in enumerate(names[v])}
                try:
                    codes.append(np.fromiter((to_no[s] for s in col.tolist()), dtype=np.int64, count=len(col)))
                except KeyError as e:
                    raise ValueError(f"Data contains unexpected states for variable: {v}.") from e
            card = [len(names[v]) for v in marginal]
            flat = np.ravel_multi_index(codes, card) if len(df) else np.zeros(0, dtype=np.int64)
            counts = np.bincount(flat, minlength=int(np.prod(card))).astype(np.float64)
            out[marginal] = DiscreteFactor(list(marginal), card, counts, state_names=names)
        return out

    def get_factors(self):
        return set(self.values())

    def __mul__(self, const):
        return FactorDict({c: _like(f, float(const) * np.asarray(f.values)) for c, f in self.items()})

    __rmul__ = __mul__

    def __add__(self, other):
        if isinstance(other, Number):
            return FactorDict({c: _like(f, np.asarray(f.values) + other) for c, f in self.items()})
        return FactorDict({c: _like(f, np.asarray(f.values) + _aligned(f, other[c])) for c, f in self.items()})

    def __sub__(self, other):
        return self + -1 * other

    def dot(self, other):
        return sum(float((np.asarray(f.values) * _aligned(f, other[c])).sum()) for c, f in self.items())

    def product(self):
        return factor_product(*self.get_factors())
