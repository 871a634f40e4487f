"""Conditional-independence tests (mirror of pgmpy/estimators/CITests.py:14-66, 280-571: chi_square, g_sq,
log_likelihood, modified_log_likelihood, power_divergence, pearsonr, get_callable_ci_test).

The reference runs one pandas groupby and one scipy.stats.chi2_contingency per stratum of one test.  Here
`CITester.tests(triples)` runs any number of tests X _|_ Y | Z at once: a test is the fit-plan family
(X, Y, Z...), so one fused count launch over the estimator's device codes (pgm_fit_count) fills every
contingency table [X][Y][Z...], one CI launch turns the tables into (statistic, dof, p-value) per test on
the device (pgm_fit_citest) and one download brings the three arrays back.  The module functions are the
one-test case with the reference's signature; they encode the frame on every call (a DataFrame is
mutable, so caching on its identity is not safe).  PC uses a CITester directly.

Deviations: a row with a missing value in any of X, Y, Z is left out of that test (the
reference, with a non-empty Z, counts NaN as a state of X or Y); a never-observed category of a
categorical column is dropped as an empty row or column (the reference raises ValueError when Z is
empty); every column is discrete whatever its dtype for the discrete tests; gcm, pillai and
independence_match are not built.

Continuous data: `GaussCITester.tests(triples)` runs any number of partial-correlation tests at once from
the moment matrix of the columns, computed once per tester by the fp64 Gram kernel (pgm_lg_gram) and left
on the device: one launch per distinct |Z| and one download per round (pgm_lgs_pcorr), the n rows are
not read again.  `pearsonr` is the one-test case with the reference's signature.  The NAME "pearsonr" stays
closed in get_callable_ci_test: pass the function object, or a GaussCITester.  Deviations: a
constant X or Y, n <= 2 or a NaN cell give a NaN coefficient and p-value (the reference warns or raises);
collinear conditioning columns are dropped pivot by pivot instead of lstsq's minimum-norm solution (the
residuals are the same); `intercept=True` (off by default) regresses with an intercept.
"""
import numpy as np

from .. import engine as E
from . import _rounds as R
from ._fit import FitPlan
from ._gauss import GaussData, cap_error
from .base import BaseEstimator

# scipy.stats.power_divergence's names
LAMBDA_NAMES = {"pearson": 1.0, "log-likelihood": 0.0, "freeman-tukey": -0.5, "mod-log-likelihood": -1.0,
                "neyman": -2.0, "cressie-read": 2.0 / 3.0}
# closed as NAMES: gcm, pillai and independence_match are not built; pearsonr is built but reached through the
# function object or a GaussCITester only
_NOT_BUILT = ("pearsonr", "gcm", "pillai", "independence_match")


def lambda_value(lambda_):
    """A float for a float or one of scipy's names (None: Pearson, scipy's default)."""
    if lambda_ is None:
        return 1.0
    if isinstance(lambda_, str):
        if lambda_ not in LAMBDA_NAMES:
            raise ValueError(f"invalid string for lambda_: {lambda_!r}. Valid strings are {sorted(LAMBDA_NAMES)}")
        return LAMBDA_NAMES[lambda_]
    value = float(lambda_)
    if not np.isfinite(value):
        raise ValueError(f"lambda_ must be finite, got {lambda_!r}")
    return value


def _triple(X, Y, Z):
    if not hasattr(Z, "__iter__") or isinstance(Z, str):
        raise ValueError(f"Z must be an iterable. Got object type: {type(Z)}")
    Z = list(Z)
    if X in Z or Y in Z:
        raise ValueError(f"The variables X or Y can't be in Z. Found {X if X in Z else Y} in Z.")
    return X, Y, Z


class CITester(BaseEstimator):
    """Batched power-divergence tests over one data set, encoded once onto the device."""

    def __init__(self, data, state_names=None):
        super(CITester, self).__init__(data, state_names=state_names)

    @classmethod
    def from_codes(cls, codes, variables, state_names):
        """A tester over device codes [len(variables), n] (uint8, 255 = missing) that are already resident,
        as BayesianModelSampling.forward_sample_codes leaves them: nothing is encoded or uploaded."""
        self = cls.__new__(cls)
        self.data, self.variables = None, list(variables)
        self.state_names = {v: list(state_names[v]) for v in self.variables}
        self._encoded = (codes, {v: j for j, v in enumerate(self.variables)})
        return self

    @E.serialized
    def tests(self, triples, lambda_=1.0):
        """(stat fp64, pvalue fp64, dof int64) numpy arrays, one entry per (X, Y, Z) of `triples`."""
        from ..inference.batch import download
        import torch

        lam = lambda_value(lambda_)
        triples = [_triple(X, Y, Z) for X, Y, Z in triples]
        out = np.empty((3, len(triples)), dtype=np.float64)
        if not triples:
            return out[0], out[1], out[2].astype(np.int64)
        codes, col_of = self._codes()
        fams = [self._family(X, [Y] + Z, col_of) for X, Y, Z in triples]
        sizes = [int(np.prod(cards, dtype=object)) for _, cards in fams]
        for idx in R.rounds(sizes, R.SCORE_BIN_BUDGET):
            plan = FitPlan([fams[i] for i in idx])
            stat, dof, pvalue = plan.citest(plan.count(codes), lam, yates=True)
            out[:, idx] = download(torch.stack([stat, pvalue, dof.to(torch.float64)]).contiguous())
        return out[0], out[1], out[2].astype(np.int64)

    def independent(self, triples, significance_level=0.01, lambda_=1.0):
        """pvalue >= significance_level per test (a NaN p-value is not independent, as in the reference)."""
        _, pvalue, _ = self.tests(triples, lambda_)
        with np.errstate(invalid="ignore"):
            return pvalue >= significance_level


def power_divergence(X, Y, Z, data, boolean=True, lambda_="cressie-read", **kwargs):
    """The Cressie-Read power-divergence test of X _|_ Y | Z (CITests.py:372-499): (chi, p_value, dof), or
    with boolean=True whether p_value >= kwargs["significance_level"]."""
    X, Y, Z = _triple(X, Y, Z)
    stat, pvalue, dof = CITester(data).tests([(X, Y, Z)], lambda_)
    if boolean:
        return bool(pvalue[0] >= kwargs["significance_level"])
    return float(stat[0]), float(pvalue[0]), int(dof[0])


def chi_square(X, Y, Z, data, boolean=True, **kwargs):
    return power_divergence(X, Y, Z, data, boolean=boolean, lambda_="pearson", **kwargs)


def g_sq(X, Y, Z, data, boolean=True, **kwargs):
    return power_divergence(X, Y, Z, data, boolean=boolean, lambda_="log-likelihood", **kwargs)


def log_likelihood(X, Y, Z, data, boolean=True, **kwargs):
    return power_divergence(X, Y, Z, data, boolean=boolean, lambda_="log-likelihood", **kwargs)


def modified_log_likelihood(X, Y, Z, data, boolean=True, **kwargs):
    return power_divergence(X, Y, Z, data, boolean=boolean, lambda_="mod-log-likelihood", **kwargs)


class GaussCITester(GaussData):
    """Batched partial-correlation tests over one continuous data set.  The columns are uploaded once (or are
    resident already: from_values) and their moment matrix is computed once, by the first test."""

    def _jobs(self, triples, intercept):
        """[(K, targets)] in column positions; every argument error comes from here, before the device."""
        from .. import _native as N

        d, room = self.d, N.LGS_MAX_COND - (1 if intercept else 0)
        jobs = []
        for X, Y, Z in triples:
            X, Y, Z = _triple(X, Y, Z)
            cx, cy, *K = self.columns([X, Y] + Z)
            if cx == cy or len(set(K)) != len(K):
                raise ValueError(f"a test names a variable twice: {X}, {Y}, {Z}")
            if len(K) > room:
                raise cap_error("conditioning variables", len(K), room)
            jobs.append(([d] + K, [cx, cy]) if intercept else (K, [cx, cy, d]))
        return jobs

    @E.serialized
    def tests(self, triples, intercept=False):
        """(coef fp64, pvalue fp64) numpy arrays, one entry per (X, Y, Z) of `triples`."""
        jobs = self._jobs(list(triples), intercept)
        out = self.run(jobs, lambda batch, G, shift: batch.pcorr(G, shift, intercept=intercept))
        return out[0], out[1]

    def independent(self, triples, significance_level=0.01, intercept=False):
        """pvalue >= significance_level per test (a NaN p-value is not independent)."""
        _, pvalue = self.tests(triples, intercept=intercept)
        with np.errstate(invalid="ignore"):
            return pvalue >= significance_level


def pearsonr(X, Y, Z, data, boolean=True, **kwargs):
    """The partial correlation of X and Y given Z on continuous data (CITests.py:502-571): X and Y are regressed on
    Z without an intercept and the residuals correlated; (coefficient, p_value), or with boolean=True whether
    p_value >= kwargs["significance_level"]."""
    if not hasattr(Z, "__iter__"):
        raise ValueError(f"Variable Z. Expected type: iterable. Got type: {type(Z)}")
    coef, pvalue = GaussCITester(data).tests([(X, Y, list(Z))])
    if boolean:
        return bool(pvalue[0] >= kwargs["significance_level"])
    return float(coef[0]), float(pvalue[0])


_DISCRETE = {"chi_square": chi_square, "g_sq": g_sq, "log_likelihood": log_likelihood,
             "modified_log_likelihood": modified_log_likelihood, "power_divergence": power_divergence}
# the lambda_ of the named tests (power_divergence: its lambda_ keyword); PC batches these through a CITester
BUILTIN_LAMBDA = {chi_square: "pearson", g_sq: "log-likelihood", log_likelihood: "log-likelihood",
                  modified_log_likelihood: "mod-log-likelihood", power_divergence: None}


def get_callable_ci_test(test, data=None):
    """The test function for a name, a callable (returned as it is) or None (chi_square: every column is
    discrete here) (CITests.py:14-66)."""
    if callable(test):
        return test
    if test is None:
        if data is None:
            raise ValueError("Cannot determine a suitable CI test as data is None.", "Please specify CI test to use")
        return chi_square
    if isinstance(test, str):
        name = test.lower()
        if name in _NOT_BUILT:
            raise ValueError(f"The continuous, mixed and independence-matching tests are not built as names: {test} "
                             f"(pearsonr: pass the function CITests.pearsonr or a GaussCITester). "
                             f"`ci_test` must either be one of {list(_DISCRETE)}, or a callable.")
        if name not in _DISCRETE:
            raise ValueError(f"`ci_test` must either be one of {list(_DISCRETE)}, or a callable. Got:{test}")
        return _DISCRETE[name]
    raise ValueError(f"`ci_test` must either be one of {list(_DISCRETE)}, or a callable. Got:{test}")
