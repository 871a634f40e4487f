"""Structure scores (mirror of pgmpy/estimators/StructureScore.py:15-1189, the discrete and the Gaussian
classes): K2, BDeu, BDs, LogLikeliHood, BIC, AIC, LogLikelihoodGauss, BICGauss, AICGauss and get_scoring_method.

The reference scores one family per call from a pandas groupby.  Here `local_scores(families)` scores
any number of families at once: one FitPlan, one fused count launch over the estimator's device codes
(pgm_fit_count), one score launch that turns the count tables into one number per family on the device
(pgm_fit_score), and one download of len(families) doubles (BDeu and BDs: three numbers per family, the
observed columns and states beside the score).  The constants that depend only on the family's shape and
the equivalent sample size are added on the host with math.lgamma, as the reference does.  `local_score`
is `local_scores` of one family.

Deviations: every column is discrete whatever its dtype; a variable with 255 or more states
raises the encoders' ValueError; the conditional-Gaussian scores are not built.

The Gaussian scores (LogLikelihoodGauss, BICGauss, AICGauss) score any number of families in one launch from
the moment matrix of the continuous columns, computed once per scorer by the fp64 Gram kernel and left on
the device (pgm_lgs_score): the concentrated log-likelihood -n/2 (log(2 pi rss / n) + 1) that the reference
reads from statsmodels' Gaussian GLM as `llf`, with df_model the rank of the parents.  Their NAMES ("ll-g",
"bic-g", "aic-g") stay closed in get_scoring_method: pass an instance.
"""
from math import lgamma, log

import numpy as np

from .. import _native as N
from .. import engine as E
from ._fit import FitPlan
from ._gauss import GaussData, cap_error
from ._rounds import SCORE_BIN_BUDGET, rounds as _rounds  # noqa: F401  (module attributes the tests patch)
from .base import BaseEstimator

_DISCRETE = ("k2", "bdeu", "bds", "bic-d", "aic-d", "ll-d")
_NOT_BUILT = ("bic-g", "ll-g", "aic-g", "bic-cg", "ll-cg", "aic-cg")
_OLD_NAMES = ("k2score", "bdeuscore", "bdsscore", "bicscore", "aicscore")


def get_scoring_method(scoring_method, data, use_cache=True):
    """(score, score) for a name or a StructureScore instance (StructureScore.py:15-89).  The score
    cache of the reference lives in HillClimbSearch here, so both entries are the same object."""
    names = {"k2": K2, "bdeu": BDeu, "bds": BDs, "bic-d": BIC, "aic-d": AIC, "ll-d": LogLikeliHood}
    if isinstance(scoring_method, str):
        name = scoring_method.lower()
        if name in _OLD_NAMES:
            raise ValueError("The scoring method names have been changed. Please refer the documentation.")
        if name in _NOT_BUILT:
            raise ValueError(f"The Gaussian and conditional-Gaussian scores are not built as names: {scoring_method} "
                             f"(Gaussian: pass an instance of LogLikelihoodGauss, BICGauss or AICGauss). "
                             f"scoring_method should be one of {list(_DISCRETE)}")
        if name not in names:
            raise ValueError("Unknown scoring method. Please refer documentation for a list of supported score metrics.")
        score = names[name](data=data)
    elif scoring_method is None:
        score = BIC(data=data)  # the reference picks the first discrete method
    elif isinstance(scoring_method, StructureScore):
        score = scoring_method
    else:
        raise ValueError(f"scoring_method should either be one of {list(_DISCRETE)} or an instance of StructureScore")
    return score, score


class StructureScore(BaseEstimator):
    def __init__(self, data, **kwargs):
        super(StructureScore, self).__init__(data, **kwargs)

    # ------------------------------------------------------------------ scoring
    @E.serialized
    def local_scores(self, families):
        """The local score of every (variable, parents) family, as a list of floats."""
        families = [(v, list(ps)) for v, ps in families]
        if not families:
            return []
        codes, col_of = self._codes()
        fams = [self._family(v, ps, col_of) for v, ps in families]
        sizes = [int(np.prod(cards, dtype=object)) for _, cards in fams]
        out = [None] * len(fams)
        for idx in _rounds(sizes, SCORE_BIN_BUDGET):
            plan = FitPlan([fams[i] for i in idx])
            counts = plan.count(codes)
            shapes = [(fams[i][1][0], sizes[i] // fams[i][1][0], len(fams[i][0]) > 1) for i in idx]
            for i, s in zip(idx, self._score_round(plan, counts, shapes)):
                out[i] = float(s)
        return out

    def local_score(self, variable, parents):
        return self.local_scores([(variable, parents)])[0]

    def _score_round(self, plan, counts, shapes):
        """Scores of one plan's families from its device count tables; shapes: (r, q, has parents) per family."""
        raise NotImplementedError("StructureScore is abstract: use K2, BDeu, BDs, LogLikeliHood, BIC or AIC")

    def score(self, model):
        """Sum of the local scores of the model's families plus the structure prior (:150-196)."""
        nodes = list(model.nodes())
        score = 0
        for s in self.local_scores([(node, list(model.predecessors(node))) for node in nodes]):
            score += s
        score += self.structure_prior(model)
        return score

    def structure_prior(self, model):
        return 0

    def structure_prior_ratio(self, operation):
        return 0


def _download(t):
    from ..inference.batch import download

    return download(t)


class K2(StructureScore):
    """BD mode with alpha = r, beta = 1 over the OBSERVED columns only, plus q * lgamma(r) for all q
    columns (:346-380: reindex=False and no adjustment for the dropped columns)."""

    def _score_round(self, plan, counts, shapes):
        alpha = E.to_device(np.array([r for r, q, _ in shapes], dtype=np.float64))
        beta = E.to_device(np.ones(len(shapes)))
        s = _download(plan.score(counts, N.SCORE_BD | N.SCORE_SKIP_EMPTY, alpha, beta))
        return [s[f] + q * lgamma(r) for f, (r, q, _) in enumerate(shapes)]


class BDeu(StructureScore):
    """BD mode with alpha = ess / q, beta = ess / (q r) over all q columns (:462-494: with its
    adjustment the reference's sum over the observed columns is the sum over all of them), less the
    terms of the state rows the reference drops (_dropped_rows)."""

    def __init__(self, data, equivalent_sample_size=10, **kwargs):
        self.equivalent_sample_size = equivalent_sample_size
        super(BDeu, self).__init__(data, **kwargs)

    @staticmethod
    def _dropped_rows(r, states_seen, has_parents):
        """State rows missing from the reference's state_counts(reindex=False): for a family with
        parents its groupby(observed=True) has no row for a state that never occurs in a complete row
        (base.py:152-174), so lgamma(0 + beta) is left out once per such state and observed column,
        while the constants and the adjustment still count all r states.  Without parents the table is
        reindexed to all states (base.py:135-139)."""
        return r - states_seen if has_parents else 0

    @staticmethod
    def _device_outputs(scores, observed, states_seen):
        """(scores, observed columns, observed states) per family in one download."""
        import torch

        out = _download(torch.stack([scores, observed.to(torch.float64), states_seen.to(torch.float64)]).contiguous())
        return out[0], [int(x) for x in out[1]], [int(x) for x in out[2]]

    def _score_round(self, plan, counts, shapes):
        ess = self.equivalent_sample_size
        a = [ess / q for r, q, _ in shapes]
        b = [ess / (q * r) for r, q, _ in shapes]
        s, q_obs, seen = self._device_outputs(
            *plan.score(counts, N.SCORE_BD, E.to_device(np.array(a, dtype=np.float64)),
                        E.to_device(np.array(b, dtype=np.float64)), want_observed=True), plan.states_observed(counts))
        return [s[f] - self._dropped_rows(r, seen[f], has_parents) * q_obs[f] * lgamma(b[f])
                + q * lgamma(a[f]) - (q * r) * lgamma(b[f]) for f, (r, q, has_parents) in enumerate(shapes)]


class BDs(BDeu):
    """alpha = ess / (observed columns) depends on the data (:654-685): a first launch counts the
    observed columns, alpha is formed from them on the device, a second launch scores the observed
    columns; the tables stay on the device."""

    def __init__(self, data, equivalent_sample_size=10, **kwargs):
        super(BDs, self).__init__(data, equivalent_sample_size, **kwargs)

    def structure_prior_ratio(self, operation):
        """Marginal uniform prior (:547-581): an added arc costs log 2, a removed one gains it."""
        return {"+": -log(2.0), "-": log(2.0)}.get(operation, 0)

    def structure_prior(self, model):
        """Marginal uniform prior (:583-616): each of the n (n - 1) / 2 node pairs has no arc with
        probability 1/2 and either direction with 1/4, so the log prior is -(edges + pairs) log 2."""
        n = float(model.number_of_nodes())
        return -(float(model.number_of_edges()) + n * (n - 1) / 2.0) * log(2.0)

    def _score_round(self, plan, counts, shapes):
        import torch

        ess = self.equivalent_sample_size
        _, observed = plan.score(counts, N.SCORE_LL, want_observed=True)
        if bool((observed == 0).any()):
            raise ZeroDivisionError("division by zero: a family has no complete row (no observed parent configuration)")
        alpha = (float(ess) / observed.to(torch.float64)).contiguous()
        b = [ess / (q * r) for r, q, _ in shapes]
        s, q_obs, seen = self._device_outputs(
            plan.score(counts, N.SCORE_BD | N.SCORE_SKIP_EMPTY, alpha, E.to_device(np.array(b, dtype=np.float64))),
            observed, plan.states_observed(counts))
        out = []
        for f, (r, q, has_parents) in enumerate(shapes):
            a = ess / q_obs[f]
            empty = q - q_obs[f]
            out.append((s[f] - self._dropped_rows(r, seen[f], has_parents) * q_obs[f] * lgamma(b[f])
                        + empty * r * lgamma(b[f])) - empty * lgamma(a) + q_obs[f] * lgamma(a) - (q * r) * lgamma(b[f]))
        return out


class LogLikeliHood(StructureScore):
    def _log_likelihoods(self, plan, counts):
        return _download(plan.score(counts, N.SCORE_LL))

    def _score_round(self, plan, counts, shapes):
        return list(self._log_likelihoods(plan, counts))


class BIC(LogLikeliHood):
    def _score_round(self, plan, counts, shapes):
        sample_size = len(self.data)  # NaN rows included (:818)
        ll = self._log_likelihoods(plan, counts)
        return [ll[f] - 0.5 * log(sample_size) * q * (r - 1) for f, (r, q, _) in enumerate(shapes)]


class AIC(LogLikeliHood):
    def _score_round(self, plan, counts, shapes):
        ll = self._log_likelihoods(plan, counts)
        return [ll[f] - q * (r - 1) for f, (r, q, _) in enumerate(shapes)]


class LogLikelihoodGauss(GaussData, StructureScore):
    """The Gaussian log-likelihood of `variable ~ parents` with an intercept (:919-1019): one pgm_lgs_score job
    per family, K = (ones column, parents), target = variable."""
    _kind = "ll"

    def __init__(self, data, **kwargs):
        GaussData.__init__(self, data)  # no state names: the columns are continuous

    def _jobs(self, families):
        from .. import _native as N

        room = N.LGS_MAX_COND - 1
        jobs = []
        for variable, parents in families:
            parents = list(parents)
            v, *P = self.columns([variable] + parents)
            if len(set(P)) != len(P) or v in P:
                raise ValueError(f"a family names a variable twice: {variable}, {parents}")
            if len(P) > room:
                raise cap_error("parents", len(P), room)
            jobs.append(([self.d] + P, [v]))
        return jobs

    @E.serialized
    def local_scores(self, families):
        """The local score of every (variable, parents) family, as a list of floats: one launch per distinct
        number of parents, one download."""
        jobs = self._jobs([(v, list(ps)) for v, ps in families])
        return [float(s) for s in self.run(jobs, lambda batch, G, shift: batch.score(G, shift, self._kind))[0]]


class BICGauss(LogLikelihoodGauss):
    """llf - (df_model + 2) / 2 log n (:1022-1104)."""
    _kind = "bic"


class AICGauss(LogLikelihoodGauss):
    """llf - (df_model + 2) (:1107-1189)."""
    _kind = "aic"
