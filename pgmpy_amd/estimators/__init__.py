"""Parameter estimators (mirror of pgmpy/estimators): the counting and the normalisation run in two
fused HIP launches per model (pgm_fit_count, pgm_fit_finish).

Built: BaseEstimator, ParameterEstimator, MaximumLikelihoodEstimator, BayesianEstimator.  Not built:
ExpectationMaximization, MarginalEstimator / IPF (MaximumLikelihoodEstimator on a JunctionTree),
structure learners and scores.
"""
from .base import BaseEstimator, ParameterEstimator
from .MLE import MaximumLikelihoodEstimator
from .BayesianEstimator import BayesianEstimator

__all__ = ["BaseEstimator", "ParameterEstimator", "MaximumLikelihoodEstimator", "BayesianEstimator"]
