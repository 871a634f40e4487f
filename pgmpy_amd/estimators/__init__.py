"""Estimators (mirror of pgmpy/estimators).  Parameter learning: the counting and the normalisation run
in two fused HIP launches per model (pgm_fit_count, pgm_fit_finish).  Structure learning: the discrete
structure scores and HillClimbSearch score all the candidate families of a step in one count launch and
one score launch (pgm_fit_score).

Built: BaseEstimator, ParameterEstimator, MaximumLikelihoodEstimator, BayesianEstimator; StructureScore,
K2, BDeu, BDs, LogLikeliHood, BIC, AIC, get_scoring_method; HillClimbSearch, ExpertKnowledge (required and
forbidden edges).  Not built: ExpectationMaximization, MarginalEstimator / IPF
(MaximumLikelihoodEstimator on a JunctionTree), PC, GES, MMHC, TreeSearch, ExhaustiveSearch, the Gaussian
and conditional-Gaussian scores.
"""
from .base import BaseEstimator, ParameterEstimator
from .MLE import MaximumLikelihoodEstimator
from .BayesianEstimator import BayesianEstimator
from .StructureScore import AIC, BIC, K2, BDeu, BDs, LogLikeliHood, StructureScore, get_scoring_method
from .HillClimbSearch import ExpertKnowledge, HillClimbSearch

__all__ = ["BaseEstimator", "ParameterEstimator", "MaximumLikelihoodEstimator", "BayesianEstimator",
           "StructureScore", "K2", "BDeu", "BDs", "LogLikeliHood", "BIC", "AIC", "get_scoring_method",
           "HillClimbSearch", "ExpertKnowledge"]
