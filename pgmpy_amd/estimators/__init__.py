"""Estimators (mirror of pgmpy/estimators).  Parameter learning: the counting and the normalisation run
in two fused HIP launches per model (pgm_fit_count, pgm_fit_finish).  Structure learning: the discrete
structure scores and HillClimbSearch score all the candidate families of a step in one count launch and
one score launch (pgm_fit_score); the conditional-independence tests and PC test all the candidate
separating sets of a level in one count launch and one CI launch per round (pgm_fit_citest).  Latent
variables: ExpectationMaximization runs one E-step launch (pgm_fit_estep: every row's posterior over the
latent configurations added straight into fp64 family tables) and one finishing launch per iteration.

Built: BaseEstimator, ParameterEstimator, MaximumLikelihoodEstimator, BayesianEstimator; StructureScore,
K2, BDeu, BDs, LogLikeliHood, BIC, AIC, get_scoring_method; HillClimbSearch, ExpertKnowledge (required and
forbidden edges); CITests (chi_square, g_sq, log_likelihood, modified_log_likelihood, power_divergence,
get_callable_ci_test, CITester) and PC (orig / stable / parallel; a PDAG from pgmpy_amd.base);
ExpectationMaximization (every row complete in its observed columns); TreeSearch (Chow-Liu and TAN: the
tables of every pair of columns from one int8 MFMA launch, pgm_pair_count, and the pair statistics from
pgm_pair_mi / pgm_pair_emi).  Not built: MarginalEstimator / IPF
(MaximumLikelihoodEstimator on a JunctionTree), GES, MMHC, ExhaustiveSearch, the conditional-Gaussian scores, the mixed CI
tests (gcm, pillai) and independence_match.

Continuous data: CITests.pearsonr / GaussCITester (partial correlations) and LogLikelihoodGauss, BICGauss,
AICGauss score all the tests of a PC level or all the families of a hill-climb step in one launch from the
moment matrix the fp64 Gram kernel leaves on the device (pgm_lgs_pcorr, pgm_lgs_score); PC takes
`ci_test=pearsonr` or `tester=GaussCITester(...)`, HillClimbSearch an instance of a Gaussian score.  The
string names "pearsonr", "ll-g", "bic-g", "aic-g" stay closed.
"""
from .base import BaseEstimator, ParameterEstimator
from .MLE import MaximumLikelihoodEstimator
from .BayesianEstimator import BayesianEstimator
from .StructureScore import (AIC, BIC, K2, AICGauss, BDeu, BDs, BICGauss, LogLikeliHood, LogLikelihoodGauss, StructureScore,
                             get_scoring_method)
from .HillClimbSearch import ExpertKnowledge, HillClimbSearch
from . import CITests
from .CITests import CITester, GaussCITester
from .PC import PC
from .EM import ExpectationMaximization
from .TreeSearch import TreeSearch

__all__ = ["BaseEstimator", "ParameterEstimator", "MaximumLikelihoodEstimator", "BayesianEstimator",
           "StructureScore", "K2", "BDeu", "BDs", "LogLikeliHood", "BIC", "AIC", "get_scoring_method",
           "LogLikelihoodGauss", "BICGauss", "AICGauss", "HillClimbSearch", "ExpertKnowledge", "CITests", "CITester",
           "GaussCITester", "PC", "ExpectationMaximization", "TreeSearch"]
