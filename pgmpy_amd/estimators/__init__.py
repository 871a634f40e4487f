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
pgm_pair_mi / pgm_pair_emi); MarginalEstimator and MirrorDescentEstimator (below).  Not built: IPF
(MaximumLikelihoodEstimator on a JunctionTree), GES, MMHC, the mixed CI
tests (gcm, pillai) and independence_match.

Continuous data: CITests.pearsonr / GaussCITester (partial correlations) and LogLikelihoodGauss, BICGauss,
AICGauss score all the tests of a PC level or all the families of a hill-climb step in one launch from the
moment matrix the fp64 Gram kernel leaves on the device (pgm_lgs_pcorr, pgm_lgs_score); PC takes
`ci_test=pearsonr` or `tester=GaussCITester(...)`, HillClimbSearch an instance of a Gaussian score.  The
string names "pearsonr", "ll-g", "bic-g", "aic-g" stay closed.

Mixed data: LogLikelihoodCondGauss, BICCondGauss, AICCondGauss score all the families of a hill-climb step
over discrete and continuous columns in one grouped-moment launch on the fp64 matrix units and one score
launch (pgm_cg_moments, pgm_cg_score); HillClimbSearch takes an instance.

Markov networks: PseudoLikelihoodEstimator fits the potentials by maximum pseudo-likelihood: one count launch on the
nodes' blanket families, then one launch pair per evaluation of the objective and its gradient on the count tables
(pgm_mnpl_eval) under L-BFGS.

Junction trees: MirrorDescentEstimator (on the MarginalEstimator base) fits the clique potentials so that chosen
marginals match the data, or a batch of measured marginal vectors: every iteration, line-search trial and log-space
calibration of the entropic mirror descent runs in one launch, one workgroup per row of targets (pgm_md_run).

Exact search: ExhaustiveSearch returns the highest-scoring DAG over up to 24 variables.  The families are scored in
batches by any StructureScore; the dynamic programme over the subset lattice (best parents by a max-zeta transform
through LDS tiles, best sinks by popcount layers, a read-back walk) runs on the device (pgm_xs_run).
ExhaustiveSearch.edge_posteriors runs the same lattice in log space for the exact posterior of every edge (pgm_xs_posterior).
"""
from .base import BaseEstimator, MarginalEstimator, ParameterEstimator
from .MLE import MaximumLikelihoodEstimator
from .BayesianEstimator import BayesianEstimator
from .StructureScore import (AIC, BIC, K2, AICCondGauss, AICGauss, BDeu, BDs, BICCondGauss, BICGauss, LogLikeliHood,
                             LogLikelihoodCondGauss, LogLikelihoodGauss, StructureScore, get_scoring_method)
from .HillClimbSearch import ExpertKnowledge, HillClimbSearch
from . import CITests
from .CITests import CITester, GaussCITester
from .PC import PC
from .EM import ExpectationMaximization
from .TreeSearch import TreeSearch
from .PseudoLikelihood import PseudoLikelihoodEstimator
from .ExhaustiveSearch import ExhaustiveSearch
from .MirrorDescentEstimator import MirrorDescentEstimator

__all__ = ["BaseEstimator", "ParameterEstimator", "MaximumLikelihoodEstimator", "BayesianEstimator",
           "MarginalEstimator", "MirrorDescentEstimator",
           "StructureScore", "K2", "BDeu", "BDs", "LogLikeliHood", "BIC", "AIC", "get_scoring_method",
           "LogLikelihoodGauss", "BICGauss", "AICGauss", "LogLikelihoodCondGauss", "BICCondGauss", "AICCondGauss",
           "HillClimbSearch", "ExpertKnowledge", "CITests", "CITester",
           "GaussCITester", "PC", "ExpectationMaximization", "TreeSearch", "PseudoLikelihoodEstimator",
           "ExhaustiveSearch"]
