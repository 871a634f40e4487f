"""MaximumLikelihoodEstimator (mirror of pgmpy/estimators/MLE.py:21-212).

estimate_cpd counts one family and get_parameters every family of the model with one count launch and
one finishing launch (pgm_fit_count, pgm_fit_finish in PGM_FIT_MLE mode: a parent configuration that
never occurred becomes a uniform column, MLE.py:187).  The CPDs are views of one device buffer.
"""
from .. import engine as E
from .base import ParameterEstimator


class MaximumLikelihoodEstimator(ParameterEstimator):
    def __init__(self, model, data, **kwargs):
        from ..models import DiscreteBayesianNetwork, JunctionTree

        if not isinstance(model, (DiscreteBayesianNetwork, JunctionTree)):
            raise NotImplementedError(
                "Maximum Likelihood Estimate is only implemented for DiscreteBayesianNetwork, JunctionTree, and DAG"
            )
        if isinstance(model, DiscreteBayesianNetwork):
            if len(model.latents) > 0:
                raise ValueError(
                    f"Found latent variables: {model.latents}. "
                    "Maximum Likelihood doesn't support latent variables, please use ExpectationMaximization."
                )
            elif set(model.nodes()) > set(data.columns):
                raise ValueError(
                    f"Nodes detected in the model that are not present "
                    f"in the dataset: {set(model.nodes) - set(data.columns)}. "
                    "Refine the model so that all parameters can be estimated from the data."
                )
        super(MaximumLikelihoodEstimator, self).__init__(model, data, **kwargs)

    @E.serialized
    def get_parameters(self, n_jobs=1, weighted=False):
        """The CPDs of every node of the model, in model.nodes() order (MLE.py:86-135).  n_jobs is
        accepted and ignored: the whole model is two launches."""
        from ..models import JunctionTree

        if isinstance(self.model, JunctionTree):
            return self.estimate_potentials()
        return self._estimate(list(self.model.nodes()), weighted)

    @E.serialized
    def estimate_cpd(self, node, weighted=False):
        """The CPD of one node (MLE.py:137-212)."""
        return self._estimate([node], weighted)[0]

    def _estimate(self, nodes, weighted):
        families = self._families(nodes)
        plan, counts = self._count_families(families, weighted)
        return self._cpds(plan, families, plan.finish(counts, bayes=False))

    def estimate_potentials(self):
        raise NotImplementedError("Iterative Proportional Fitting on a JunctionTree (estimate_potentials) is not built")
