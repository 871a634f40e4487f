"""BayesianEstimator (mirror of pgmpy/estimators/BayesianEstimator.py:18-264).

The pseudo-counts of every node (BDeu, K2 or dirichlet) are built on the host into one buffer with the
count tables' layout and uploaded once; pgm_fit_finish adds them to the counts and normalises
(PGM_FIT_BAYES: no uniform fill, 0/0 stays NaN as in the reference's normalize).
"""
import logging
import numbers

import numpy as np

from .. import engine as E
from .base import ParameterEstimator

logger = logging.getLogger("pgmpy")


class BayesianEstimator(ParameterEstimator):
    def __init__(self, model, data, **kwargs):
        from ..models import DiscreteBayesianNetwork

        if not isinstance(model, DiscreteBayesianNetwork):
            raise NotImplementedError(
                "Bayesian Parameter Estimation is only implemented for DAG or DiscreteBayesianNetwork"
            )
        if len(model.latents) != 0:
            raise ValueError(
                f"Bayesian Parameter Estimation works only "
                f"on models with all observed variables. Found latent variables: {model.latents}"
            )
        super(BayesianEstimator, self).__init__(model, data, **kwargs)

    def _pseudo_counts(self, node, prior_type, pseudo_counts, equivalent_sample_size):
        """The [node_card, prod(parent_card)] pseudo-counts of one node (BayesianEstimator.py:212-250):
        a host array, or a device tensor passed through (fit_update builds them on the device)."""
        node_cardinality = len(self.state_names[node])
        parents = sorted(self.model.get_parents(node))
        parents_cardinalities = [len(self.state_names[parent]) for parent in parents]
        cpd_shape = (node_cardinality, int(np.prod(parents_cardinalities, dtype=int)))
        prior_type = prior_type.lower()
        on_device = hasattr(pseudo_counts, "data_ptr")
        if (pseudo_counts is not None and (on_device or np.array(pseudo_counts).size > 0)
                and (prior_type != "dirichlet")):
            logger.warning(
                f"pseudo count specified with {prior_type} prior. It will be ignored, "
                "use dirichlet prior for specifying pseudo_counts"
            )
        if prior_type == "k2":
            return np.ones(cpd_shape, dtype=int)
        if prior_type == "bdeu":
            alpha = float(equivalent_sample_size) / (node_cardinality * np.prod(parents_cardinalities))
            return np.ones(cpd_shape, dtype=float) * alpha
        if prior_type == "dirichlet":
            if isinstance(pseudo_counts, numbers.Real):
                return np.ones(cpd_shape, dtype=int) * pseudo_counts
            if not on_device:
                pseudo_counts = np.array(pseudo_counts)
            if tuple(pseudo_counts.shape) != cpd_shape:
                raise ValueError(f"The shape of pseudo_counts for the node: {node} must be of shape: {str(cpd_shape)}")
            return pseudo_counts
        raise ValueError("'prior_type' not specified")

    @E.serialized
    def get_parameters(self, prior_type="BDeu", equivalent_sample_size=5, pseudo_counts=None, n_jobs=1,
                       weighted=False):
        """The CPDs of every node, in model.nodes() order (BayesianEstimator.py:50-145).
        equivalent_sample_size: a number or a dict per node; pseudo_counts: a number or a dict of
        per-node arrays.  n_jobs is accepted and ignored."""
        nodes = list(self.model.nodes())
        priors = []
        for node in nodes:
            ess = equivalent_sample_size[node] if isinstance(equivalent_sample_size, dict) else equivalent_sample_size
            if isinstance(pseudo_counts, numbers.Real):
                pc = pseudo_counts
            else:
                pc = pseudo_counts[node] if pseudo_counts else None
            priors.append(self._pseudo_counts(node, prior_type, pc, ess))
        return self._estimate(nodes, priors, weighted)

    @E.serialized
    def estimate_cpd(self, node, prior_type="BDeu", pseudo_counts=[], equivalent_sample_size=5, weighted=False):
        """The CPD of one node (BayesianEstimator.py:147-264)."""
        prior = self._pseudo_counts(node, prior_type, pseudo_counts, equivalent_sample_size)
        return self._estimate([node], [prior], weighted)[0]

    def _estimate(self, nodes, priors, weighted):
        import torch

        self._check_weighted(weighted)  # every check before any compute
        families = self._families(nodes)
        plan, counts = self._count_families(families, weighted)
        if any(hasattr(p, "data_ptr") for p in priors):
            pseudo = torch.empty(plan.total_bins, dtype=torch.float64, device=counts.device)
            for f, p in enumerate(priors):
                dst = pseudo[plan.offsets[f]:plan.offsets[f] + plan.sizes[f]]
                dst.copy_(p.reshape(-1) if hasattr(p, "data_ptr") else torch.from_numpy(
                    np.ascontiguousarray(p, dtype=np.float64).reshape(-1)))
        else:  # one host buffer, one upload
            host = np.empty(plan.total_bins, dtype=np.float64)
            for f, p in enumerate(priors):
                host[plan.offsets[f]:plan.offsets[f] + plan.sizes[f]] = np.asarray(p, dtype=np.float64).reshape(-1)
            pseudo = E.to_device_raw(host)
        return self._cpds(plan, families, plan.finish(counts, pseudo=pseudo, bayes=True))
