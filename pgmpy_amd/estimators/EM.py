"""ExpectationMaximization (mirror of pgmpy/estimators/EM.py:22-410).

The reference expands the unique rows by every latent configuration into a pandas frame, weights each
expanded row with one cpd.get_value per CPD under DataFrame.apply, and runs a weighted groupby per node.
Here one iteration is two launches on the resident uint8 codes: the E-step kernel (pgm_fit_estep) adds every
row's posterior over the joint latent configuration straight into fp64 family tables, and pgm_fit_finish
| PGM_FIT_WEIGHTED turns them into the next CPD values.  The posterior needs only the families with a latent
in scope: the factor of a latent-free family is the same for every configuration and cancels.  The values
stay on the device between iterations, the convergence test runs there and one scalar comes back per
iteration; the CPD objects are built once at the end.

Extensions: `n_iter_` (iterations run) and `log_likelihoods_` (per iteration, the log-likelihood of the data
under the parameters the iteration started from, with the reference's floor of 1e-10 per CPD entry).

Deviations: this project has no DAG class, its DAGs are CPD-less DiscreteBayesianNetworks; at
most 8 latent variables with at most 4,096 joint configurations and 32 families with a latent in scope;
with apply_smoothing the CPDs estimated once get the prior of **kwargs (the reference gives them
BayesianEstimator's default, BDeu with equivalent_sample_size 5); n_jobs, batch_size and show_progress are
accepted and ignored.
"""
import logging
import numbers
from itertools import chain

import numpy as np

from .. import engine as E
from ._fit import FitPlan
from .base import ParameterEstimator

logger = logging.getLogger("pgmpy")

RTOL = 1e-5  # np.allclose's default, which TabularCPD.__eq__(atol=) leaves as it is (EM.py:182-194)


class ExpectationMaximization(ParameterEstimator):
    def __init__(self, model, data, **kwargs):
        from ..models import DiscreteBayesianNetwork

        if not isinstance(model, DiscreteBayesianNetwork):
            raise NotImplementedError(
                "Expectation Maximization is only implemented for DAG or DiscreteBayesianNetwork"
            )
        # fully missing columns are latents (EM.py:80-91)
        original_cols = set(data.columns)
        data = data.dropna(axis=1, how="all")
        dropped_cols = original_cols - set(data.columns)
        new_latents = [col for col in dropped_cols if col not in model.latents]
        if new_latents:
            logger.warning(
                f"Columns {new_latents} have all missing values and are not marked as latent. "
                "Treating them as latent variables."
            )
            model.latents.update(new_latents)
        # rows with any missing value are dropped (EM.py:93-102)
        original_rows_count = data.shape[0]
        data = data.dropna()
        dropped_rows_count = original_rows_count - data.shape[0]
        if dropped_rows_count:
            logger.warning(
                f"{dropped_rows_count} rows with missing values in partially "
                "missing columns were dropped from the dataset."
            )
        super(ExpectationMaximization, self).__init__(model, data, **kwargs)
        self.model_copy = self.model.copy()
        self.n_iter_ = 0
        self.log_likelihoods_ = []

    # ------------------------------------------------------------------ host side: every check, no compute
    def _initial_values(self, cpd, node, parents, n_states):
        """The values of an initial CPD as [node, parents...] in the plan's order (parents sorted) and
        this estimator's state order, flat."""
        from ..factors.discrete import TabularCPD

        if not isinstance(cpd, TabularCPD):
            raise ValueError(f"init_cpds[{node!r}] must be a TabularCPD. Got {type(cpd)}")
        scope = [node] + parents
        if cpd.variable != node or set(cpd.variables[1:]) != set(parents) or len(cpd.variables) != len(scope):
            raise ValueError(f"init_cpds[{node!r}] must be the CPD of {node} given its parents {parents}. "
                             f"Got the scope {list(cpd.variables)}")
        card = dict(zip(cpd.variables, (int(c) for c in cpd.cardinality)))
        for v in scope:
            if card[v] != n_states[v]:
                raise ValueError(f"init_cpds[{node!r}]: {v} has {card[v]} states, the estimator has {n_states[v]}")
        values = np.asarray(cpd._values_readonly(), dtype=np.float64).reshape([card[v] for v in cpd.variables])
        values = values.transpose([list(cpd.variables).index(v) for v in scope])
        for axis, v in enumerate(scope):
            theirs, mine = list(cpd.state_names[v]), list(self.state_names[v])
            if theirs != mine:
                if set(theirs) != set(mine):
                    raise ValueError(f"init_cpds[{node!r}]: the states of {v} are {theirs}, the estimator has {mine}")
                values = np.take(values, [theirs.index(s) for s in mine], axis=axis)
        return np.ascontiguousarray(values).reshape(-1)

    def _prior(self, nodes, kwargs):
        """Per node the pseudo-counts of BayesianEstimator.estimate_cpd(node, **kwargs)."""
        from .BayesianEstimator import BayesianEstimator

        unknown = set(kwargs) - {"prior_type", "pseudo_counts", "equivalent_sample_size"}
        if unknown:
            raise TypeError(f"estimate_cpd() got an unexpected keyword argument {sorted(unknown)[0]!r}")
        prior_type = kwargs.get("prior_type", "BDeu")
        if not isinstance(prior_type, str):
            raise ValueError("'prior_type' not specified")
        return [np.asarray(BayesianEstimator._pseudo_counts(self, node, prior_type, kwargs.get("pseudo_counts", []),
                                                            kwargs.get("equivalent_sample_size", 5)), dtype=np.float64)
                for node in nodes]

    def _pseudo_buffer(self, plan, priors):
        host = np.empty(plan.total_bins, dtype=np.float64)
        for f, p in enumerate(priors):
            host[plan.offsets[f]:plan.offsets[f] + plan.sizes[f]] = p.reshape(-1)
        return E.to_device_raw(host)

    @E.serialized
    def get_parameters(self, latent_card=None, apply_smoothing=False, max_iter=100, atol=1e-8, n_jobs=1,
                       batch_size=1000, seed=None, init_cpds={}, show_progress=True, **kwargs):
        """The CPDs of every node by expectation maximisation (EM.py:196-410).

        latent_card: {latent: cardinality}, 2 each by default; the latents' states are range(card).
        init_cpds: {node: TabularCPD} to start from, or "random" / "uniform" for every node.  The nodes
        that are not latent, not a child of a latent and not in init_cpds are estimated once (MLE, or with
        apply_smoothing the Bayesian estimate under the prior of **kwargs: prior_type, pseudo_counts,
        equivalent_sample_size); the others start from init_cpds or TabularCPD.get_random(seed=seed) and are
        re-estimated every iteration until every entry satisfies |old - new| <= atol + 1e-5 |new| or
        max_iter is reached.  n_jobs, batch_size and show_progress are accepted and ignored."""
        import torch

        from ..factors.discrete import TabularCPD
        from ..inference.batch import download

        # Step 1: every check, on the host
        model = self.model
        latents = [v for v in model.nodes() if v in self.model_copy.latents]
        if not isinstance(max_iter, numbers.Integral) or max_iter < 1:
            raise ValueError(f"max_iter must be a positive integer. Got: {max_iter}")
        if not (isinstance(atol, numbers.Real) and atol >= 0):
            raise ValueError(f"atol must be a non-negative number. Got: {atol}")
        if not latents:
            raise ValueError("The model has no latent variable: use MaximumLikelihoodEstimator or BayesianEstimator")
        if latent_card is None:
            latent_card = {var: 2 for var in latents}
        for var in latents:
            if var not in latent_card:
                raise ValueError(f"latent_card has no cardinality for the latent variable {var}")
            if not isinstance(latent_card[var], numbers.Integral) or not 1 <= latent_card[var] < 255:
                raise ValueError(f"latent_card[{var!r}] must be an integer in 1 .. 254. Got: {latent_card[var]}")
        observed = [v for v in model.nodes() if v not in self.model_copy.latents]
        missing = [v for v in observed if v not in self.state_names]
        if missing:
            raise ValueError(f"Nodes {missing} are neither latent nor present in the dataset.")
        if not apply_smoothing and kwargs:
            raise TypeError(f"estimate_cpd() got an unexpected keyword argument {sorted(kwargs)[0]!r}")
        n_states = {key: len(value) for key, value in self.state_names.items()}
        n_states.update({var: int(latent_card[var]) for var in latents})
        for var in latents:
            self.state_names[var] = list(range(n_states[var]))

        if isinstance(init_cpds, str):
            if init_cpds not in ("random", "uniform"):
                raise ValueError(
                    f"If `init_cpds` is a string, it must be either 'random' or 'uniform'. Got: {init_cpds}"
                )
            make = TabularCPD.get_random if init_cpds == "random" else TabularCPD.get_uniform
            init_cpds = {}
            for var in model.nodes():
                scope = [var] + model.get_parents(var)
                init_cpds[var] = make(variable=var, evidence=scope[1:], cardinality={v: n_states[v] for v in scope},
                                      state_names={v: self.state_names[v] for v in scope}, seed=seed)
        elif not isinstance(init_cpds, dict):
            raise ValueError(f"init_cpds must be a dict or one of 'random' / 'uniform'. Got: {type(init_cpds)}")
        for var in init_cpds:
            if var not in model.nodes():
                raise ValueError(f"init_cpds has the variable {var}, which is not in the model")

        latent_children = set(chain(*[model.get_children(var) for var in latents]))
        fixed_nodes = [v for v in model.nodes()
                       if v not in self.model_copy.latents and v not in latent_children and v not in init_cpds]
        em_nodes = [v for v in model.nodes() if v not in fixed_nodes]
        fixed_families, em_families = self._families(fixed_nodes), self._families(em_nodes)

        # the code columns: the data's own, then one virtual column per latent
        data_columns = [v for v in self.variables if v != "_weight"]
        col_of = {v: j for j, v in enumerate(data_columns)}
        latent_cols = []
        for var in latents:
            col_of[var] = len(col_of)
            latent_cols.append(col_of[var])
        plan = FitPlan([self._family(v, ps, col_of) for v, ps in em_families])
        plan.estep_info(latent_cols)  # the limits of pgm_fit_estep, before any compute

        host = np.empty(plan.total_bins, dtype=np.float64)
        for f, (node, parents) in enumerate(em_families):
            cpd = init_cpds.get(node)
            if cpd is None:  # EM.py:359-378
                scope = [node] + list(self.model_copy.predecessors(node))
                cpd = TabularCPD.get_random(variable=node, evidence=scope[1:],
                                            cardinality={v: n_states[v] for v in scope},
                                            state_names={v: self.state_names[v] for v in scope}, seed=seed)
            host[plan.offsets[f]:plan.offsets[f] + plan.sizes[f]] = self._initial_values(cpd, node, parents, n_states)
        em_prior = self._prior(em_nodes, kwargs) if apply_smoothing else None
        fixed_prior = self._prior(fixed_nodes, kwargs) if apply_smoothing else None

        # Step 2: the CPDs that no latent touches, once, and their constant share of the log-likelihood
        codes, _ = self._codes()
        fixed_cpds, ll_const = [], 0.0
        if fixed_families:
            fplan, fcounts = self._count_families(fixed_families)
            fpseudo = self._pseudo_buffer(fplan, fixed_prior) if apply_smoothing else None
            fvalues = fplan.finish(fcounts, pseudo=fpseudo, bayes=apply_smoothing)
            fixed_cpds = self._cpds(fplan, fixed_families, fvalues)
            terms = fcounts.to(torch.float64) * torch.log(torch.clamp(fvalues, min=1e-10))
            ll_const = float(download(torch.where(fcounts > 0, terms, torch.zeros_like(terms)).sum().reshape(1))[0])

        # Step 3: iterate on the device
        values = E.to_device_raw(host)
        new_values = torch.empty_like(values)
        tables = torch.empty_like(values)
        pseudo = self._pseudo_buffer(plan, em_prior) if apply_smoothing else None
        ll = torch.zeros(int(max_iter), dtype=torch.float64, device=values.device)
        self.n_iter_ = 0
        for it in range(int(max_iter)):
            tables.zero_()
            _, loglik = plan.estep(latent_cols, values, codes, tables=tables, want_loglik=True)
            plan.finish(tables, pseudo=pseudo, bayes=bool(apply_smoothing), out=new_values)
            ll[it] = loglik.sum()
            # np.allclose(old, new, atol=atol): a NaN never converges
            close = ((values - new_values).abs() <= atol + RTOL * new_values.abs()).all()
            values, new_values = new_values, values
            self.n_iter_ = it + 1
            if int(download(close.to(torch.uint8).reshape(1))[0]):
                break
        self.log_likelihoods_ = [float(x) + ll_const for x in download(ll)[:self.n_iter_]]
        return fixed_cpds + self._cpds(plan, em_families, values)
