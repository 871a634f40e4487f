"""LoopyBeliefPropagation: approximate marginals and a partition-function estimate on networks whose treewidth defeats
the junction tree (grids, Ising and Potts models), by sum-product belief propagation with the flooding schedule.

The reference has no loopy BP.  A whole run is one launch of csrc/pgmlbp.hip k_lbp: every iteration, the convergence
test, the node and factor beliefs and the Bethe estimate of log Z, for one instance (``query``) or, through
``query_batch``, for a batch that shares the factor tables and differs in its node terms.  Factor values are
multiplicative potentials, finite and >= 0 (zeros are hard constraints).  The result is exact on a forest and an
approximation on a graph with loops, where the iteration need not converge: ``n_iter_used`` and ``residual`` tell.
There is no CPU path: without a device a compute call raises ``NativeUnavailable``.
"""
import numpy as np

from .. import engine as E
from ..factors.discrete import DiscreteFactor
from ._lbp import LbpPlan
from .base import Inference


class LbpBatch:
    """What ``query_batch`` returns, all device tensors: ``marginals`` [B, n_unary] in the order of
    ``LoopyBeliefPropagation.nodes`` (node v at ``node_offsets[v]``), ``values`` [B, 2] (``log_partition``: the Bethe
    estimate of log Z, ``residual``: the last iteration's), ``n_iter`` [B] int32 (-1: a contradiction, the row is NaN),
    ``factor_beliefs`` [B, n_theta] (factor f at ``factor_offsets[f]``) or None, and ``state`` [B, state_len] (the
    messages) or None that a later call resumes from."""

    def __init__(self, marginals, values, iters, factor_beliefs, state):
        self.marginals, self.values, self.n_iter = marginals, values, iters
        self.factor_beliefs, self.state = factor_beliefs, state
        self.log_partition, self.residual = values[:, 0], values[:, 1]


class LoopyBeliefPropagation(Inference):
    def __init__(self, model):
        from ..models import DiscreteBayesianNetwork, DiscreteMarkovNetwork, FactorGraph

        if not isinstance(model, (DiscreteMarkovNetwork, FactorGraph, DiscreteBayesianNetwork)):
            raise TypeError("Only DiscreteMarkovNetwork, FactorGraph and DiscreteBayesianNetwork are supported")
        super().__init__(model)
        if isinstance(model, DiscreteBayesianNetwork):
            for cpd in model.get_cpds():
                if len(cpd.scope()) > 3:
                    raise ValueError(f"the family of {cpd.variable} ({list(cpd.scope())}) has {len(cpd.scope())} "
                                     f"variables: LoopyBeliefPropagation takes factors of at most 3")
            self.factors = [cpd.to_factor() for cpd in model.get_cpds()]
        else:
            self.factors = list(model.get_factors())
        in_scope = {v for factor in self.factors for v in factor.scope()}
        self.nodes = [v for v in model.nodes() if not isinstance(v, DiscreteFactor) and
                      (v in in_scope or not isinstance(model, FactorGraph))]  # a factor graph's factor nodes are no variables
        self._index = {v: i for i, v in enumerate(self.nodes)}
        card, self._to_no, self._names = {}, {}, {}
        for factor in self.factors:
            for v, k in zip(factor.scope(), factor.cardinality):
                if v not in card:
                    card[v], self._to_no[v] = int(k), factor.name_to_no[v]
                    self._names[v] = [factor.no_to_name[v][i] for i in range(int(k))]
        missing = [v for v in self.nodes if v not in card]
        if missing:
            raise ValueError(f"no factor over {missing}: every node needs one")
        self.card = [card[v] for v in self.nodes]
        theta = []
        for factor in self.factors:
            values = np.asarray(factor._values_readonly(), dtype=np.float64).reshape(-1)
            if not (np.isfinite(values).all() and (values >= 0).all()):
                raise ValueError(f"the values of the factor over {list(factor.scope())} are not all finite and >= 0")
            theta.append(values)
        self._theta = np.concatenate(theta) if theta else np.zeros(0)
        self.scopes = [tuple(self._index[v] for v in f.scope()) for f in self.factors]
        self.plan = LbpPlan(self.card, self.scopes, self._theta)
        self.node_offsets, self.factor_offsets = self.plan.node_offsets, self.plan.factor_offsets
        self.n_unary, self.state_len = self.plan.n_unary, self.plan.state_len
        self._theta_dev = None
        self._last = None  # (factor beliefs, log Z) of the last query, on the host
        self.n_iter_used = self.residual = None

    @E.serialized
    def query_batch(self, unaries, n_iter=100, tol=1e-8, damping=0.0, state=None, return_state=False,
                    return_factor_beliefs=False):
        """Loopy BP on every row of `unaries`, a device fp64 tensor [B, n_unary] of node terms in the order of
        ``nodes`` (ones: no term), with the model's factors, in one launch.  A row stops by itself after the first
        iteration whose residual (the largest change of a message cell) is below `tol`; ``tol=0`` runs `n_iter`
        iterations.  `damping` in [0, 1) mixes the old message into the new one.  `state` resumes from the
        ``state`` of an earlier call.  Returns an ``LbpBatch``."""
        if self._theta_dev is None:
            self._theta_dev = E.to_device(self._theta)
        return LbpBatch(*self.plan.run(unaries, self._theta_dev, n_iter, tol, damping, state=state,
                                       want_beliefs=return_factor_beliefs, want_state=return_state))

    def _state_no(self, var, state):
        try:
            return self._to_no[var][state]
        except KeyError:
            raise ValueError(f"{state!r} is not a state of {var!r}") from None

    @E.serialized_instance
    def query(self, variables, evidence=None, virtual_evidence=None, n_iter=100, tol=1e-8, damping=0.0):
        """{variable: DiscreteFactor} of the normalised single-variable beliefs given the evidence ({variable: state
        name}, an indicator node term) and the virtual evidence (single-variable factors or CPDs that multiply the
        node term).  Raises ValueError when the evidence contradicts the model."""
        from .batch import download

        evidence = {} if evidence is None else evidence
        unknown = [v for v in list(variables) + list(evidence) if v not in self._index]
        if unknown:
            raise ValueError(f"not in the model: {unknown}")
        common = set(evidence).intersection(variables)
        if common:
            raise ValueError(f"Can't have the same variables in both `variables` and `evidence`. Found in both: {common}")
        row = np.ones(self.n_unary)
        for var, state in evidence.items():
            at, k = self.node_offsets[self._index[var]], self.card[self._index[var]]
            row[at:at + k] = np.eye(k)[self._state_no(var, state)]
        if virtual_evidence is not None:
            self._check_virtual_evidence(virtual_evidence)
            for cpd in virtual_evidence:
                at = self.node_offsets[self._index[cpd.variables[0]]]
                values = np.asarray(cpd.values, dtype=np.float64).reshape(-1)
                row[at:at + values.size] *= values
        got = self.query_batch(E.to_device(row[None, :]), n_iter, tol, damping, return_factor_beliefs=True)
        self.n_iter_used = int(download(got.n_iter)[0])
        if self.n_iter_used < 0:
            self._last = None
            raise ValueError("the evidence contradicts the model: a message or a belief sums to 0")
        marginals, values = download(got.marginals)[0], download(got.values)[0]
        self._last, self.residual = (download(got.factor_beliefs)[0], float(values[0])), float(values[1])
        out = {}
        for var in variables:
            at, k = self.node_offsets[self._index[var]], self.card[self._index[var]]
            out[var] = DiscreteFactor([var], [k], marginals[at:at + k], state_names={var: self._names[var]})
        return out

    def factor_beliefs(self):
        """{scope tuple: DiscreteFactor} of the normalised beliefs of the factor scopes after the last query (of two
        factors with one scope, the later one's)."""
        if self._last is None:
            raise ValueError("factor_beliefs() needs a query first")
        out = {}
        for f, factor in enumerate(self.factors):
            scope = list(factor.scope())
            values = self._last[0][self.factor_offsets[f]:self.factor_offsets[f + 1]]
            out[tuple(scope)] = DiscreteFactor(scope, list(factor.cardinality), values,
                                               state_names={v: self._names[v] for v in scope})
        return out

    def log_partition(self):
        """The Bethe estimate of log Z of the last query: of log P~(evidence) when there was evidence; exact on a
        forest."""
        if self._last is None:
            raise ValueError("log_partition() needs a query first")
        return self._last[1]
