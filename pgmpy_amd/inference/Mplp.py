"""Mplp (mirror of pgmpy/inference/mplp.py): MAP on a DiscreteMarkovNetwork by max-product linear programming
with triplet tightening.

The factor values are the additive terms theta, as in the reference (``log=True`` takes their logarithm first,
for a network of multiplicative potentials).  A whole ``_run_mplp`` is one launch of csrc/pgmmplp.hip k_mplp:
every iteration, the decode, the primal and dual values and the convergence test, for one instance or, through
``map_query_batch``, for a batch that shares the cluster terms and differs in its node terms.  Tightening stays on
the host: the state is downloaded, the triangles are scored as ``_get_triplet_scores`` does, the plan is rebuilt
with the chosen triplets appended and the carried state is relaunched.

Deviations from the reference: a node without a unary factor gets zeros (the reference raises KeyError); the best
primal value starts at -inf, not 0 (the reference returns {} when every assignment scores below 0); the model's
factors are not modified (the reference's first update adds into them in place, and appends the triplets); the
order of a cluster's intersection sets is fixed (the reference iterates a set); a triangle with an edge that has no
pairwise factor is not a candidate for tightening (the reference raises KeyError).
There is no CPU path: without a device a compute call raises ``NativeUnavailable``.
"""
import itertools

import networkx as nx
import numpy as np

from .. import engine as E
from ._mplp import MplpPlan
from .base import Inference


class MplpBatch:
    """What ``map_query_batch`` returns, all device tensors: ``codes`` [B, n_nodes] uint8 in the order of
    ``Mplp.nodes``, ``primal`` (the best primal value), ``dual_lp``, ``dual_gap``, ``integrality_gap`` [B] fp64,
    ``n_iter`` [B] int32, and ``state`` [B, state_len] (or None) that a later call resumes from."""

    def __init__(self, codes, values, iters, state):
        self.codes, self.values, self.n_iter, self.state = codes, values, iters, state
        self.primal, self.dual_lp, self.dual_gap, self.integrality_gap = (values[:, i] for i in range(4))


class Mplp(Inference):
    def __init__(self, model, log=False):
        from ..models import DiscreteMarkovNetwork

        if not isinstance(model, DiscreteMarkovNetwork):
            raise TypeError("Only DiscreteMarkovNetwork is supported")
        super().__init__(model)
        self.nodes = list(model.nodes())
        self._index = {v: i for i, v in enumerate(self.nodes)}
        card = model.get_cardinality()
        self.card = [int(card[v]) for v in self.nodes]
        unary = [np.zeros(k) for k in self.card]
        self._clusters, theta, seen = [], [], set()
        for factor in model.get_factors():
            scope = frozenset(factor.scope())
            if scope in seen:
                raise ValueError(f"two factors over {sorted(map(str, scope))}: Mplp takes one factor per scope")
            seen.add(scope)
            values = np.asarray(factor._values_readonly(), dtype=np.float64).reshape(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                values = np.log(values) if log else values
            if not np.isfinite(values).all():
                raise ValueError(f"the terms of the factor over {list(factor.scope())} are not all finite")
            if len(scope) == 1:
                unary[self._index[factor.scope()[0]]] = values
            else:
                self._clusters.append(tuple(self._index[v] for v in factor.scope()))
                theta.append(values)
        self._unary = np.concatenate(unary)
        self._theta = np.concatenate(theta) if theta else np.zeros(0)
        self._plans = {}
        self._triplets = ()            # the tightening triplets of map_query so far, as node indices
        self._state = None             # the carried state of map_query (host, [state_len])
        self.plan = self._plan_for(())
        self.node_offsets, self.n_unary = self.plan.node_offsets, self.plan.n_unary
        self.dual_threshold = self.integrality_gap_threshold = 0.0002
        self.best_int_objective, self.best_assignment = -np.inf, {}
        self.dual_lp = self.dual_gap = self.integrality_gap = None

    # ------------------------------------------------------------------ plans
    def _plan_for(self, triplets):
        """(plan, theta on the host) for the model's clusters and these triplets (node indices) appended."""
        if triplets not in self._plans:
            plan = MplpPlan(self.card, list(self._clusters) + list(triplets), len(triplets))
            self._plans[triplets] = (plan, np.concatenate([self._theta, np.zeros(plan.n_theta - self._theta.size)]))
        return self._plans[triplets][0]

    def _theta_dev(self, triplets):
        plan, theta = self._plans[triplets]
        return E.to_device(theta)

    def unaries(self):
        """The model's own node terms as a device row [1, n_unary], in plan node order."""
        return E.to_device(self._unary[None, :])

    def find_triangles(self):
        """All triangles of the model (mplp.py:346-376)."""
        return list(filter(lambda x: len(x) == 3, nx.find_cliques(self.model)))

    # ------------------------------------------------------------------ the batch
    @E.serialized
    def map_query_batch(self, unaries, n_iter=1000, dual_threshold=0.0002, integrality_gap_threshold=0.0002,
                        triplets=None, state=None, return_state=False):
        """MPLP on every row of `unaries`, a device fp64 tensor [B, n_unary] of node terms in the order of
        ``nodes`` (node v at ``node_offsets[v]``), with the model's cluster terms, in one launch.  `triplets`
        (triples of node names) are tightening clusters that apply to every instance; `state` resumes from the
        ``state`` of an earlier call with the same triplets.  Returns an ``MplpBatch``."""
        key = tuple(tuple(self._index[v] for v in t) for t in (triplets or ()))
        plan = self._plan_for(key)
        out = plan.run(unaries, self._theta_dev(key), n_iter, dual_threshold, integrality_gap_threshold, state=state,
                       want_state=return_state)
        return MplpBatch(*out)

    # ------------------------------------------------------------------ the reference's interface
    def _run_mplp(self, n_iter):
        from .batch import download

        plan = self._plan_for(self._triplets)
        state = None if self._state is None else E.to_device(self._state[None, :])
        codes, values, _, out = plan.run(self.unaries(), self._theta_dev(self._triplets), n_iter, self.dual_threshold,
                                         self.integrality_gap_threshold, state=state, want_state=True)
        self._state = download(out)[0]
        self.best_int_objective, self.dual_lp, dual_gap, gap = (float(x) for x in download(values)[0])
        if n_iter > 0:
            self.dual_gap, self.integrality_gap = dual_gap, gap
        self.best_assignment = {v: int(c) for v, c in zip(self.nodes, download(codes)[0])}

    def _objective(self, c):
        """Cluster c's objective in the carried state, shaped by its variables."""
        plan = self._plan_for(self._triplets)
        at = plan.n_unary + plan.cluster_offsets[c]
        shape = [self.card[v] for v in plan.clusters[c]]
        return self._state[at:at + int(np.prod(shape))].reshape(shape)

    def _is_converged(self):
        """mplp.py:302-344 with the integrality gap alone, on the carried state."""
        plan = self._plan_for(self._triplets)
        offs = plan.node_offsets
        new_dual = sum(self._state[offs[v]:offs[v + 1]].max() for v in range(len(self.nodes)))
        new_dual += sum(self._objective(c).max() for c in range(len(plan.clusters)))
        self.dual_gap = abs(self.dual_lp - new_dual)
        self.integrality_gap = abs(self.dual_lp - self.best_int_objective)
        if self.integrality_gap_threshold and self.integrality_gap < self.integrality_gap_threshold:
            return True
        self.dual_lp = self._state[plan.n_unary + plan.n_theta + plan.n_msg + 1] = new_dual
        return False

    def _get_triplet_scores(self, triangles):
        """{triangle: independent maxima of its edges' objectives less their joint maximum} (mplp.py:409-445)."""
        edge = {frozenset(c): i for i, c in enumerate(self._clusters) if len(c) == 2}
        scores = {}
        for tri in triangles:
            t = tuple(self._index[v] for v in tri)
            pairs = list(itertools.combinations(range(3), 2))
            if t in self._triplets or any(frozenset((t[a], t[b])) not in edge for a, b in pairs):
                continue
            ind_max, joint = 0.0, np.zeros([self.card[v] for v in t])
            for a, b in pairs:
                c = edge[frozenset((t[a], t[b]))]
                obj = self._objective(c) if self._clusters[c][0] == t[a] else self._objective(c).T
                ind_max += obj.max()
                joint = joint + obj.reshape([self.card[t[p]] if p in (a, b) else 1 for p in range(3)])
            scores[t] = ind_max - joint.max()
        return scores

    def _update_triangles(self, triplets):
        """Append the triplets with zero terms and zero messages; the carried state moves to the new layout."""
        old = self._plan_for(self._triplets)
        self._triplets = self._triplets + tuple(triplets)
        new = self._plan_for(self._triplets)
        tables, msgs = old.n_unary + old.n_theta, old.n_msg
        self._state = np.concatenate([self._state[:tables], np.zeros(new.n_theta - old.n_theta),
                                      self._state[tables:tables + msgs], np.zeros(new.n_msg - msgs),
                                      self._state[tables + msgs:]])

    def _tighten_triplet(self, max_iterations, later_iter, max_triplets, prolong):
        scores = self._get_triplet_scores(self.find_triangles())
        order = sorted(scores, key=scores.get)
        for _ in range(max_iterations):
            if self._is_converged():
                break
            add = [order.pop() for _ in range(min(max_triplets, len(order)))]
            if not add and prolong is False:
                break
            self._update_triangles(add)
            self._run_mplp(later_iter)

    def get_integrality_gap(self):
        return self.integrality_gap

    def query(self):
        raise NotImplementedError("map_query() is the only query method available.")

    @E.serialized_instance
    def map_query(self, init_iter=1000, later_iter=20, dual_threshold=0.0002, integrality_gap_threshold=0.0002,
                  tighten_triplet=True, max_triplets=5, max_iterations=100, prolong=False):
        """{node: state index} of the best assignment found (mplp.py:554-674).  A second call goes on from the
        state the first one left, as in the reference."""
        self.dual_threshold, self.integrality_gap_threshold = dual_threshold, integrality_gap_threshold
        self._run_mplp(init_iter)
        if tighten_triplet:
            self._tighten_triplet(max_iterations, later_iter, max_triplets, prolong)
        return dict(self.best_assignment)
