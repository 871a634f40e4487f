"""MirrorDescentEstimator (mirror of pgmpy/estimators/MirrorDescentEstimator.py): the clique potentials of a junction
tree fitted so that chosen marginals match the data, by entropic mirror descent (McKenna, Sheldon and Miklau 2019,
Appendix A.1).

The reference rebuilds DiscreteFactor objects and calibrates the tree on the host for every line-search trial, up to
iterations x 25 times.  Here the whole optimisation (every iteration, every trial, every calibration) is ONE launch of
k_md (pgm_md_run, csrc/pgmmd.hip): one workgroup per row of targets, the potentials, beliefs and messages in LDS.
`estimate` fits the data's own marginals (one row); `estimate_batch` fits B measured rows of the same marginals in
one launch (noisy measurements, bootstrap replicates).

Deviation: the calibration runs in log space, as the reference's TODO asks.  The reference calibrates in
probability space on the values of theta (it multiplies and adds log-potentials as if they were probabilities) and
only then reads the result as a log-belief; the two agree on a single clique and differ on every tree with an edge.
"""
import numpy as np

from .. import engine as E
from ..factors import FactorDict
from ..factors.discrete import DiscreteFactor
from ._md import MdPlan
from .base import MarginalEstimator


class MirrorDescentEstimator(MarginalEstimator):
    def _tree(self):
        """(cliques, {clique: its variables in its factor's order}, variables, {variable: index}, edges)."""
        jt = self.belief_propagation.junction_tree
        cliques = list(jt.nodes())
        order = {c: list(jt.get_factors(c).variables) for c in cliques}
        variables = list(dict.fromkeys(v for c in cliques for v in order[c]))
        index = {v: i for i, v in enumerate(variables)}
        at = {c: i for i, c in enumerate(cliques)}
        return cliques, order, variables, index, [(at[a], at[b]) for a, b in jt.edges()]

    def _plan(self, marginals):
        """The MdPlan of the tree and these marginals (kept for the next call with the same marginals)."""
        key = tuple(tuple(m) for m in marginals)
        hit = getattr(self, "_md_plan", None)
        if hit is not None and hit[0] == key:
            return hit[1]
        jt = self.belief_propagation.junction_tree
        cliques, order, variables, index, edges = self._tree()
        self._clique_to_marginal(marginals={m: None for m in key}, clique_nodes=cliques)  # the reference's ValueError
        card = jt.get_cardinality()
        plan = MdPlan([card[v] for v in variables], [[index[v] for v in order[c]] for c in cliques], edges,
                      [[index[v] for v in m] for m in key])
        self._md_plan = (key, plan)
        return plan

    def _start(self, order):
        """The flat start [1, n_cells] on the host: self.theta, or else the tree's factors read as log-potentials."""
        source = self.theta if self.theta else self.belief_propagation.junction_tree.clique_beliefs
        parts = []
        for c, scope in order.items():
            f = source[c]
            parts.append(np.transpose(np.asarray(f.values), [f.variables.index(v) for v in scope]).ravel())
        return np.concatenate(parts)[None, :]

    def _factors(self, plan, order, row):
        """FactorDict of the cliques' tables in a flat device row."""
        jt = self.belief_propagation.junction_tree
        out = FactorDict({})
        for i, (c, scope) in enumerate(order.items()):
            f = jt.get_factors(c)
            out[c] = DiscreteFactor(scope, [int(k) for k in f.cardinality],  # scope is f's own order
                                    row[plan.clique_offsets[i]:plan.clique_offsets[i + 1]],
                                    state_names={v: list(f.state_names[v]) for v in scope})
        return out

    @E.serialized
    def estimate(self, marginals, metric="L2", iterations=100, stepsize=None, show_progress=True):
        """Fit the tree to the data's `marginals` (tuples of column names) and return the junction tree, its factors
        set to the fitted clique marginals mu (counts: they sum to len(data)); `self.theta` keeps the log-potentials,
        from which the next call starts.  `stepsize` None: a line search from alpha = 1 / n^2, doubled at every
        iteration; a float: that fixed step; anything else: a fixed step of 1 / n^2 (the reference's reading).
        `show_progress` is accepted and ignored: there is one launch."""
        if self.data is None:
            raise ValueError(f"No data was found to fit to the marginals {marginals}")
        if metric not in ("L1", "L2"):
            raise ValueError("Metric must be one of L1 or L2.")
        marginals = [tuple(m) for m in marginals]
        plan = self._plan(marginals)
        _, order, _, _, _ = self._tree()
        y = FactorDict.from_dataframe(self.data, marginals, state_names=self.state_names)
        targets = np.concatenate([np.asarray(y[m].values).ravel() for m in marginals])[None, :]
        if targets.shape[1] != plan.n_y:
            raise ValueError("the data's states do not match the model's cardinalities: pass `state_names`")
        theta, mu, _, _ = plan.run(E.to_device(targets), E.to_device(np.array([float(len(self.data))])),
                                   E.to_device(self._start(order)), metric, iterations, stepsize)
        self.theta = self._factors(plan, order, theta[0])
        self.belief_propagation.junction_tree.clique_beliefs = self._factors(plan, order, mu[0])
        return self.belief_propagation.junction_tree

    @E.serialized
    def estimate_batch(self, marginals, targets, totals=None, metric="L2", iterations=100, stepsize=None):
        """Fit B measured rows of the same marginals in one launch.  `targets` [B, n_y] (device tensor or array): row b
        holds the cells of every marginal, C-ordered in the marginal's own variable order, one marginal after the other;
        `totals` [B]: each row's number of records (None: the sum of the row's first marginal).  Every row starts from
        `self.theta`, or else from the tree's factors.  Returns the device tensors (theta [B, n_cells], mu [B, n_cells],
        values [B, 2]: the loss and the final alpha, trials [B, 2]: trials taken and rejected); the estimator and its
        tree are left as they are."""
        import torch

        if metric not in ("L1", "L2"):
            raise ValueError("Metric must be one of L1 or L2.")
        plan = self._plan([tuple(m) for m in marginals])
        _, order, _, _, _ = self._tree()
        targets = targets if isinstance(targets, torch.Tensor) else E.to_device(np.atleast_2d(targets))
        if totals is None:
            totals = targets[:, :plan.y_offsets[1]].sum(dim=1)
        totals = totals if isinstance(totals, torch.Tensor) else E.to_device(np.asarray(totals, dtype=np.float64).reshape(-1))
        return plan.run(targets.contiguous(), totals.contiguous(), E.to_device(self._start(order)), metric, iterations, stepsize)
