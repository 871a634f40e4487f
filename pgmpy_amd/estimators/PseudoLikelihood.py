"""PseudoLikelihoodEstimator: the potentials of a DiscreteMarkovNetwork from data, by maximum pseudo-likelihood.

The reference's undirected learner (MirrorDescentEstimator, built here too) needs a junction tree; Besag's
pseudo-likelihood

    PL(theta) = sum_rows sum_i log p(x_i | x_MB(i); theta),   p(x_i = s | .) prop. to exp sum_{f holds i} theta_f(s, x_{f\\i})

needs no partition function, so it works at any treewidth; it is concave in the log-potentials theta and consistent.
A row enters only through the configuration of a node and its blanket, so the rows are counted once (the fused
family-count kernel, on the blanket families) and every evaluation of PL and its gradient is one pgm_mnpl_eval on the
count tables (csrc/pgmmnpl.hip): its cost does not depend on the number of rows.  The optimiser is torch.optim.LBFGS
with a strong-Wolfe line search on the device-resident theta.  Value and gradient are fixed-order fp64 sums, so a fit
is reproducible bit for bit.

A row with a missing cell is dropped per node, for the nodes whose blanket family holds the cell (the family count's
rule).  There is no CPU path: without a device a compute call raises ``NativeUnavailable``.
"""
import warnings

import numpy as np

from .. import engine as E
from ..sampling import column_order
from ._mnpl import MnplPlan
from .base import BaseEstimator


class PseudoLikelihoodEstimator(BaseEstimator):
    def __init__(self, model, data=None, state_names=None, scopes=None):
        """`scopes`: the variables of every factor to fit, each in the order of its table; None: the scopes of the
        model's factors when it has some, else one factor per edge and one per isolated node.  State names default to
        the model's (when it has factors), then to what the data holds."""
        from ..models import DiscreteMarkovNetwork

        if not isinstance(model, DiscreteMarkovNetwork):
            raise TypeError(f"model must be a DiscreteMarkovNetwork. Got {type(model)}")
        self.model = model
        self.nodes = column_order(model)
        known = dict(model.states) if model.factors else {}
        if isinstance(state_names, dict):
            known.update(state_names)
        if data is not None:
            missing = [v for v in self.nodes if v not in data.columns]
            if missing:
                raise ValueError(f"data has no column for {missing}")
            data = data[self.nodes]
        super().__init__(data, state_names=known)
        if data is None:
            self.state_names = known
        self._resident = None
        self._scopes = self._default_scopes() if scopes is None else [tuple(s) for s in scopes]
        unknown = [v for s in self._scopes for v in s if v not in model.nodes()]
        if unknown:
            raise ValueError(f"scopes name {unknown}, not in the model")
        self._built = None

    @classmethod
    def from_codes(cls, model, codes, nodes=None, card=None, state_names=None, scopes=None):
        """The resident form: `codes` is a uint8 device tensor [n_nodes, n_rows] of state codes (255: missing), its
        rows in the order of `nodes` (default: column_order(model), what GibbsSampling.sample_codes returns).
        Cardinalities come from `card` ({node: states}), else from the model's factors, else from the codes."""
        est = cls(model, None, state_names, scopes)
        est.nodes = list(est.nodes if nodes is None else nodes)
        if sorted(map(str, est.nodes)) != sorted(map(str, model.nodes())):
            raise ValueError("nodes must list every node of the model once")
        E.device()
        if codes.dim() != 2 or int(codes.shape[0]) != len(est.nodes):
            raise ValueError(f"codes must be [{len(est.nodes)}, n_rows]")
        have = dict(model.get_cardinality()) if model.factors else {}
        have.update(card or {})
        for j, v in enumerate(est.nodes):
            if v in est.state_names:
                continue
            if v not in have:  # the largest code that is not the missing mark
                col = codes[j]
                have[v] = int(col[col != 255].max().item()) + 1
            est.state_names[v] = list(range(int(have[v])))
        est._resident = codes
        return est

    def _default_scopes(self):
        if self.model.factors:
            return [tuple(f.variables) for f in self.model.factors]
        at = {v: j for j, v in enumerate(self.nodes)}
        edges = sorted(tuple(sorted(e, key=at.__getitem__)) for e in self.model.edges())
        return edges + [(v,) for v in self.nodes if self.model.degree(v) == 0]

    # ------------------------------------------------------------------ device side
    def _build(self):
        """(plan, int64 count tables of the blanket families, rows): the one pass over the data."""
        if self._built is None:
            codes = self._resident if self._resident is not None else self._codes()[0]
            at = {v: j for j, v in enumerate(self.nodes)}
            card = [len(self.state_names[v]) for v in self.nodes]
            plan = MnplPlan([([at[v] for v in s], [card[at[v]] for v in s]) for s in self._scopes], card)
            self._built = (plan, plan.fit_plan().count(codes), int(codes.shape[1]))
        return self._built

    @property
    def plan(self):
        return self._build()[0]

    @E.serialized
    def value_and_grad(self, theta, l2=0.0, want_grad=True):
        """(value [1], grad [n_theta]) on the device: PL(theta) - l2 / 2 |theta|^2 and its gradient at the device
        fp64 `theta`, factor f of the scopes at ``plan.offsets[f]``.  One pgm_mnpl_eval."""
        plan, counts, _ = self._build()
        value, grad, _ = plan.eval(counts, theta, l2, want_grad)
        return value, grad

    def _factors(self, theta):
        import torch

        from ..factors.discrete import DiscreteFactor

        plan = self.plan
        values = torch.exp(theta)
        out = []
        for f, scope in enumerate(self._scopes):
            cards = [len(self.state_names[v]) for v in scope]
            table = values[plan.offsets[f]:plan.offsets[f] + plan.sizes[f]].reshape(cards)
            out.append(DiscreteFactor(list(scope), cards, table, state_names={v: list(self.state_names[v]) for v in scope}))
        return out

    @E.serialized
    def estimate(self, l2=0.0, max_iter=200, tol=1e-7, init=None):
        """The fitted factors, one DiscreteFactor per scope holding exp(theta): multiplicative potentials, what
        LoopyBeliefPropagation and GibbsSampling read (and ``Mplp(model, log=True)``).

        theta maximises PL(theta) - l2 / 2 |theta|^2 from `init` (a flat array of log-potentials; default 0) by
        L-BFGS; every closure call is one pgm_mnpl_eval.  The fit stops when max |grad| / n_rows <= tol, read once
        per outer iteration, or after `max_iter` of them (a warning; ``converged`` tells).  ``theta`` keeps the
        result on the device, ``n_iter`` and ``n_eval`` the outer iterations and the evaluations used.

        l2 = 0 is the plain estimator.  A state that never occurs under some blanket configuration then has no
        finite optimum: its log-potential runs to -inf and the fit only stops at `max_iter`.  Give l2 > 0 (a
        Gaussian prior on theta) for sparse data."""
        import torch

        plan, counts, n_rows = self._build()
        if init is None:
            theta = torch.zeros(plan.n_theta, dtype=torch.float64, device=counts.device)
        else:
            theta = E.to_device(np.asarray(init, dtype=np.float64).reshape(-1))
            if theta.numel() != plan.n_theta:
                raise ValueError(f"init has {theta.numel()} entries, the scopes need {plan.n_theta}")
        scale = 1.0 / max(n_rows, 1)
        theta.requires_grad_(True)
        opt = torch.optim.LBFGS([theta], lr=1.0, max_iter=20, history_size=20, tolerance_grad=float(tol),
                                tolerance_change=0.0, line_search_fn="strong_wolfe")
        self.n_eval = 0

        def closure():  # the loss LBFGS minimises: - (PL - ridge) / n_rows
            value, grad, _ = plan.eval(counts, theta.detach(), l2)
            self.n_eval += 1
            theta.grad = grad.mul_(-scale)
            return value[0] * -scale

        self.converged, self.n_iter = False, 0
        while True:
            _, grad, _ = plan.eval(counts, theta.detach(), l2)
            self.n_eval += 1
            self.converged = float(grad.abs().max()) * scale <= tol  # the one read of the iteration
            if self.converged or self.n_iter >= int(max_iter):
                break
            opt.step(closure)
            self.n_iter += 1
        if not self.converged:
            warnings.warn(f"PseudoLikelihoodEstimator: max |grad| / n_rows is above {tol} after {max_iter} iterations "
                          "(a state unseen under some blanket configuration has no finite optimum: give l2 > 0)")
        self.theta = theta.detach()
        return self._factors(self.theta)

    def get_parameters(self, **kwargs):
        """A copy of the model carrying the factors of ``estimate(**kwargs)``."""
        factors = self.estimate(**kwargs)
        model = self.model.copy()
        model.factors = []
        for scope in self._scopes:  # a factor's scope must be a clique of the graph
            model.add_edges_from((a, b) for i, a in enumerate(scope) for b in scope[i + 1:])
        model.add_factors(*factors)
        return model
