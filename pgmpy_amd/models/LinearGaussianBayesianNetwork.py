"""LinearGaussianBayesianNetwork: a DAG whose CPDs are linear Gaussians, with pgmpy's names and semantics
(pgmpy/models/LinearGaussianBayesianNetwork.py) and the data paths on the device.

  fit             one upload, one column-sum launch, one fp64 MFMA Gram launch, one download of (d + 1)^2
                  numbers; every node's regression is then a small host solve (models/_lg.py ols).  The
                  reference runs one scikit-learn LinearRegression per node over the frame.
  log_likelihood  the factorised density, one lane per row (pgm_lg_logpdf): mathematically the reference's
                  scipy multivariate_normal.logpdf of the joint.
  predict         W = cov_ab cov_bb^-1 and cov_cond on the host, the rows through pgm_lg_affine.
  simulate        forward sampling on the Philox stream (pgm_lg_sample): equal to the reference's numpy
                  multivariate_normal draws in distribution, not in value.  Evidence conditions the joint on the
                  host and turns N(m, C) into a dense chain of regressions the same kernel draws.

fit_values / log_likelihood_values / simulate_values / predict_values work on a resident matrix: a contiguous
torch.float64 device tensor X[n_cols, ld] (X[col, row]), `columns` naming the variable of each column.

Deviation: to_joint_gaussian is not rounded to 8 decimals (the reference rounds to hide asymmetry of
inv.T @ omega @ inv; nothing here depends on exact symmetry).  There is no CPU fallback: without a GPU
the compute calls raise NativeUnavailable.
"""
import logging

import networkx as nx
import numpy as np

from .. import engine as E
from .._plan import MASK64
from ..factors.continuous import LinearGaussianCPD
from . import _lg

logger = logging.getLogger("pgmpy")


class LinearGaussianBayesianNetwork(nx.DiGraph):
    def __init__(self, ebunch=None, latents=set(), lavaan_str=None, dagitty_str=None):
        super().__init__()
        self.cpds = []
        self.latents = set(latents)
        if ebunch:
            self.add_edges_from(ebunch)

    # ------------------------------------------------------------------ structure
    def add_edge(self, u, v, **kwargs):
        if u == v:
            raise ValueError("Self loops are not allowed.")
        if u in self.nodes() and v in self.nodes() and nx.has_path(self, v, u):
            raise ValueError(f"Loops are not allowed. Adding the edge from ({u}->{v}) forms a loop.")
        super().add_edge(u, v, **kwargs)

    def add_edges_from(self, ebunch, **kwargs):
        for e in ebunch:
            self.add_edge(*e[:2], **kwargs)

    def get_parents(self, node):
        return list(self.predecessors(node))

    def get_children(self, node):
        return list(self.successors(node))

    # ------------------------------------------------------------------ CPDs
    def add_cpds(self, *cpds):
        for cpd in cpds:
            if not isinstance(cpd, LinearGaussianCPD):
                raise ValueError("Only LinearGaussianCPD can be added.")
            if set(cpd.variables) - set(self.nodes()):
                raise ValueError("CPD defined on variable not in the model", cpd)
            for i, old in enumerate(self.cpds):
                if old.variable == cpd.variable:
                    logger.warning(f"Replacing existing CPD for {cpd.variable}")
                    self.cpds[i] = cpd
                    break
            else:
                self.cpds.append(cpd)

    def get_cpds(self, node=None):
        if node is None:
            return self.cpds
        if node not in self.nodes():
            raise ValueError("Node not present in the Directed Graph")
        for cpd in self.cpds:
            if cpd.variable == node:
                return cpd
        return None

    def remove_cpds(self, *cpds):
        for cpd in cpds:
            if isinstance(cpd, (str, int)):
                cpd = self.get_cpds(cpd)
            self.cpds.remove(cpd)

    def check_model(self):
        for node in self.nodes():
            cpd = self.get_cpds(node=node)
            if isinstance(cpd, LinearGaussianCPD) and set(cpd.evidence) != set(self.get_parents(node)):
                raise ValueError("CPD associated with %s doesn't have proper parents associated with it." % node)
        return True

    def get_cardinality(self, node=None):
        raise ValueError("Cardinality is not defined for continuous variables.")

    def copy(self):
        m = LinearGaussianBayesianNetwork(latents=self.latents)
        m.add_nodes_from(self.nodes())
        m.add_edges_from(self.edges())
        if self.cpds:
            m.add_cpds(*[cpd.copy() for cpd in self.cpds])
        return m

    def to_markov_model(self):
        raise NotImplementedError("to_markov_model method has not been implemented for LinearGaussianBayesianNetwork.")

    def is_imap(self, JPD):
        raise NotImplementedError("is_imap method has not been implemented for LinearGaussianBayesianNetwork.")

    def get_random_cpds(self, loc=0, scale=1, inplace=False, seed=None):
        """One LinearGaussianCPD.get_random per node, node i of self.nodes() with seed + i (42 when no seed)."""
        seed = seed if seed else 42
        cpds = [LinearGaussianCPD.get_random(variable=v, evidence=self.get_parents(v), loc=loc, scale=scale, seed=seed + i)
                for i, v in enumerate(self.nodes())]
        if not inplace:
            return cpds
        self.add_cpds(*cpds)

    @staticmethod
    def get_random(n_nodes=5, edge_prob=0.5, node_names=None, latents=False, loc=0, scale=1, seed=None):
        """A random DAG (the upper triangle of an n x n Bernoulli(edge_prob) matrix drawn WITHOUT the seed,
        as the reference's call does) with get_random_cpds(loc, scale, seed)."""
        gen = np.random.default_rng()
        adj = np.triu(gen.choice([0, 1], size=(n_nodes, n_nodes), p=[1 - edge_prob, edge_prob]), k=1)
        names = [f"X_{i}" for i in range(n_nodes)] if node_names is None else list(node_names)
        m = LinearGaussianBayesianNetwork()
        # the nodes in the order the edges name them, then the isolated ones: get_random_cpds seeds node i with seed + i
        m.add_edges_from((names[i], names[j]) for i, j in zip(*np.nonzero(adj)))
        m.add_nodes_from(names)
        if latents:
            m.latents = set(gen.choice(list(m.nodes()), gen.integers(low=0, high=n_nodes)))
        m.add_cpds(*m.get_random_cpds(loc=loc, scale=scale, seed=seed))
        return m

    # ------------------------------------------------------------------ the joint Gaussian
    def to_joint_gaussian(self):
        """(mean, cov) over list(nx.topological_sort(self)): mean_v = beta_0 + sum beta_i mean_{p_i}; with B the
        matrix of edge coefficients (B[parent, child]) and Omega = diag(std^2), cov = (I - B)^-T Omega (I - B)^-1.
        Not rounded (module docstring)."""
        order = list(nx.topological_sort(self))
        pos = {v: i for i, v in enumerate(order)}
        n = len(order)
        mean, B, omega = np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
        for v in order:
            cpd = self.get_cpds(v)
            mean[pos[v]] = (cpd.beta * np.array([1.0] + [mean[pos[u]] for u in cpd.evidence])).sum()
            for i, u in enumerate(cpd.evidence):
                B[pos[u], pos[v]] = cpd.beta[i + 1]
            omega[pos[v], pos[v]] = cpd.std ** 2
        inv = np.linalg.inv(np.eye(n) - B)
        return mean, inv.T @ omega @ inv

    # ------------------------------------------------------------------ plans
    def _families(self, columns):
        """(order, plan, coef, konst): the network handle over `columns` (a list naming every node's column),
        its flat coefficients and the constants -log std - 0.5 log 2 pi, nodes in topological order."""
        col = {v: i for i, v in enumerate(columns)}
        missing = set(self.nodes()) - set(col)
        if missing:
            raise ValueError(f"Missing required columns in DataFrame: {missing}")
        order = list(nx.topological_sort(self))
        self.check_model()
        cpds = [self.get_cpds(v) for v in order]
        for v, cpd in zip(order, cpds):
            if cpd is None:
                raise ValueError(f"No CPD associated with {v}")
        fams = tuple(tuple([col[c.variable]] + [col[u] for u in c.evidence]) for c in cpds)
        cache = self.__dict__.setdefault("_net_plans", {})
        if fams not in cache:
            cache.clear()
            cache[fams] = _lg.NetPlan(fams)
        plan = cache[fams]
        stds = [float(c.std) for c in cpds]
        coef = plan.coef([c.beta for c in cpds], stds)
        return order, plan, coef, np.array(stds)

    def _gram_plan(self, cols):
        cache = self.__dict__.setdefault("_gram_plans", {})
        key = tuple(cols)
        if key not in cache:
            cache.clear()
            cache[key] = _lg.GramPlan(cols)
        return cache[key]

    @staticmethod
    def _upload(data, variables):
        """The frame's columns `variables` as a device matrix [len(variables), n] (one upload)."""
        import torch

        from .. import _native as N

        N.lib()
        host = np.ascontiguousarray(data.loc[:, list(variables)].to_numpy(dtype=np.float64).T)
        return torch.from_numpy(host).cuda()

    # ------------------------------------------------------------------ fit
    def fit(self, data, estimator="mle", std_estimator="unbiased"):
        """OLS CPDs from a DataFrame: fit_values on its uploaded matrix."""
        self._fit_args(set(data.columns), estimator, std_estimator)
        nodes = list(self.nodes())
        return self.fit_values(self._upload(data, nodes), nodes, estimator=estimator, std_estimator=std_estimator)

    def _fit_args(self, columns, estimator, std_estimator):
        if len(missing_vars := (set(self.nodes()) - columns)) > 0:
            raise ValueError(f"Following variables are missing in the data: {missing_vars}")
        if estimator not in {"mle"}:
            raise ValueError("estimator must be one of {'mle', 'unbiased'}")
        if std_estimator not in {"mle", "unbiased"}:
            raise ValueError("std_estimator must be one of {'mle', 'unbiased'}")

    @E.serialized
    def fit_values(self, X, columns, estimator="mle", std_estimator="unbiased", n_rows=None, row0=0):
        """OLS CPDs from the rows [row0, row0 + n_rows) of a resident matrix; `columns[c]` names column c
        (columns that are no node are not read).  Raises ValueError when a used column holds NaN or Inf."""
        columns = list(columns)
        self._fit_args(set(columns), estimator, std_estimator)
        nodes = list(self.nodes())
        plan = self._gram_plan([columns.index(v) for v in nodes])
        G, shift = plan.moments_on_device(X, n_rows, row0)
        self.add_cpds(*self._finish_fit(nodes, G, shift, std_estimator))
        return self

    def _finish_fit(self, nodes, G, shift, std_estimator):
        """The CPDs from the downloaded Gram matrix of `nodes` (host only)."""
        d = len(nodes)
        bad = [v for j, v in enumerate(nodes) if not np.isfinite(G[j, j])]
        if bad:
            raise ValueError(f"the data holds NaN or Inf in the columns {bad}")
        n, mean, S = _lg.moments(G, shift)
        pos = {v: j for j, v in enumerate(nodes)}
        cpds = []
        for v in nodes:
            parents = self.get_parents(v)
            beta, std = _lg.ols(n, mean, S, pos[v], [pos[u] for u in parents], std_estimator)
            cpds.append(LinearGaussianCPD(variable=v, beta=beta, std=std, evidence=parents))
        assert len(cpds) == d
        return cpds

    # ------------------------------------------------------------------ log-likelihood
    def log_likelihood(self, data):
        """The total log-density of the frame's rows under the model."""
        missing = set(self.nodes()) - set(data.columns)
        if missing:
            raise ValueError(f"Missing required columns in DataFrame: {missing}")
        nodes = list(self.nodes())
        return float(self.log_likelihood_values(self._upload(data, nodes), nodes)[1])

    @E.serialized
    def log_likelihood_values(self, X, columns, total=True, n_rows=None, row0=0):
        """Per-row log-densities of the window, an fp64 device tensor [n_rows]; with `total` (logp, float)."""
        import torch

        _, plan, coef, stds = self._families(list(columns))
        if not (stds > 0).all():
            raise ValueError("every CPD needs std > 0 for a density")
        konst = -np.log(stds) - 0.5 * np.log(2 * np.pi)
        logp, tot = plan.logpdf(torch.from_numpy(coef).to(X.device), torch.from_numpy(konst).to(X.device), X, n_rows, row0,
                                total=total)
        return (logp, float(tot.cpu()[0])) if total else logp

    # ------------------------------------------------------------------ predict
    def _conditional(self, observed):
        """(missing_vars, observed_vars, W, c, cov_cond): x_a | x_b = N(c + W x_b, cov_cond), both lists in
        topological order."""
        missing = set(self.nodes()) - set(observed)
        if len(missing) == 0:
            raise ValueError("No missing variables in the data")
        mu, cov = self.to_joint_gaussian()
        order = list(nx.topological_sort(self))
        a = [i for i, v in enumerate(order) if v in missing]
        b = [i for i, v in enumerate(order) if v not in missing]
        W, cov_cond = _lg.condition(mu, cov, a, b)
        return [order[i] for i in a], [order[i] for i in b], W, mu[a] - W @ mu[b], cov_cond

    def predict(self, data, distribution="joint"):
        """(missing variables in topological order, mu_cond [n, |a|], cov_cond) for the frame's rows."""
        missing_vars, observed_vars, W, c, cov_cond = self._conditional(data.columns)
        if not observed_vars:
            return missing_vars, np.tile(c, (len(data), 1)), cov_cond
        mu = _lg.affine(W, c, list(range(len(observed_vars))), self._upload(data, observed_vars))
        return missing_vars, mu.cpu().numpy().T.copy(), cov_cond

    @E.serialized
    def predict_values(self, X, columns, n_rows=None, row0=0):
        """As predict on a resident matrix whose column c holds variable columns[c] (the nodes that are not
        named are the missing ones): (missing variables, mu_cond device tensor [|a|, n_rows], cov_cond)."""
        columns = list(columns)
        missing_vars, observed_vars, W, c, cov_cond = self._conditional([v for v in columns if v in self.nodes()])
        if not observed_vars:
            raise ValueError("No observed variables in the data")
        return missing_vars, _lg.affine(W, c, [columns.index(v) for v in observed_vars], X, n_rows, row0), cov_cond

    # ------------------------------------------------------------------ simulate
    @E.serialized
    def simulate_values(self, n, seed=None, first_row=0, out=None, row0=0):
        """Forward samples as a resident matrix [n_nodes, ld] whose column c is list(self.nodes())[c]: the rows
        [row0, row0 + n) of `out` (a new [n_nodes, n] tensor when None) are stream rows first_row ..  A row's
        values depend on (seed, stream row) alone."""
        import torch

        from .. import _native as N

        N.lib()
        nodes = list(self.nodes())
        _, plan, coef, _ = self._families(nodes)
        seed = int(np.random.SeedSequence().entropy & MASK64) if seed is None else int(seed)
        if out is None:
            out = torch.empty((len(nodes), int(n)), dtype=torch.float64, device="cuda")
        if int(n) == 0:
            return out
        plan.sample(torch.from_numpy(coef).to(out.device), out, int(n), row0, first_row, seed)
        return out

    def _intervened(self, do, virtual_intervention):
        """The model after the graph surgery of `do` (the nodes leave; a child's intercept absorbs beta * value)
        and of `virtual_intervention` (the given CPDs replace the nodes' own and cut their incoming edges)."""
        model = self.copy()
        for var, val in do.items():
            for parent in model.get_parents(var):
                model.remove_edge(parent, var)
            model.remove_cpds(model.get_cpds(var))
            for child in model.get_children(var):
                cpd = model.get_cpds(child)
                k = cpd.evidence.index(var)
                beta = list(cpd.beta)
                beta[0] += beta[k + 1] * val
                del beta[k + 1]
                model.remove_cpds(cpd)
                model.add_cpds(LinearGaussianCPD(child, beta, cpd.std, cpd.evidence[:k] + cpd.evidence[k + 1:]))
            model.remove_node(var)
        for cpd in virtual_intervention:
            model.remove_cpds(model.get_cpds(cpd.variable))
            model.add_cpds(cpd)
            for parent in model.get_parents(cpd.variable):
                model.remove_edge(parent, cpd.variable)
        return model

    def _evidence_chain(self, evidence):
        """(missing variables, the dense-chain model over them) of this model conditioned on `evidence`: the
        conditional N(m, C) of the joint as regressions x_j | x_<j, which simulate_values draws."""
        missing_vars, observed_vars, W, c, cov_cond = self._conditional(list(evidence))
        m = c + W @ np.array([float(evidence[v]) for v in observed_vars])
        chain = LinearGaussianBayesianNetwork()
        chain.add_nodes_from(missing_vars)
        for j, (beta, std) in enumerate(_lg.dense_chain(m, cov_cond)):
            chain.add_edges_from((u, missing_vars[j]) for u in missing_vars[:j])
            chain.add_cpds(LinearGaussianCPD(missing_vars[j], beta, std, missing_vars[:j]))
        return missing_vars, chain

    def simulate(self, n_samples=1000, do=None, evidence=None, virtual_intervention=None, include_latents=False, seed=None):
        """A DataFrame of n_samples rows drawn on the device (module docstring)."""
        import pandas as pd

        evidence = {} if evidence is None else evidence
        do = {} if do is None else do
        virtual_intervention = [] if virtual_intervention is None else virtual_intervention
        do_nodes, evidence_nodes = list(do.keys()), list(evidence.keys())
        if invalid_nodes := set(do_nodes) - set(self.nodes()):
            raise ValueError(f"The following do-nodes are not present in the model: {invalid_nodes}. "
                             f"do argument contains: {do_nodes}")
        if invalid_nodes := set(evidence_nodes) - set(self.nodes()):
            raise ValueError(f"The following evidence-nodes are not present in the model: {invalid_nodes}. "
                             f"evidence argument contains: {evidence_nodes}")
        self.check_model()
        if common_vars := set(do_nodes) & set(evidence_nodes):
            raise ValueError(f"Variable(s) can't be in both do and evidence: {', '.join(common_vars)}")
        for cpd in virtual_intervention:
            if cpd.variable not in self.nodes():
                raise ValueError(f"Virtual intervention provided for variable which is not in the model: {cpd.variable}"
                                 f"The following nodes are present in the model: {self.nodes()}")
        model = self._intervened(do, virtual_intervention)
        variables = list(nx.topological_sort(model))
        if evidence:
            drawn, sampler = model._evidence_chain(evidence)
        else:
            drawn, sampler = list(model.nodes()), model
        values = sampler.simulate_values(n_samples, seed=seed).cpu().numpy()
        frame = {v: values[j] for j, v in enumerate(drawn)}
        for v, val in evidence.items():
            frame[v] = np.full(n_samples, val)
        df = pd.DataFrame({v: frame[v] for v in variables}, columns=variables)
        for v, val in do.items():
            df[v] = val
        if not include_latents:
            df = df.drop(columns=list(self.latents))
        return df
