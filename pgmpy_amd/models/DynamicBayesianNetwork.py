"""DynamicBayesianNetwork: the two-slice temporal network (2-TBN) of pgmpy/models/DynamicBayesianNetwork.py.

The class is host-side bookkeeping: nodes are ``(name, time_slice)`` pairs of slices 0 and 1, an
intra-slice edge is copied to the other slice, an inter-slice edge goes from slice 0 to slice 1.
What computes runs on the device through the static network:

* ``fit`` takes the constant network (``get_constant_bn``, a DiscreteBayesianNetwork) and calls its
  ``fit`` on slices (0, 1) and ``fit_update`` on every later pair, so the counts run in the family-count
  kernel.  As in the reference the result is an average of normalised CPDs, not pooled counts.
* ``fit(estimator="EM")`` / ``fit_codes`` learn from incomplete sequences (Baum-Welch): an iteration is one
  launch of the E-step kernel over the whole batch (csrc/pgmdbn.hip k_dbn_estep, through
  ``DBNInference.expected_counts_codes``'s plan) and one ``pgm_fit_finish`` per slice set.
* ``simulate`` / ``simulate_codes`` unroll the network over the slices asked for and call the device
  sampler once.  ``simulate_codes`` returns the resident uint8 code matrix in the layout
  ``DBNInference.smooth_codes`` reads: column ``t * n + v`` is node ``v`` (sorted name order) of slice t.

Inference over sequences is pgmpy_amd.inference.DBNInference.
"""
from collections import defaultdict
from itertools import combinations

import networkx as nx
import numpy as np

from .. import engine as E
from ..factors.discrete import TabularCPD


class DynamicNode(tuple):
    """A node of a dynamic network: ``(node, time_slice)``.  It is a tuple, so it equals, hashes and
    sorts as the plain pair does and either can be used wherever the other is."""

    __slots__ = ()

    def __new__(cls, node, time_slice):
        return tuple.__new__(cls, (node, time_slice))

    @property
    def node(self):
        return tuple.__getitem__(self, 0)

    @property
    def time_slice(self):
        return tuple.__getitem__(self, 1)

    def __getitem__(self, idx):
        if idx in (0, 1):
            return tuple.__getitem__(self, idx)
        raise IndexError(f"Index {idx} out of bounds.")

    def __eq__(self, other):
        if isinstance(other, list):
            other = tuple(other)
        return tuple.__eq__(self, other) is True

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = tuple.__hash__

    def __str__(self):
        return f"({self.node}, {self.time_slice})"

    def __repr__(self):
        return f"<DynamicNode({self.node}, {self.time_slice}) at {hex(id(self))}>"

    def to_tuple(self):
        return (self.node, self.time_slice)


def _flat(node, shift=0):
    """The static network's name of a dynamic node: ``{name}_{time_slice + shift}``."""
    return f"{node[0]}_{node[1] + shift}"


def _check_slice(time_slice, message):
    if not isinstance(time_slice, int) or time_slice < 0:
        raise ValueError(message)


class DynamicBayesianNetwork(nx.DiGraph):
    def __init__(self, ebunch=None):
        super().__init__()
        self.cpds = []
        self.cardinalities = defaultdict(int)
        if ebunch:
            self.add_edges_from(ebunch)

    # ------------------------------------------------------------------ structure
    def _graph_nodes(self):
        return super().nodes()

    def add_node(self, node, **attr):
        super().add_node(DynamicNode(node, 0), **attr)

    def add_nodes_from(self, nodes, **attr):
        for node in nodes:
            self.add_node(node)

    def _nodes(self):
        """The names of the slice nodes, each once, in the order they were added."""
        return list(dict.fromkeys(node for node, _ in self._graph_nodes()))

    def _timeslices(self):
        return sorted({t for _, t in self._graph_nodes()})

    def get_parents(self, node):
        return list(self.predecessors(node))

    def get_children(self, node):
        return list(self.successors(node))

    def add_edge(self, start, end, **kwargs):
        bad = "Nodes must be of type (node, time_slice)."
        try:
            if len(start) != 2 or len(end) != 2:
                raise ValueError(bad)
            if not isinstance(start[1], int) or not isinstance(end[1], int):
                raise ValueError(bad)
            gap = end[1] - start[1]
        except TypeError:
            raise ValueError(bad)
        if gap < 0:
            raise NotImplementedError("Edges in backward direction are not allowed.")
        if gap > 1:
            raise ValueError("Edges over multiple time slices is not currently supported")
        start, end = DynamicNode(start[0], 0), DynamicNode(end[0], gap)
        if start == end:
            raise ValueError("Self Loops are not allowed")
        known = self._graph_nodes()
        if start in known and end in known and nx.has_path(self, end, start):
            raise ValueError(f"Loops are not allowed. Adding the edge from ({str(start)} --> {str(end)}) forms a loop.")
        super().add_edge(start, end, **kwargs)
        if gap == 0:  # the copy in the other slice
            super().add_edge(DynamicNode(start[0], 1), DynamicNode(end[0], 1))
        else:
            super().add_node(DynamicNode(end[0], 0))

    def add_edges_from(self, ebunch, **kwargs):
        for edge in ebunch:
            self.add_edge(edge[0], edge[1])

    def get_intra_edges(self, time_slice=0):
        _check_slice(time_slice, "The timeslice should be a positive value greater than or equal to zero")
        return [tuple(DynamicNode(x[0], time_slice) for x in edge) for edge in self.edges()
                if edge[0][1] == edge[1][1] == 0]

    def get_inter_edges(self):
        return [edge for edge in self.edges() if edge[0][1] != edge[1][1]]

    def get_interface_nodes(self, time_slice=0):
        _check_slice(time_slice, "The timeslice should be a positive integer greater than"
                                 f" or equal to zero: ({type(time_slice)}, value: {time_slice})")
        return [DynamicNode(edge[time_slice][0], edge[time_slice][1]) for edge in self.get_inter_edges()]

    def get_slice_nodes(self, time_slice=0):
        _check_slice(time_slice, "The timeslice should be a positive value greater than or equal to zero")
        return [DynamicNode(node, time_slice) for node in self._nodes()]

    # ------------------------------------------------------------------ CPDs
    def add_cpds(self, *cpds):
        known = set(self._graph_nodes())
        for cpd in cpds:
            if not isinstance(cpd, TabularCPD):
                raise ValueError("cpd should be an instance of TabularCPD")
            if set(cpd.variables) - known:
                raise ValueError("CPD defined on variable not in the model", cpd)
        self.cpds.extend(cpds)

    def get_cpds(self, node=None, time_slice=None):
        if time_slice is None:
            time_slices = self._timeslices()
        elif isinstance(time_slice, int) and time_slice >= 0:
            time_slices = [time_slice]
        elif hasattr(time_slice, "__iter__"):
            if not all(isinstance(n, int) for n in time_slice):
                raise ValueError("At least one element inside time_slice iterable is not positive and/or integer")
            time_slices = time_slice
        else:
            raise ValueError("Time slice is not a positive integer neither a iterable of integers")
        if node:
            if node not in self._graph_nodes():
                raise ValueError("Node not present in the model.")
            for cpd in self.cpds:
                if cpd.variable == node:
                    return cpd
            return None
        found = []
        for t in time_slices:
            for var in self.get_slice_nodes(time_slice=t):
                cpd = self.get_cpds(node=var) if var in self._graph_nodes() else None
                if cpd:
                    found.append(cpd)
        return found

    def remove_cpds(self, *cpds):
        for cpd in cpds:
            if isinstance(cpd, (tuple, list)):
                cpd = self.get_cpds(cpd)
            self.cpds.remove(cpd)

    @property
    def states(self):
        return {node: names for cpd in self.cpds for node, names in cpd.state_names.items()}

    def check_model(self):
        for node in self._graph_nodes():
            cpd = self.get_cpds(node=node)
            if not isinstance(cpd, TabularCPD):
                continue
            if set(cpd.variables[1:]) != set(self.get_parents(node)):
                raise ValueError(f"CPD associated with {node} doesn't have proper parents associated with it.")
            columns = np.asarray(cpd._values_readonly(), dtype=np.float64).sum(axis=0)
            if not np.allclose(columns, 1.0, atol=0.01):
                raise ValueError(f"Sum of probabilities of states for node {node} is not equal to 1")
        return True

    def initialize_initial_state(self):
        """Give every node that has a CPD in one slice only its CPD in the other one: the same table when
        the node's parents there are the copies of its parents here, the table with the parents summed out
        when it has none there (a node whose only parents are in the slice before)."""
        for cpd in list(self.cpds):
            twin = DynamicNode(cpd.variable[0], 1 - cpd.variable[1])
            if any(c.variable == twin for c in self.cpds):
                continue
            parents = self.get_parents(twin)
            if not all(p[1] == parents[0][1] for p in parents):
                continue
            state_names = dict(self.states)
            state_names[twin] = state_names[cpd.variable]
            card = int(cpd.cardinality[0])
            if parents:
                values = np.asarray(cpd._values_readonly(), dtype=np.float64).reshape(card, -1)
                new = TabularCPD(twin, card, values, parents, [int(k) for k in cpd.cardinality[1:]],
                                 {v: state_names[v] for v in [twin] + parents})
            else:
                base = cpd.marginalize(list(cpd.variables[1:]), inplace=False) if len(cpd.variables) > 1 else cpd
                values = np.asarray(base._values_readonly(), dtype=np.float64).reshape(card, 1)
                new = TabularCPD(twin, card, values, state_names={twin: state_names[twin]})
            self.add_cpds(new)
        self.check_model()

    # ------------------------------------------------------------------ graph views
    def moralize(self):
        moral = self.to_undirected()
        for node in self._graph_nodes():
            moral.add_edges_from(combinations(self.get_parents(node), 2))
        return moral

    def copy(self):
        dbn = DynamicBayesianNetwork()
        dbn.add_nodes_from(self._nodes())
        dbn.add_edges_from([(tuple(u), tuple(v)) for u, v in self.edges()])
        dbn.add_cpds(*[cpd.copy() for cpd in self.get_cpds()])
        return dbn

    def _blanket(self, node):
        out = set(self.get_parents(node)) | set(self.get_children(node))
        for child in self.get_children(node):
            out.update(self.get_parents(child))
        out.discard(node)
        return out

    def get_markov_blanket(self, node):
        """Parents, children and the children's other parents; for a node of the last slice also the
        children it would have in the slice after, and their parents, found on the slice before."""
        node = DynamicNode(*node)
        blanket = self._blanket(node)
        if node.time_slice == max(t for _, t in self._graph_nodes()):
            before = DynamicNode(node.node, node.time_slice - 1)
            children = self.get_children(before) if before in self._graph_nodes() else []
            blanket |= {DynamicNode(c[0], c[1] + 1) for c in children}
            blanket |= {DynamicNode(p[0], p[1] + 1) for c in children for p in self.get_parents(c)}
        return sorted(blanket)

    def _static(self, shift=0, cpds=True):
        from .DiscreteBayesianNetwork import DiscreteBayesianNetwork

        bn = DiscreteBayesianNetwork([(_flat(u, shift), _flat(v, shift)) for u, v in self.edges()])
        bn.add_nodes_from(_flat(v, shift) for v in self._graph_nodes())
        if cpds and self.cpds:
            bn.add_cpds(*[_renamed(cpd, [_flat(v, shift) for v in cpd.variables]) for cpd in self.cpds])
        return bn

    def get_constant_bn(self, t_slice=0):
        """The part of the network that stays the same from slice to slice as a DiscreteBayesianNetwork
        over slices t_slice and t_slice + 1, its nodes named ``{name}_{time_slice}``."""
        return self._static(shift=t_slice)

    def active_trail_nodes(self, variables, observed=None, include_latents=False):
        from .DiscreteBayesianNetwork import DiscreteBayesianNetwork

        def wrap(x):
            if len(x) == 2 and isinstance(x[1], int):
                return DynamicNode(*x)
            return [DynamicNode(*v) for v in x]

        variables = wrap(variables)
        if observed is not None and len(observed) > 0:
            observed = wrap(observed)
            observed = [observed] if isinstance(observed, DynamicNode) else observed
        graph = DiscreteBayesianNetwork()
        graph.add_nodes_from(self._graph_nodes())
        graph.add_edges_from(self.edges())
        starts = [variables] if isinstance(variables, DynamicNode) else variables
        return graph.active_trail_nodes(starts, observed, include_latents)

    # ------------------------------------------------------------------ unrolling
    def _slice_order(self):
        """The slice nodes in the column order of every code matrix: sorted by name."""
        return sorted(self._nodes())

    def _both_slices(self):
        """{name: (CPD of slice 0, CPD of slice 1)}; ValueError when one is missing."""
        out = {}
        for name in self._slice_order():
            pair = tuple(self.get_cpds(DynamicNode(name, t)) if DynamicNode(name, t) in self._graph_nodes() else None
                         for t in (0, 1))
            for t, cpd in enumerate(pair):
                if cpd is None:
                    raise ValueError(f"No CPD associated with ({name}, {t}): add it, or call initialize_initial_state()")
            out[name] = pair
        return out

    def unroll(self, n_time_slices):
        """(DiscreteBayesianNetwork over n_time_slices slices, its nodes in slice-major order).  Node
        ``{name}_{t}`` of slice t >= 1 carries the CPD of ``(name, 1)`` moved t - 1 slices on."""
        n_time_slices = int(n_time_slices)
        if n_time_slices < 1:
            raise ValueError(f"n_time_slices must be at least 1. Got {n_time_slices}")
        from ..factors.discrete.DiscreteFactor import values_epoch

        # kept while the CPDs and their values are the same, so the sampler's compiled plan of the network is reused
        key = (n_time_slices, tuple(id(c) for c in self.cpds), tuple(self.edges()), values_epoch())
        hit = self.__dict__.get("_unrolled")
        if hit is not None and hit[0] == key:
            return hit[1], hit[2]
        bn, columns = self._unroll(n_time_slices)
        self.__dict__["_unrolled"] = (key[:3] + (values_epoch(),), bn, columns)  # making the copies counts as a change
        return bn, columns

    def _unroll(self, n_time_slices):
        from .DiscreteBayesianNetwork import DiscreteBayesianNetwork

        self.check_model()
        pairs = self._both_slices()
        names = self._slice_order()
        columns = [_flat((name, t)) for t in range(n_time_slices) for name in names]
        bn = DiscreteBayesianNetwork()
        bn.add_nodes_from(columns)
        cpds = []
        for t in range(n_time_slices):
            for name in names:
                cpd = pairs[name][min(t, 1)]
                new_vars = [_flat(v, max(t - 1, 0)) for v in cpd.variables]
                bn.add_edges_from((p, new_vars[0]) for p in new_vars[1:])
                cpds.append(_renamed(cpd, new_vars))
        bn.add_cpds(*cpds)
        bn.__dict__["_sample_columns"] = columns
        return bn, columns

    # ------------------------------------------------------------------ learning and simulation
    def fit(self, data, estimator="MLE", max_iter=100, atol=1e-8, init_cpds=None, seed=None):
        """Learn the CPDs of both slices from a frame with ``(name, time_slice)`` columns.

        estimator="MLE" needs every cell observed: the two-slice network is fitted window by window.

        estimator="EM" (Baum-Welch; max_iter, atol, init_cpds and seed are its alone) takes incomplete
        sequences: a NaN cell is unobserved, a node whose columns are absent or all NaN is hidden.
        Cardinalities, state names and the starting values come from the CPDs the model carries for both
        slices; init_cpds="random" / "uniform" replaces the starting values of the nodes that are hidden or
        have a hidden parent by TabularCPD.get_random(seed=seed) / get_uniform.  One iteration is one launch of
        the E-step kernel and one pgm_fit_finish per slice set, the values staying on the device, until every
        entry satisfies |old - new| <= atol + 1e-5 |new| or max_iter is reached.  The slice-0 CPDs are fitted
        to slice 0 alone and the transition CPDs to slices 1 .. T: the maximum-likelihood estimate of the
        unrolled network (the "MLE" path pools every window's first slice into the slice-0 CPDs instead).
        Sets ``n_iter_`` and ``log_likelihoods_`` (per iteration, the log-likelihood of the sequences that
        are possible under the parameters the iteration started from)."""
        import pandas as pd

        if not isinstance(data, pd.DataFrame):
            raise ValueError(f"data must be a pandas dataframe. Got: {type(data)}")
        if min(t for _, t in data.columns) != 0:
            raise ValueError("data column names must start from time slice 0.")
        if estimator in {"EM", "em"}:
            inf = self._em_start(max_iter, atol, init_cpds)
            codes, observed = inf.encode(data)
            seen = (codes != 255).reshape(-1, len(inf.names), codes.shape[1]).any(axis=(0, 2))
            hidden = [name for name, s in zip(inf.names, seen) if not s]
            return self._fit_em(inf, E.to_device_raw(codes), observed, hidden, max_iter, atol, init_cpds, seed)
        if estimator not in {"MLE", "mle"}:
            raise ValueError("Only Maximum Likelihood Estimator (\"MLE\") and expectation maximisation (\"EM\") are supported currently")
        n_samples = data.shape[0]
        last = max(t for _, t in data.columns)
        const_bn = self._static(cpds=False)
        names = self._nodes()
        for t in range(last):
            window = data.loc[:, [(name, t + h) for h in (0, 1) for name in names]]
            window.columns = [_flat((name, h)) for h in (0, 1) for name in names]
            if t == 0:
                const_bn.fit(window)
            else:
                const_bn.fit_update(window, n_prev_samples=t * n_samples)
        back = {_flat(v): v for v in self._graph_nodes()}
        self.add_cpds(*[_renamed(cpd, [back[v] for v in cpd.variables]) for cpd in const_bn.cpds])

    def fit_codes(self, codes, n_time_slices, observed=(), max_iter=100, atol=1e-8, init_cpds=None, seed=None):
        """``fit(estimator="EM")`` on a resident uint8 code matrix ``[n_time_slices * n, B]`` in the layout of
        ``simulate_codes`` (255: not observed): nothing leaves the device but one scalar per iteration and, at
        the end, the CPD values.  `observed`: the names observed in every cell of the batch (a 255 in one of
        their cells raises ValueError); with init_cpds="random" / "uniform" every other node counts as hidden."""
        inf = self._em_start(max_iter, atol, init_cpds)
        n = len(inf.names)
        if codes.dim() != 2 or int(codes.shape[0]) != int(n_time_slices) * n:
            raise ValueError(f"codes must be [n_time_slices * n, B] = [{int(n_time_slices)} * {n}, B]. Got {tuple(codes.shape)}")
        observed = set(observed)
        hidden = [name for name in inf.names if name not in observed]
        return self._fit_em(inf, codes, observed, hidden, max_iter, atol, init_cpds, seed)

    def _em_start(self, max_iter, atol, init_cpds):
        """The checks of the EM path that need no data, and the DBNInference of the model (which names a
        node without a CPD in either slice)."""
        import numbers

        from ..inference.dbn_inference import DBNInference

        if not isinstance(max_iter, numbers.Integral) or max_iter < 1:
            raise ValueError(f"max_iter must be a positive integer. Got: {max_iter}")
        if not (isinstance(atol, numbers.Real) and atol >= 0):
            raise ValueError(f"atol must be a non-negative number. Got: {atol}")
        if init_cpds is not None and not (isinstance(init_cpds, str) and init_cpds in ("random", "uniform")):
            raise ValueError(f"init_cpds must be None (start from the model's CPDs), 'random' or 'uniform'. Got: {init_cpds!r}")
        return DBNInference(self)

    @E.serialized
    def _fit_em(self, inf, codes, observed, hidden, max_iter, atol, init_cpds, seed):
        import torch

        from ..estimators._fit import FitPlan
        from ..inference._dbn import flat_values
        from ..inference.batch import download

        n = len(inf.names)
        cpds = [list(inf.cpds0), list(inf.cpds1)]
        if init_cpds is not None:
            make = TabularCPD.get_random if init_cpds == "random" else TabularCPD.get_uniform
            hidden = set(hidden)
            for group in cpds:
                for j, cpd in enumerate(group):
                    scope = list(cpd.variables)
                    if any(name in hidden for name, _ in scope):
                        group[j] = make(variable=scope[0], evidence=scope[1:],
                                        cardinality={v: int(k) for v, k in zip(scope, cpd.cardinality)},
                                        state_names={v: cpd.state_names[v] for v in scope}, seed=seed)
        plan = inf.plan(observed, [])
        # a fit plan over the same family lists has the layout of the values: its finish is the M-step
        fits = [FitPlan(inf.families0), FitPlan(inf.families1)]
        assert fits[0].offsets == plan.offsets0 and fits[1].offsets == plan.offsets1
        values = [E.to_device(flat_values(group)) for group in cpds]
        new = [torch.empty_like(v) for v in values]
        tables = [torch.empty_like(v) for v in values]
        one_slice = int(codes.shape[0]) == n  # no transition is in the data: the transition CPDs stay
        ll = torch.zeros(int(max_iter), dtype=torch.float64, device=values[0].device)
        self.n_iter_ = 0
        for it in range(int(max_iter)):
            for t in tables:
                t.zero_()
            _, _, loglik, flags = plan.estep(codes, values[0], values[1], tables[0], tables[1])
            fits[0].finish(tables[0], out=new[0])
            if one_slice:
                new[1].copy_(values[1])
            else:
                fits[1].finish(tables[1], out=new[1])
            ll[it] = torch.where(flags != 0, torch.zeros_like(loglik), loglik).sum()
            # np.allclose(old, new, atol=atol) over both sets: a NaN never converges
            close = torch.stack([((v - w).abs() <= atol + 1e-5 * w.abs()).all() for v, w in zip(values, new)]).all()
            values, new = new, values
            self.n_iter_ = it + 1
            if int(download(close.to(torch.uint8).reshape(1))[0]):
                break
        self.log_likelihoods_ = [float(x) for x in download(ll)[:self.n_iter_]]
        fitted = []
        for k, group in enumerate(cpds):
            host = download(values[k])
            for f, cpd in enumerate(group):
                card = [int(c) for c in cpd.cardinality]
                table = host[fits[k].offsets[f]:fits[k].offsets[f] + fits[k].sizes[f]].reshape(card[0], -1)
                fitted.append(TabularCPD(cpd.variable, card[0], table, evidence=list(cpd.variables[1:]) or None,
                                         evidence_card=card[1:] or None,
                                         state_names={v: cpd.state_names[v] for v in cpd.variables}))
        done = {c.variable for c in fitted}
        self.cpds = [c for c in self.cpds if c.variable not in done] + fitted

    def _back(self, n_time_slices):
        return {_flat((name, t)): (name, t) for t in range(n_time_slices) for name in self._nodes()}

    def simulate(self, n_samples=10, n_time_slices=2, do=None, evidence=None, virtual_evidence=None,
                 virtual_intervention=None, include_latents=False, seed=None, show_progress=True):
        """Simulate sequences: the network is unrolled over n_time_slices and the device sampler runs
        once, so evidence conditions the whole sequence.  Returns a frame with ``(name, t)`` columns,
        slice by slice.  include_latents and show_progress are accepted; a dynamic network has no
        latent set."""
        bn, columns = self.unroll(n_time_slices)
        flat_cpd = [[_renamed(cpd, [_flat(v) for v in cpd.variables]) for cpd in (group or [])]
                    for group in (virtual_evidence, virtual_intervention)]
        sampled = bn.simulate(n_samples=n_samples, do={_flat(v): s for v, s in (do or {}).items()},
                              evidence={_flat(v): s for v, s in (evidence or {}).items()},
                              virtual_evidence=flat_cpd[0], virtual_intervention=flat_cpd[1], include_latents=True,
                              seed=seed, show_progress=False)
        sampled = sampled.loc[:, columns]
        back = self._back(n_time_slices)
        sampled.columns = [back[c] for c in columns]
        return sampled

    def simulate_codes(self, n_samples, n_time_slices, seed=None):
        """The resident uint8 code matrix ``[n_time_slices * n, n_samples]`` of the unrolled network:
        column ``t * n + v`` is node v (sorted name order) of slice t."""
        from ..sampling import BayesianModelSampling

        bn, columns = self.unroll(n_time_slices)
        codes, nodes = BayesianModelSampling(bn).forward_sample_codes(n_samples, seed=seed)
        assert list(nodes) == columns
        return codes


def _renamed(cpd, new_vars):
    """`cpd` over other variable names, its values and state names kept."""
    card = [int(k) for k in cpd.cardinality]
    values = np.asarray(cpd._values_readonly(), dtype=np.float64).reshape(card[0], -1)
    names = {new: cpd.state_names[old] for new, old in zip(new_vars, cpd.variables)}
    return TabularCPD(new_vars[0], card[0], values, evidence=list(new_vars[1:]) or None, evidence_card=card[1:] or None,
                      state_names=names)
