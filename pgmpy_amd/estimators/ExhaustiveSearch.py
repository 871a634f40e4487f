"""ExhaustiveSearch (mirror of pgmpy/estimators/ExhaustiveSearch.py:14-195): the DAG with the highest score.

The reference enumerates every DAG with networkx, which ends at six nodes.  A decomposable score is a sum of family
scores, so the same maximum comes from the dynamic programme of Silander and Myllymaki over the subset lattice: the
best parent set of every node within every candidate set, then the best sink of every set, then a walk down from the
full set (include/pgmhip.h "Exact structure search").  `estimate` enumerates the families on the host, scores them
with the scorer's batched `local_scores` and runs the programme on the device (pgm_xs_run): n * 2^(n-1) table cells,
up to 24 variables.  `edge_posteriors` takes the same families through the same lattice with a log-sum-exp in place
of the maximum (pgm_xs_posterior) and returns the exact posterior probability of every edge.

Deviations: `estimate` takes `max_indegree` and `expert_knowledge` (required and forbidden edges), which
the reference does not have; among DAGs of equal score the one the recurrence's tie rules pick is returned (fewer
parents, then the smaller mask; the smaller sink), not the first in networkx's enumeration; the result is a CPD-less
DiscreteBayesianNetwork, as HillClimbSearch returns.  `all_dags` and `all_scores` run on the host and are for small n.
"""
import logging
from itertools import combinations
from operator import itemgetter
from math import comb

import networkx as nx

from .. import _native as N
from .base import BaseEstimator, WEIGHT
from .HillClimbSearch import ExpertKnowledge
from .StructureScore import K2, get_scoring_method

logger = logging.getLogger("pgmpy_amd")

MAX_FAMILIES = 1 << 22  # families `estimate` will score; beyond it, it asks for max_indegree
SCORE_BATCH = 1 << 15   # families per local_scores call


def enumerate_families(n, max_indegree=None, forbidden=(), required=()):
    """[(v, parent mask)] over nodes 0 .. n - 1: every node with every parent set of at most `max_indegree` parents
    that holds no u of a forbidden (u, v) and every u of a required (u, v); by node, then by the number of parents,
    then in combination order.  A ValueError when there are more than MAX_FAMILIES."""
    cap = n - 1 if max_indegree is None else min(int(max_indegree), n - 1)
    forbidden, required = set(forbidden), set(required)
    plan, total = [], 0
    for v in range(n):
        must = [u for u in range(n) if (u, v) in required]
        free = [u for u in range(n) if u != v and (u, v) not in forbidden and (u, v) not in required]
        for u in must:
            if (u, v) in forbidden:
                raise ValueError(f"edge ({u}, {v}) is both required and forbidden")
        plan.append((must, free))
        total += sum(comb(len(free), k) for k in range(0, cap - len(must) + 1))
    if total > MAX_FAMILIES:
        raise ValueError(f"{total} families to score, more than {MAX_FAMILIES}: limit the parents of a node with max_indegree")
    families = []
    for v, (must, free) in enumerate(plan):
        base = sum(1 << u for u in must)
        for k in range(0, cap - len(must) + 1):
            families.extend((v, base | sum(1 << u for u in extra)) for extra in combinations(free, k))
    return families


class ExhaustiveSearch(BaseEstimator):
    def __init__(self, data, scoring_method=None, use_cache=True, **kwargs):
        super(ExhaustiveSearch, self).__init__(data, **kwargs)
        self.use_cache = use_cache
        if scoring_method is None:
            self.scoring_method = K2(data=self.data)  # the reference's default
        else:
            _, self.scoring_method = get_scoring_method(scoring_method, self.data, use_cache)
        self.best_score = None  # R[V] of the last estimate()
        self.n_families = None  # families it scored
        self.log_marginal = None  # F[V] of the last edge_posteriors()
        self._cache = {}

    def _nodes(self):
        return [v for v in self.variables if v != WEIGHT]

    def _scores(self, nodes, families, arc_prior=True):
        """The score of every (v, mask) family: local_scores in batches, plus (arc_prior) the per-arc prior."""
        def parents(mask):
            return [nodes[u] for u in range(len(nodes)) if mask >> u & 1]

        if not self.use_cache:
            self._cache = {}
        need = [f for f in families if f not in self._cache]
        for i in range(0, len(need), SCORE_BATCH):
            batch = need[i:i + SCORE_BATCH]
            for f, s in zip(batch, self.scoring_method.local_scores([(nodes[v], parents(m)) for v, m in batch])):
                self._cache[f] = s
        arc = self.scoring_method.structure_prior_ratio("+") if arc_prior else 0
        return [self._cache[f] + bin(f[1]).count("1") * arc for f in families]

    def _scored_families(self, max_indegree, expert_knowledge):
        """(nodes, families, scores) of `estimate` and `edge_posteriors`: their checks, the families that
        `max_indegree` and the required and forbidden edges leave, and their scores with the per-arc prior."""
        nodes = self._nodes()
        n = len(nodes)
        if n > N.XS_MAX_NODES:
            raise ValueError(f"ExhaustiveSearch: {n} variables; the exact search takes {N.XS_MAX_NODES} at most")
        if expert_knowledge is None:
            expert_knowledge = ExpertKnowledge()
        if getattr(expert_knowledge, "search_space", None) or any(getattr(expert_knowledge, "temporal_order", None) or []):
            raise NotImplementedError("ExpertKnowledge: temporal_order and search_space are not built")
        required = set(tuple(e) for e in expert_knowledge.required_edges)
        forbidden = set(tuple(e) for e in expert_knowledge.forbidden_edges)
        unknown = sorted({str(v) for e in required | forbidden for v in e if v not in nodes})
        if unknown:
            raise ValueError(f"ExhaustiveSearch: expert_knowledge names variables that are not in the data: {unknown}")
        if not nx.is_directed_acyclic_graph(nx.DiGraph(required)):
            raise ValueError("required_edges create a cycle in start_dag. Please modify either required_edges or start_dag.")
        index = {v: i for i, v in enumerate(nodes)}
        as_index = lambda edges: [(index[u], index[v]) for u, v in edges]
        families = enumerate_families(n, max_indegree, as_index(forbidden), as_index(required))
        return nodes, families, self._scores(nodes, families)

    def estimate(self, max_indegree=None, expert_knowledge=None, show_progress=True):
        """A CPD-less DiscreteBayesianNetwork of the highest score over all the data's variables, among the DAGs
        whose nodes have at most `max_indegree` parents and that hold every required and no forbidden edge.
        `show_progress` is accepted and ignored."""
        from ..models import DiscreteBayesianNetwork
        from ._xs import XsPlan

        nodes, families, scores = self._scored_families(max_indegree, expert_knowledge)
        n = len(nodes)
        res = XsPlan(n).run([v for v, _ in families], [m for _, m in families], scores)
        self.n_families, self.best_score = len(families), res["score"]
        if res["infeasible"]:
            raise ValueError("ExhaustiveSearch: no DAG meets max_indegree and the required edges")
        model = DiscreteBayesianNetwork()
        model.add_nodes_from(nodes)
        model.add_edges_from((nodes[u], nodes[v]) for v, mask in enumerate(res["parents"]) for u in range(n) if mask >> u & 1)
        return model

    def edge_posteriors(self, max_indegree=None, expert_knowledge=None):
        """The exact posterior probability of every edge, as a DataFrame indexed by parent with the children as
        columns, summed over all DAGs that `estimate` would search (pgm_xs_posterior: the same lattice with a
        log-sum-exp for the maximum, after Koivisto and Sood).  Sets `log_marginal`, the log of the data's marginal
        likelihood summed over orders and DAGs, and `n_families`.  The diagonal and every forbidden edge are exactly
        0; a required edge is 1 up to rounding.

        The prior is order-modular: uniform over the linear orders of the variables, times whatever prior the family
        scores carry.  A DAG consistent with more orders therefore weighs more than under a uniform prior over DAGs;
        that is the price of an exact sum and is not corrected.  The numbers are posteriors only when a family's score
        is a log marginal likelihood plus a log prior (K2, BDeu, BDs); any StructureScore is accepted, and BIC or AIC
        give the approximation that their penalty is.  The checks and errors are `estimate`'s."""
        import pandas as pd

        from ._xs import XsPlan

        nodes, families, scores = self._scored_families(max_indegree, expert_knowledge)
        res = XsPlan(len(nodes)).posterior([v for v, _ in families], [m for _, m in families], scores)
        self.n_families, self.log_marginal = len(families), float(res["log_z"][0])
        if res["infeasible"]:
            raise ValueError("ExhaustiveSearch: no DAG meets max_indegree and the required edges")
        return pd.DataFrame(res["edge_post"], index=nodes, columns=nodes)

    # ------------------------------------------------------------------ every DAG, on the host (small n)
    def all_dags(self, nodes=None):
        """A generator of every DAG over `nodes` (default: the data's variables, sorted) as nx.DiGraph, by ascending
        number of edges, the empty graph first, as the reference's all_dags yields them.  For six nodes at most."""
        names = sorted(self._nodes()) if nodes is None else list(nodes)
        if len(names) > 6:
            logger.warning("all_dags over %d nodes walks up to 2^%d candidate graphs; estimate() finds the best DAG "
                           "without them", len(names), len(names) * (len(names) - 1))
        for masks in dag_masks(len(names)):
            yield _graph(names, masks)

    def all_scores(self):
        """[(score, dag)] of every DAG, lowest score first (the reference's all_scores): a score is the sum of the
        DAG's family scores, all of which come from one batched scoring, plus the scorer's structure prior."""
        names = self._nodes()
        families = enumerate_families(len(names))
        table = dict(zip(families, self._scores(names, families, arc_prior=False)))
        scored = []
        for masks in dag_masks(len(names)):
            dag, total = _graph(names, masks), 0
            for family in enumerate(masks):
                total += table[family]
            scored.append((total + self.scoring_method.structure_prior(dag), dag))
        scored.sort(key=itemgetter(0))
        return scored


def _graph(names, masks):
    graph = nx.DiGraph()
    graph.add_nodes_from(names)
    graph.add_edges_from((names[u], names[v]) for v, mask in enumerate(masks) for u in range(len(names)) if mask >> u & 1)
    return graph


def _acyclic(masks):
    """Peel the nodes whose parents are all gone; a cycle is what cannot be peeled."""
    left = (1 << len(masks)) - 1
    while left:
        free = sum(1 << v for v, mask in enumerate(masks) if left >> v & 1 and not mask & left)
        if not free:
            return False
        left &= ~free
    return True


def dag_masks(m):
    """Every DAG over nodes 0 .. m - 1 as a tuple of parent masks, by ascending number of edges: for each edge count
    the nodes take their parent sets (enumerate_families' order) one after the other out of that budget."""
    options = [[mask for v, mask in enumerate_families(m) if v == node] for node in range(m)]

    def assign(node, budget, chosen):
        if node == m:
            if budget == 0 and _acyclic(chosen):
                yield tuple(chosen)
            return
        for mask in options[node]:
            arcs = bin(mask).count("1")
            if arcs <= budget <= arcs + (m - 1 - node) * (m - 1):
                yield from assign(node + 1, budget - arcs, chosen + [mask])

    for edges in range(m * (m - 1) // 2 + 1):
        yield from assign(0, edges, [])
