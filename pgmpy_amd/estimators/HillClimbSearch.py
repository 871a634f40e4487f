"""HillClimbSearch (mirror of pgmpy/estimators/HillClimbSearch.py:30-292) with the scores of a step
computed in one batch.

The reference evaluates each candidate operation with two to four cached `local_score` calls, one pandas
groupby per cache miss.  Here every iteration first enumerates its legal operations, collects the
families they need that are not in the score cache, gets all of them with ONE `local_scores` call (one
count launch and one score launch, estimators/StructureScore.py) and then evaluates the deltas from the
cache.  A score does not depend on the order of the parents, so the cache key is
(variable, tuple(sorted(parents))).

`hill_climb` is the loop itself; it takes its scorer as any object with `local_scores`,
`structure_prior_ratio` and `structure_prior`, so it runs without a device under a host scorer.

Deviation: among operations of equal score delta the reference takes whichever its `max`
over a set in hash order meets first; here the first in the order kind "+", "-", "flip", then X's data
column, then Y's data column wins, and deltas that differ by rounding only count as equal
(TIE_TOLERANCE), so results are reproducible and the same under a device and a host scorer.
"""
from collections import deque

import networkx as nx

from .base import BaseEstimator
from .StructureScore import get_scoring_method


class ExpertKnowledge:
    """Required and forbidden edges (pgmpy/estimators/ExpertKnowledge.py:87-111).  Temporal order and a
    limited search space are not built."""

    def __init__(self, forbidden_edges=None, required_edges=None, temporal_order=None, search_space=None, **kwargs):
        if temporal_order is not None or search_space is not None:
            raise NotImplementedError("ExpertKnowledge: temporal_order and search_space are not built")
        self.forbidden_edges = self._validate_edges(forbidden_edges) if forbidden_edges is not None else set()
        self.required_edges = self._validate_edges(required_edges) if required_edges is not None else set()
        self.search_space = set()
        self.temporal_order = [[]]

    @staticmethod
    def _validate_edges(edge_list):
        if not hasattr(edge_list, "__iter__"):
            raise TypeError(f"Expected iterator type for edge information. Got {type(edge_list)} instead.")
        return set(tuple(e) for e in edge_list)


def _family(variable, parents):
    return (variable, tuple(sorted(parents)))


def legal_operations(model, variables, tabu_list, max_indegree, forbidden_edges, required_edges):
    """[(operation, [(sign, family), ...])] of every legal (= not tabu) single-edge change of `model`
    (HillClimbSearch.py:63-138), in the documented order: "+", "-", "flip", then X's column, then Y's.
    The score delta of an operation is the signed sum of its families' scores, in the listed order."""
    tabu = set(tabu_list)
    order = {v: i for i, v in enumerate(variables)}
    parents = {v: list(model.predecessors(v)) for v in variables}
    edges = sorted(model.edges(), key=lambda e: (order[e[0]], order[e[1]]))
    ops = []
    for X in variables:
        for Y in variables:
            if X == Y or model.has_edge(X, Y) or model.has_edge(Y, X):
                continue
            if nx.has_path(model, Y, X):  # adding (X, Y) would close a cycle
                continue
            operation = ("+", (X, Y))
            if operation in tabu or (X, Y) in forbidden_edges:
                continue
            new_parents = parents[Y] + [X]
            if len(new_parents) <= max_indegree:
                ops.append((operation, [(1, _family(Y, new_parents)), (-1, _family(Y, parents[Y]))]))
    for X, Y in edges:
        operation = ("-", (X, Y))
        if operation not in tabu and (X, Y) not in required_edges:
            new_parents = [v for v in parents[Y] if v != X]
            ops.append((operation, [(1, _family(Y, new_parents)), (-1, _family(Y, parents[Y]))]))
    for X, Y in edges:
        # flipping (X, Y) closes a cycle when another path leads from X to Y
        model.remove_edge(X, Y)
        other_path = nx.has_path(model, X, Y)
        model.add_edge(X, Y)
        if other_path:
            continue
        operation = ("flip", (X, Y))
        if (operation in tabu or ("flip", (Y, X)) in tabu or (X, Y) in required_edges or (Y, X) in forbidden_edges):
            continue
        new_X_parents = parents[X] + [Y]
        new_Y_parents = [v for v in parents[Y] if v != X]
        if len(new_X_parents) <= max_indegree:
            ops.append((operation, [(1, _family(X, new_X_parents)), (1, _family(Y, new_Y_parents)),
                                    (-1, _family(X, parents[X])), (-1, _family(Y, parents[Y]))]))
    return ops


def operation_delta(op, cache, scorer):
    """The score change of one entry of legal_operations under cached family scores."""
    operation, terms = op
    delta = None
    for sign, fam in terms:
        s = cache[fam] if sign > 0 else -cache[fam]
        delta = s if delta is None else delta + s
    return delta + scorer.structure_prior_ratio(operation[0])


# Two deltas closer than this fraction of the family scores they are formed from count as equal.  Score-
# equivalent scores (BDeu, BDs, LL, BIC, AIC) give "+ (X, Y)" and "+ (Y, X)" the same delta up to the
# rounding of four sums of thousands of terms; which of the two comes out larger depends on the scorer
# (device or host, the reduction order).  With the tolerance the choice among such operations is the
# documented order's, whatever the scorer: 2^-40 is ~10^4 times the relative error of a score and far
# below any difference that data makes.
TIE_TOLERANCE = 2.0 ** -40


def operation_scale(op, cache):
    """Sum of the magnitudes of the family scores of one entry of legal_operations."""
    return sum(abs(cache[fam]) for _, fam in op[1])


def hill_climb(variables, scorer, start_dag=None, tabu_length=100, max_indegree=None, required_edges=(),
               forbidden_edges=(), epsilon=1e-4, max_iter=int(1e6), use_cache=True, cache=None):
    """The search (HillClimbSearch.py:214-292) over a networkx.DiGraph; returns (graph, iterations that
    applied an operation, the tabu list at the end).  `cache` (a dict, optional) receives every family
    score."""
    variables = list(variables)
    required_edges, forbidden_edges = set(required_edges), set(forbidden_edges)
    model = nx.DiGraph()
    model.add_nodes_from(variables)
    if start_dag is not None:
        model.add_edges_from(start_dag.edges())
    model.add_edges_from(required_edges)
    if set(model.nodes()) != set(variables) or not nx.is_directed_acyclic_graph(model):
        raise ValueError("required_edges create a cycle in start_dag. Please modify either required_edges or start_dag.")
    model.remove_edges_from(forbidden_edges)
    if max_indegree is None:
        max_indegree = float("inf")
    tabu_list = deque(maxlen=tabu_length)
    cache = {} if cache is None else cache
    steps = 0
    for _ in range(int(max_iter)):
        if not use_cache:
            cache.clear()
        ops = legal_operations(model, variables, tabu_list, max_indegree, forbidden_edges, required_edges)
        need = []
        for _, terms in ops:
            for _, fam in terms:
                if fam not in cache:
                    cache[fam] = None
                    need.append(fam)
        if need:
            for fam, s in zip(need, scorer.local_scores([(v, list(ps)) for v, ps in need])):
                cache[fam] = s
        best_operation, best_score_delta, best_scale = None, None, 0.0
        for op in ops:
            delta, scale = operation_delta(op, cache, scorer), operation_scale(op, cache)
            # ties (within TIE_TOLERANCE): the first in the order wins
            if best_score_delta is None or delta > best_score_delta + TIE_TOLERANCE * max(scale, best_scale):
                best_operation, best_score_delta, best_scale = op[0], delta, scale
        if best_operation is None or best_score_delta < epsilon:
            break
        kind, (X, Y) = best_operation
        if kind == "+":
            model.add_edge(X, Y)
            tabu_list.append(("-", (X, Y)))
        elif kind == "-":
            model.remove_edge(X, Y)
            tabu_list.append(("+", (X, Y)))
        else:
            model.remove_edge(X, Y)
            model.add_edge(Y, X)
            tabu_list.append(best_operation)
        steps += 1
    return model, steps, list(tabu_list)


class HillClimbSearch(BaseEstimator):
    def __init__(self, data, use_cache=True, **kwargs):
        self.use_cache = use_cache
        self.n_iterations = None  # operations applied by the last estimate()
        super(HillClimbSearch, self).__init__(data, **kwargs)

    def estimate(self, scoring_method=None, start_dag=None, tabu_length=100, max_indegree=None, expert_knowledge=None,
                 epsilon=1e-4, max_iter=int(1e6), show_progress=True):
        """A CPD-less DiscreteBayesianNetwork over all the data's variables at a local score maximum.
        `show_progress` is accepted and ignored."""
        from ..models import DiscreteBayesianNetwork

        score, _ = get_scoring_method(scoring_method, self.data, self.use_cache)
        if start_dag is not None and (not isinstance(start_dag, nx.DiGraph)
                                      or set(start_dag.nodes()) != set(self.variables)):
            raise ValueError("'start_dag' should be a DAG with the same variables as the data set, or 'None'.")
        if expert_knowledge is None:
            expert_knowledge = ExpertKnowledge()
        if getattr(expert_knowledge, "search_space", None) or any(getattr(expert_knowledge, "temporal_order", None) or []):
            raise NotImplementedError("ExpertKnowledge: temporal_order and search_space are not built")
        graph, self.n_iterations, _ = hill_climb(
            self.variables, score, start_dag=start_dag, tabu_length=tabu_length, max_indegree=max_indegree,
            required_edges=set(tuple(e) for e in expert_knowledge.required_edges),
            forbidden_edges=set(tuple(e) for e in expert_knowledge.forbidden_edges), epsilon=epsilon, max_iter=max_iter,
            use_cache=self.use_cache)
        model = DiscreteBayesianNetwork()
        model.add_nodes_from(self.variables)
        model.add_edges_from(graph.edges())
        return model
