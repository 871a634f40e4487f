"""PC: constraint-based structure learning (mirror of pgmpy/estimators/PC.py:23-371 and
BaseConstraintEstimator.py:57-356) with the independence tests of a level asked for in batches.

The reference runs one CI test per call: a pandas groupby and one scipy.stats.chi2_contingency per
stratum, thousands of tests per level, fanned out over joblib.  Here every level enumerates the candidate
separating sets of all its remaining edges and hands them to the tester in rounds of up to
MAX_TESTS_PER_ROUND tests: one count launch and one CI launch per round (estimators/CITests.py,
pgm_fit_citest), one download of the p-values.  On continuous data, `ci_test=pearsonr` (the function) or
a `tester=GaussCITester(...)` hands a level to the partial-correlation kernel: no counting, one launch per
level on the moment matrix (pgm_lgs_pcorr).

`pc_skeleton` is the loop itself; it takes its tester as any object with
`independent(triples, significance_level)`, so it runs without a device under a host tester.

Deviations: the reference walks the neighbours of an edge's ends as Python sets, in hash
order, so which of several separating sets it records (and the edge order of its "orig" and "stable"
variants, which both remove edges as they go) changes with PYTHONHASHSEED.  Here edges and neighbours are
walked in data-column order, so results are reproducible; "stable" and "parallel" are one algorithm
(neighbour sets frozen per level, every edge with an independent candidate removed, the first
independent candidate in enumeration order recorded), "orig" removes edges as it goes.  Independence
assertions instead of data, temporal order and a search space are not built; expert knowledge needs
enforce_expert_knowledge=True.
"""
from itertools import chain, combinations

import networkx as nx

from ..base import PDAG
from .base import BaseEstimator
from .CITests import BUILTIN_LAMBDA, CITester, GaussCITester, get_callable_ci_test, lambda_value, pearsonr
from .HillClimbSearch import ExpertKnowledge

# Most tests one round hands to the tester.  A level with more runs in several rounds; an edge separated in
# an earlier round drops its later candidates.  (The tester splits a round further by count bins.)
MAX_TESTS_PER_ROUND = 1 << 16

VARIANTS = ("orig", "stable", "parallel")


def potential_sepsets(u, v, adj, order, size):
    """The candidate separating sets of the edge u - v: the `size`-subsets of adj(u) - {v}, then those of
    adj(v) - {u} not met yet, neighbours in column order.  (The reference tests a set that both ends share
    twice, the empty set of level 0 included; the first independent candidate is the same.)"""
    nu = sorted((w for w in adj[u] if w != v), key=order.__getitem__)
    nv = sorted((w for w in adj[v] if w != u), key=order.__getitem__)
    seen = set()
    for Z in chain(combinations(nu, size), combinations(nv, size)):
        if Z not in seen:
            seen.add(Z)
            yield Z


def pc_skeleton(variables, tester, variant="stable", significance_level=0.01, max_cond_vars=5, forbidden_edges=(),
                required_edges=(), max_tests=None):
    """(skeleton nx.Graph, {frozenset((u, v)): separating set tuple}) by the first phase of PC
    (BaseConstraintEstimator.py:172-299).  forbidden_edges are removed before level 0; required_edges
    are never tested."""
    if variant not in VARIANTS:
        raise ValueError(f"variant must be one of: orig, stable, or parallel. Got: {variant}")
    variables = list(variables)
    order = {v: i for i, v in enumerate(variables)}
    max_tests = MAX_TESTS_PER_ROUND if max_tests is None else int(max_tests)
    graph = nx.Graph()
    graph.add_nodes_from(variables)
    graph.add_edges_from(combinations(variables, 2))
    graph.remove_edges_from([e for e in forbidden_edges if graph.has_edge(*e)])
    required = {frozenset(e) for e in required_edges}
    separating_sets = {}
    size = 0
    while not all(graph.degree(v) < size for v in variables):
        edges = sorted(((u, v) if order[u] < order[v] else (v, u) for u, v in graph.edges()),
                       key=lambda e: (order[e[0]], order[e[1]]))
        edges = [e for e in edges if frozenset(e) not in required]
        if variant == "orig":
            for u, v in edges:
                cands = list(potential_sepsets(u, v, graph.adj, order, size))
                for start in range(0, len(cands), max_tests):
                    batch = cands[start:start + max_tests]
                    hits = tester.independent([(u, v, list(Z)) for Z in batch], significance_level)
                    first = next((Z for Z, hit in zip(batch, hits) if hit), None)
                    if first is not None:
                        separating_sets[frozenset((u, v))] = first
                        graph.remove_edge(u, v)
                        break
        else:
            adj = {v: list(graph.adj[v]) for v in variables}  # frozen for the level
            found = {}

            def level_tests():
                for u, v in edges:
                    for Z in potential_sepsets(u, v, adj, order, size):
                        if (u, v) in found:  # separated in an earlier round
                            break
                        yield u, v, Z

            def flush(batch):
                hits = tester.independent([(u, v, list(Z)) for u, v, Z in batch], significance_level)
                for (u, v, Z), hit in zip(batch, hits):
                    if hit and (u, v) not in found:
                        found[(u, v)] = Z

            batch = []
            for test in level_tests():
                batch.append(test)
                if len(batch) >= max_tests:
                    flush(batch)
                    batch = []
            if batch:
                flush(batch)
            for (u, v), Z in found.items():
                separating_sets[frozenset((u, v))] = Z
                graph.remove_edge(u, v)
        if size >= max_cond_vars:
            break
        size += 1
    return graph, separating_sets


class _BatchTester:
    """A CITester with its lambda bound."""

    def __init__(self, tester, lambda_):
        self.tester, self.lambda_ = tester, lambda_

    def independent(self, triples, significance_level):
        return self.tester.independent(triples, significance_level, self.lambda_)


class _GaussTester:
    """A GaussCITester with its intercept option bound: a level's partial correlations in one launch."""

    def __init__(self, tester, intercept):
        self.tester, self.intercept = tester, bool(intercept)

    def independent(self, triples, significance_level):
        return self.tester.independent(triples, significance_level, intercept=self.intercept)


class _CallableTester:
    """A user's test function, called one test at a time with the reference's keyword arguments."""

    def __init__(self, fn, data, kwargs):
        self.fn, self.data, self.kwargs = fn, data, kwargs

    def independent(self, triples, significance_level):
        return [bool(self.fn(X, Y, Z, data=self.data, independencies=None, significance_level=significance_level,
                             **self.kwargs)) for X, Y, Z in triples]


class PC(BaseEstimator):
    def __init__(self, data=None, independencies=None, tester=None, **kwargs):
        """`tester`: a CITester over the same variables to run the named tests with (one built over
        resident device codes by CITester.from_codes, say); by default one is built from `data`.  A
        GaussCITester runs partial correlations on continuous data; with one, `data` may be None (its
        variables are the tester's) and no state names are collected."""
        if independencies is not None:
            raise NotImplementedError("PC: independence assertions instead of data are not built")
        self._ci = tester
        if isinstance(tester, GaussCITester):
            self.data, self._encoded, self.state_names = data, None, {}
            self.variables = list(tester.variables)
            if data is not None and list(data.columns.values) != self.variables:
                raise ValueError("the tester's variables are not the data's columns")
            return
        if data is None:
            raise ValueError("PC needs data")
        super(PC, self).__init__(data, **kwargs)

    def _tester(self, ci_test, kwargs):
        if isinstance(self._ci, GaussCITester):
            if ci_test is not None and ci_test is not pearsonr:
                raise ValueError("a GaussCITester runs pearsonr: leave ci_test out or pass CITests.pearsonr")
            return _GaussTester(self._ci, kwargs.get("intercept", False))
        fn = get_callable_ci_test(ci_test, data=self.data)
        if fn is pearsonr:  # one launch per level instead of one call per test
            if getattr(self, "_gauss", None) is None:
                self._gauss = GaussCITester(self.data)
            return _GaussTester(self._gauss, kwargs.get("intercept", False))
        if fn not in BUILTIN_LAMBDA:
            return _CallableTester(fn, self.data, kwargs)
        lam = BUILTIN_LAMBDA[fn]
        if lam is None:  # power_divergence: its own default
            lam = kwargs.get("lambda_", "cressie-read")
        if self._ci is None:
            self._ci = CITester(self.data, state_names=self.state_names)
        return _BatchTester(self._ci, lambda_value(lam))

    @staticmethod
    def _knowledge(expert_knowledge, enforce_expert_knowledge):
        if expert_knowledge is None:
            expert_knowledge = ExpertKnowledge()
        if getattr(expert_knowledge, "search_space", None) or any(getattr(expert_knowledge, "temporal_order", None) or []):
            raise NotImplementedError("ExpertKnowledge: temporal_order and search_space are not built")
        forbidden = set(tuple(e) for e in expert_knowledge.forbidden_edges)
        required = set(tuple(e) for e in expert_knowledge.required_edges)
        if (forbidden or required) and not enforce_expert_knowledge:
            raise NotImplementedError("PC: expert knowledge is only built with enforce_expert_knowledge=True")
        return forbidden, required

    def build_skeleton(self, variant="stable", ci_test=None, significance_level=0.01, max_cond_vars=5,
                       expert_knowledge=None, enforce_expert_knowledge=False, n_jobs=-1, show_progress=True, **kwargs):
        """(skeleton, separating sets).  `n_jobs` and `show_progress` are accepted and ignored."""
        if variant not in VARIANTS:
            raise ValueError(f"variant must be one of: orig, stable, or parallel. Got: {variant}")
        forbidden, required = self._knowledge(expert_knowledge, enforce_expert_knowledge)
        tester = self._tester(ci_test, kwargs)
        return pc_skeleton(self.variables, tester, variant=variant, significance_level=significance_level,
                           max_cond_vars=max_cond_vars, forbidden_edges=forbidden, required_edges=required)

    @staticmethod
    def orient_colliders(skeleton, separating_sets):
        """The PDAG of the skeleton with its v-structures: for every node Z and every pair X, Y of its
        neighbours that are not adjacent, X -> Z <- Y when Z is not in the separating set recorded for
        (X, Y).  A pair without a recorded set orients nothing.  An edge that two v-structures claim in
        opposite directions stays undirected (the reference drops such an edge from the graph)."""
        nodes = list(skeleton.nodes())
        arrows = set()
        for Z in nodes:
            for X, Y in combinations(list(skeleton.neighbors(Z)), 2):
                sep = separating_sets.get(frozenset((X, Y)))
                if sep is not None and not skeleton.has_edge(X, Y) and Z not in sep:
                    arrows.update(((X, Z), (Y, Z)))
        directed, undirected = [], []
        for u, v in skeleton.edges():
            if ((u, v) in arrows) == ((v, u) in arrows):
                undirected.append((u, v))
            else:
                directed.append((u, v) if (u, v) in arrows else (v, u))
        return PDAG(directed, undirected, nodes=nodes)

    def estimate(self, variant="parallel", ci_test=None, return_type="pdag", significance_level=0.01, max_cond_vars=5,
                 expert_knowledge=None, enforce_expert_knowledge=False, n_jobs=-1, show_progress=True, **kwargs):
        """The skeleton and its separating sets (return_type "skeleton"), the PDAG after collider
        orientation and Meek's rules ("pdag", "cpdag"), or one DAG of its class as a CPD-less
        DiscreteBayesianNetwork ("dag")."""
        if variant not in VARIANTS:
            raise ValueError(f"variant must be one of: orig, stable, or parallel. Got: {variant}")
        if not isinstance(return_type, str) or return_type.lower() not in ("dag", "pdag", "cpdag", "skeleton"):
            raise ValueError(f"return_type must be one of: dag, pdag, cpdag, or skeleton. Got: {return_type}")
        skeleton, separating_sets = self.build_skeleton(
            variant=variant, ci_test=ci_test, significance_level=significance_level, max_cond_vars=max_cond_vars,
            expert_knowledge=expert_knowledge, enforce_expert_knowledge=enforce_expert_knowledge, **kwargs)
        if return_type.lower() == "skeleton":
            return skeleton, separating_sets
        pdag = self.orient_colliders(skeleton, separating_sets)
        pdag = pdag.apply_meeks_rules(apply_r4=False)
        if not enforce_expert_knowledge:
            # the reference's second pass after its (here empty) expert knowledge (PC.py:272-275)
            pdag = pdag.apply_meeks_rules(apply_r4=True)
        pdag.add_nodes_from(self.variables)
        if return_type.lower() in ("pdag", "cpdag"):
            return pdag
        return pdag.to_dag()
