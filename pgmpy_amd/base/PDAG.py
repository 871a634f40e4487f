"""PDAG: a partially directed acyclic graph, the output of PC before and after Meek's rules (the interface
of pgmpy/base/PDAG.py).  Host-only code over networkx.DiGraph: an undirected edge X - Y is stored as the two
arcs X -> Y and Y -> X, and `directed_edges` / `undirected_edges` say which is which.

Orientation follows C. Meek, "Causal inference and causal explanation with background knowledge" (UAI
1995), rules R1-R4 as published; the extension to a DAG follows D. Dor and M. Tarsi, "A simple algorithm to
construct a consistent extension of a partially oriented graph" (1992).  Wherever an order matters (which of
two conflicting orientations wins, which DAG of the class comes out) nodes are taken in the order they
were added: `nodes` first, then the edges as given.
"""
from itertools import combinations

import networkx as nx


class PDAG(nx.DiGraph):
    def __init__(self, directed_ebunch=(), undirected_ebunch=(), nodes=()):
        super(PDAG, self).__init__()
        directed = [tuple(e) for e in directed_ebunch]
        undirected = [tuple(e) for e in undirected_ebunch]
        self.directed_edges, self.undirected_edges = set(directed), set(undirected)
        self.add_nodes_from(nodes)
        self.add_edges_from(directed)
        self.add_edges_from(undirected)
        self.add_edges_from((v, u) for u, v in undirected)

    # ------------------------------------------------------------------ queries
    def copy(self):
        rank = self._rank()
        key = lambda e: (rank[e[0]], rank[e[1]])  # noqa: E731
        return PDAG(sorted(self.directed_edges, key=key), sorted(self.undirected_edges, key=key), nodes=self.nodes())

    def _rank(self):
        return {v: i for i, v in enumerate(self.nodes())}

    def has_directed_edge(self, u, v):
        return (u, v) in self.directed_edges

    def has_undirected_edge(self, u, v):
        return (u, v) in self.undirected_edges or (v, u) in self.undirected_edges

    def directed_parents(self, node):
        return {u for u in self.predecessors(node) if (u, node) in self.directed_edges}

    def directed_children(self, node):
        return {v for v in self.successors(node) if (node, v) in self.directed_edges}

    def undirected_neighbors(self, node):
        return {v for v in self.successors(node) if self.has_edge(v, node)}

    def all_neighbors(self, node):
        return set(self.successors(node)) | set(self.predecessors(node))

    def is_adjacent(self, u, v):
        return self.has_edge(u, v) or self.has_edge(v, u)

    def __eq__(self, other):
        if not isinstance(other, PDAG):
            return False
        return (set(self.nodes()) == set(other.nodes()) and self.directed_edges == other.directed_edges
                and {frozenset(e) for e in self.undirected_edges} == {frozenset(e) for e in other.undirected_edges})

    __hash__ = nx.DiGraph.__hash__

    # ------------------------------------------------------------------ orientation
    def orient_undirected_edge(self, u, v, inplace=False):
        """Turn the undirected edge u - v into u -> v."""
        pdag = self if inplace else self.copy()
        if not pdag.has_undirected_edge(u, v):
            raise ValueError(f"Undirected Edge {u} - {v} not present in the PDAG.")
        pdag.undirected_edges -= {(u, v), (v, u)}
        pdag.remove_edge(v, u)
        pdag.directed_edges.add((u, v))
        return None if inplace else pdag

    def _meek_orients(self, a, b, apply_r4):
        """Whether one of Meek's rules orients the undirected edge a - b as a -> b."""
        into_a, into_b = self.directed_parents(a), self.directed_parents(b)
        # R1: c -> a - b with c, b not adjacent (else b -> a would make the new collider c -> a <- b)
        if any(not self.is_adjacent(c, b) for c in into_a):
            return True
        # R2: a -> c -> b (else b -> a would close a directed cycle)
        if self.directed_children(a) & into_b:
            return True
        # R3: a - c -> b and a - d -> b with c, d not adjacent
        spouses = self.undirected_neighbors(a) & into_b
        if any(not self.is_adjacent(c, d) for c, d in combinations(spouses, 2)):
            return True
        # R4: a - d -> c -> b with a, c adjacent and d, b not adjacent
        if apply_r4:
            for c in into_b & self.all_neighbors(a):
                if any(not self.is_adjacent(d, b) for d in self.directed_parents(c) & self.undirected_neighbors(a)):
                    return True
        return False

    def apply_meeks_rules(self, apply_r4=False, inplace=False):
        """Orient undirected edges by Meek's rules R1-R3 (and R4 with apply_r4) until none applies: a pass
        asks for every undirected edge, ends in node order, whether a rule orients it either way."""
        pdag = self if inplace else self.copy()
        rank = pdag._rank()
        changed = True
        while changed:
            changed = False
            pending = sorted((tuple(sorted(e, key=rank.__getitem__)) for e in pdag.undirected_edges),
                             key=lambda e: (rank[e[0]], rank[e[1]]))
            for a, b in pending:
                for u, v in ((a, b), (b, a)):
                    if pdag._meek_orients(u, v, apply_r4):
                        pdag.orient_undirected_edge(u, v, inplace=True)
                        changed = True
                        break
        return None if inplace else pdag

    # ------------------------------------------------------------------ extension
    def to_dag(self):
        """One DAG of the class the PDAG stands for, as a CPD-less DiscreteBayesianNetwork, so `fit`
        follows directly.  Dor & Tarsi: while nodes are left, take a node x that is a sink of the directed
        part and whose undirected neighbours are adjacent to every other node adjacent to x; point its
        undirected edges at x; remove x.  When no node qualifies the PDAG has no consistent extension: the
        undirected edges left are then directed from the earlier node to the later one in node order,
        which cannot close a cycle among themselves; one that would close a cycle with the directed part
        is turned round."""
        from ..models import DiscreteBayesianNetwork

        rank = self._rank()
        dag = nx.DiGraph()
        dag.add_nodes_from(self.nodes())
        dag.add_edges_from(self.directed_edges)
        left = set(self.nodes())
        out_of = {v: self.directed_children(v) for v in left}
        und = {v: self.undirected_neighbors(v) for v in left}
        near = {v: self.all_neighbors(v) for v in left}

        def removable(x):
            if out_of[x] & left:
                return False
            around = near[x] & left
            return all(w == y or w in near[y] for y in und[x] & left for w in around)

        while left:
            x = next((v for v in self.nodes() if v in left and removable(v)), None)
            if x is None:
                rest = sorted(((u, v) for u in left for v in und[u] & left if rank[u] < rank[v]),
                              key=lambda e: (rank[e[0]], rank[e[1]]))
                for u, v in rest:
                    if nx.has_path(dag, v, u):
                        u, v = v, u
                    dag.add_edge(u, v)
                break
            dag.add_edges_from((y, x) for y in und[x] & left)
            left.discard(x)
        model = DiscreteBayesianNetwork()
        model.add_nodes_from(dag.nodes())
        model.add_edges_from(dag.edges())
        return model
