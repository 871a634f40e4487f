"""NaiveBayes (mirror of pgmpy/models/NaiveBayes.py:5-222): a DiscreteBayesianNetwork whose only edges lead
from the dependent variable to the features.  `fit` and `predict` are the base class's: the counting,
the normalisation and the row queries run on the device kernels (pgm_fit_count, pgm_fit_finish, the fused
row plan).  TreeSearch.estimate("tan", ...) extends this structure by a tree over the features.
"""
from .DiscreteBayesianNetwork import DiscreteBayesianNetwork


class IndependenceAssertion:
    """(event1 _|_ event2 | event3), each a frozenset of variables (pgmpy/independencies)."""

    def __init__(self, event1, event2, event3=()):
        as_set = lambda e: frozenset([e] if isinstance(e, str) or not hasattr(e, "__iter__") else e)
        self.event1, self.event2, self.event3 = as_set(event1), as_set(event2), as_set(event3)

    def _key(self):
        return (frozenset([self.event1, self.event2]), self.event3)

    def __eq__(self, other):
        return isinstance(other, IndependenceAssertion) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        text = lambda e: ", ".join(sorted(str(v) for v in e))
        given = f" | {text(self.event3)}" if self.event3 else ""
        return f"({text(self.event1)} ⟂ {text(self.event2)}{given})"


class Independencies:
    """A set of independence assertions: what local_independencies returns."""

    def __init__(self, *assertions):
        self.independencies = []
        self.add_assertions(*assertions)

    def add_assertions(self, *assertions):
        for a in assertions:
            self.independencies.append(a if isinstance(a, IndependenceAssertion) else IndependenceAssertion(*a))

    def get_assertions(self):
        return self.independencies

    def __eq__(self, other):
        return isinstance(other, Independencies) and set(self.independencies) == set(other.independencies)

    def __repr__(self):
        return "\n".join(repr(a) for a in self.independencies)


class NaiveBayes(DiscreteBayesianNetwork):
    def __init__(self, feature_vars=None, dependent_var=None):
        self.dependent = dependent_var
        self.features = set(feature_vars) if feature_vars is not None else set()
        if (feature_vars is not None) and (dependent_var is not None):
            ebunch = [(self.dependent, feature) for feature in self.features]
        else:
            ebunch = []
        super(NaiveBayes, self).__init__(ebunch=ebunch)

    def add_edge(self, u, v, *kwargs):
        """An edge from the dependent variable `u` to the feature `v`; ValueError for any other `u` once
        the dependent variable is known (NaiveBayes.py:64-70)."""
        if self.dependent and u != self.dependent:
            raise ValueError(f"Model can only have edges outgoing from: {self.dependent}")
        self.dependent = u
        self.features.add(v)
        super(NaiveBayes, self).add_edge(u, v, *kwargs)

    def add_edges_from(self, ebunch):
        for u, v in ebunch:
            self.add_edge(u, v)

    def _get_ancestors_of(self, obs_nodes_list):
        if not obs_nodes_list:
            return set()
        return set(obs_nodes_list) | set(self.dependent)

    def active_trail_nodes(self, start, observed=None):
        """The nodes reachable from `start` by an active trail: `start` alone once the dependent variable
        is observed, else every node that is not observed (NaiveBayes.py:139-142)."""
        if observed and self.dependent in observed:
            return set(start)
        else:
            return set(self.nodes()) - set(observed if observed else [])

    def local_independencies(self, variables):
        """Each feature is independent of the other features given the dependent variable."""
        independencies = Independencies()
        for variable in [variables] if isinstance(variables, str) else variables:
            if variable != self.dependent:
                independencies.add_assertions([variable, list(set(self.features) - set(variable)), self.dependent])
        return independencies

    def fit(self, data, parent_node=None, estimator=None):
        """The CPDs from `data` on the device; every column that is not `parent_node` (default: the
        dependent variable known so far) becomes a feature (NaiveBayes.py:210-222)."""
        if not parent_node:
            if not self.dependent:
                raise ValueError("parent node must be specified for the model")
            else:
                parent_node = self.dependent
        if parent_node not in data.columns:
            raise ValueError(f"Dependent variable: {parent_node} is not present in the data")
        for child_node in data.columns:
            if child_node != parent_node:
                self.add_edge(parent_node, child_node)
        super(NaiveBayes, self).fit(data, estimator)
