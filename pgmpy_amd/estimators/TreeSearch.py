"""TreeSearch (mirror of pgmpy/estimators/TreeSearch.py:21-402): Chow-Liu trees and tree-augmented naive
Bayes (TAN), with the edge weights of every pair of columns from one pairwise-count launch.

The reference calls a scikit-learn score once per pair of columns (and per class value for TAN).  Here the
named weightings (`mutual_info`, `normalized_mutual_info`, `adjusted_mutual_info`) come from the device:
BaseEstimator.pairwise_mutual_information counts the tables of all pairs in one int8 MFMA launch
(pgm_pair_count), reduces them to mutual information, entropies and, for the adjusted kind, expected mutual
information in one or two more, and downloads one array.  A callable `edge_weights_fn` is applied to the
frame's columns pair by pair on the host, as the reference does: the slow path.

`tree_search` is the tree logic itself; it takes its scorer as any object with
`pairwise_mutual_information(variables, given, kind)`, so it runs without a device under a host scorer.

Deviations: `estimate` returns a CPD-less DiscreteBayesianNetwork with EVERY data column as a
node (the reference drops a column whose weights are all exactly 0); a row with a missing cell is left out
per pair (the reference's scikit-learn calls raise); every column is discrete whatever its dtype; `n_jobs`
and `show_progress` are accepted and ignored; the strata of a TAN weight are added in state order.
"""
from itertools import combinations

import networkx as nx
import numpy as np
import pandas as pd

from ._pairs import KINDS, weight_matrix
from .base import BaseEstimator


def _check_weights_fn(edge_weights_fn):
    if edge_weights_fn not in KINDS and not callable(edge_weights_fn):
        raise ValueError(
            f"edge_weights_fn should either be 'mutual_info', 'adjusted_mutual_info', "
            f"'normalized_mutual_info'or a function of form fun(array, array). Got: f{edge_weights_fn}")


def host_weights(data, edge_weights_fn, class_node=None):
    """The weight matrix of a callable `edge_weights_fn(column, column)`, pair by pair on the host
    (TreeSearch.py:252-266, 329-356)."""
    columns = list(data.columns)
    if class_node is None:
        vals = [edge_weights_fn(data.loc[:, u], data.loc[:, v]) for u, v in combinations(columns, 2)]
    else:
        cond_marginal = data.loc[:, class_node].value_counts() / data.shape[0]
        vals = []
        for u, v in combinations(columns, 2):
            w = 0
            for index, marg_prob in cond_marginal.items():
                subset = data[data.loc[:, class_node] == index]
                w += marg_prob * edge_weights_fn(subset.loc[:, u], subset.loc[:, v])
            vals.append(w)
    return weight_matrix(len(columns), vals)


def create_tree_and_dag(weights, columns, root_node):
    """The maximum spanning tree of the weight matrix (built in the order of `columns`), directed away
    from `root_node`; every column is a node of the result (TreeSearch.py:359-402)."""
    from ..models import DiscreteBayesianNetwork

    columns = list(columns)
    T = nx.maximum_spanning_tree(
        nx.from_pandas_adjacency(pd.DataFrame(weights, index=columns, columns=columns), create_using=nx.Graph))
    D = nx.bfs_tree(T, root_node)
    model = DiscreteBayesianNetwork()
    model.add_nodes_from(columns)
    model.add_edges_from(D.edges())
    return model


def tree_search(scorer, columns, root_node=None, estimator_type="chow-liu", class_node=None,
                edge_weights_fn="mutual_info"):
    """(model, root_node) of TreeSearch.estimate (TreeSearch.py:132-194) under `scorer`, any object with
    pairwise_mutual_information(variables, given, kind) that returns the symmetric weight matrix."""
    columns = list(columns)
    if estimator_type not in {"chow-liu", "tan"}:
        raise ValueError(f"Invalid estimator_type. Expected either chow-liu or tan. Got: {estimator_type}")
    if estimator_type == "tan" and class_node is None:
        raise ValueError("class_node argument must be specified for estimator_type='tan'")
    if estimator_type == "tan" and class_node not in columns:
        raise ValueError(f"Class node: {class_node} not found in data columns")
    _check_weights_fn(edge_weights_fn)

    weights = None
    if root_node is None:
        weights = scorer.pairwise_mutual_information(columns, None, edge_weights_fn)
        sum_weights = weights.sum(axis=0)
        root_node = columns[np.argsort(sum_weights)[::-1][0]]
    if estimator_type == "chow-liu":
        if weights is None:
            weights = scorer.pairwise_mutual_information(columns, None, edge_weights_fn)
        return create_tree_and_dag(weights, columns, root_node), root_node

    weights = scorer.pairwise_mutual_information(columns, class_node, edge_weights_fn)
    if root_node == class_node:
        raise ValueError(f"Root node: {root_node} and class node: {class_node} are identical")
    k = columns.index(class_node)
    weights = np.delete(np.delete(weights, k, axis=0), k, axis=1)
    reduced = columns[:k] + columns[k + 1:]
    model = create_tree_and_dag(weights, reduced, root_node)
    model.add_edges_from([(class_node, node) for node in reduced])
    return model, root_node


class _Scorer:
    """The device scorer of a frame for the named weightings; a callable goes pair by pair on the host."""

    def __init__(self, data, estimator=None):
        self.data = data
        self.estimator = estimator

    def pairwise_mutual_information(self, variables, given, kind):
        if callable(kind):
            return host_weights(self.data.loc[:, list(variables)], kind, given)
        if self.estimator is None:
            self.estimator = BaseEstimator(self.data)
        return self.estimator.pairwise_mutual_information(list(variables), given, kind)


class TreeSearch(BaseEstimator):
    def __init__(self, data, root_node=None, n_jobs=-1, **kwargs):
        if root_node is not None and root_node not in data.columns:
            raise ValueError(f"Root node: {root_node} not found in data columns.")
        self.root_node = root_node
        self.n_jobs = n_jobs  # accepted and ignored: the pairs are one launch
        super(TreeSearch, self).__init__(data, **kwargs)

    def estimate(self, estimator_type="chow-liu", class_node=None, edge_weights_fn="mutual_info", show_progress=True):
        """The Chow-Liu tree (`chow-liu`) or the tree-augmented naive Bayes structure with edges from
        `class_node` to every other column (`tan`) as a DiscreteBayesianNetwork without CPDs.  Without a
        root node the column with the largest sum of (unconditional) edge weights becomes the root and is
        kept in `self.root_node`, as in the reference."""
        model, self.root_node = tree_search(_Scorer(self.data, self), list(self.data.columns), self.root_node,
                                            estimator_type, class_node, edge_weights_fn)
        return model

    @staticmethod
    def _get_weights(data, edge_weights_fn="mutual_info", n_jobs=-1, show_progress=True):
        """The symmetric matrix of edge weights of every pair of columns (TreeSearch.py:196-266)."""
        _check_weights_fn(edge_weights_fn)
        return _Scorer(data).pairwise_mutual_information(list(data.columns), None, edge_weights_fn)

    @staticmethod
    def _get_conditional_weights(data, class_node, edge_weights_fn="mutual_info", n_jobs=-1, show_progress=True):
        """The weights given the class: sum over its states c of p(c) w(u, v | c) (TreeSearch.py:268-356)."""
        _check_weights_fn(edge_weights_fn)
        return _Scorer(data).pairwise_mutual_information(list(data.columns), class_node, edge_weights_fn)

    @staticmethod
    def _create_tree_and_dag(weights, columns, root_node):
        return create_tree_and_dag(weights, columns, root_node)
