"""The exact structure search on the device (pgm_xs_run, csrc/pgmxs.hip; ExhaustiveSearch) against the two numpy
references of tests/xs_cases.py."""
from functools import lru_cache

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import xs_cases as C

pytestmark = pytest.mark.gpu

L = 12  # log2 of the default tile

# (n, input, tiling).  Default tiling: a partial tile (1, 2, 5), a full sink tile (L), a full zeta tile and the first high
# sink bit (L + 1), one high zeta bit (L + 2), a trip of three (L + 4).  A full trip with a remainder behind it needs
# L + h + 2 nodes, so it runs under a small tiling: (10, (4, 3)) has trips of 3 and 2 bits and 7 sink launches.
TABLE_CASES = [(1, "normal", None), (2, "ties", None), (5, "normal", None), (5, "ties", None), (5, "nofamily", None),
               (L, "normal", None), (L, "indegree2", None), (L + 1, "ties", None), (L + 1, "minf", None),
               (L + 2, "indegree2", None), (L + 2, "normal", None), (L + 4, "ties", None), (L + 4, "nofamily", None),
               (10, "ties", (4, 3)), (10, "normal", (4, 3)), (9, "minf", (4, 2)), (9, "indegree2", (3, 1))]


def device(n, kind, tiling=None, tables=True):
    from pgmpy_amd import engine as E
    from pgmpy_amd.estimators._xs import XsPlan
    E.device()  # first: it brings torch's HIP runtime in before the library loads
    plan = XsPlan(n, *(tiling or ()))
    return dict(plan.run(*C.families(n, kind), want_tables=tables), phase_ms=plan.phase_ms())


@pytest.mark.parametrize("n, kind, tiling", TABLE_CASES)
def test_tables_equal_the_recurrence_bit_for_bit(n, kind, tiling):
    """Q, A, R, K and the result record against reference (a).  Every operation of the recurrence is a compare or a
    single IEEE fp64 add of two given numbers, and the order of step 1 is total, so no tiling or order of passes can
    change a bit: equality is the bar, not a tolerance."""
    ref, got = C.recurrence(n, *C.families(n, kind)), device(n, kind, tiling)
    for name in ("Q", "A", "R", "K"):
        bits = np.uint64 if name in "QR" else np.uint32
        same = got[name].view(bits) == ref[name].view(bits)
        assert same.all(), (name, int((~same).sum()), np.argwhere(~same)[:4].tolist())
    assert (got["parents"], got["order"], got["score"]) == (ref["parents"], ref["order"], ref["score"])
    assert got["infeasible"] == ref["infeasible"] == (kind == "nofamily")
    assert list(got["phase_ms"]) == ["scatter", "zeta", "sink"] and min(got["phase_ms"].values()) >= 0.0


@pytest.mark.parametrize("n", [4, 5, 6])
@pytest.mark.parametrize("kind", ["normal", "ties", "indegree2", "minf"])
def test_result_against_brute_force(n, kind):
    """Reference (b) shares nothing with the lattice.  The parent sets are given families, acyclic along the order, and
    sum to R[V], the brute-force maximum: only the order of n adds differs, hence n * 2^-52 * sum |terms|."""
    nodes, masks, scores = C.families(n, kind)
    got = device(n, kind, tables=False)
    given = {(int(v), int(m)): s for v, m, s in zip(nodes, masks, scores)}
    terms = [given[(v, got["parents"][v])] for v in range(n)]
    later = 0
    for v in reversed(got["order"]):  # sinks come first: a node's parents all stand after it
        assert got["parents"][v] & ~later == 0
        later |= 1 << v
    assert sorted(got["order"]) == list(range(n)) and not got["infeasible"]
    tol = n * 2.0 ** -52 * sum(abs(t) for t in terms)
    assert abs(sum(terms) - got["score"]) <= tol and abs(C.brute_force(n, nodes, masks, scores) - got["score"]) <= tol


def test_repeatable_and_independent_of_the_tiling():
    n, kind = L + 1, "ties"
    runs = [device(n, kind), device(n, kind), device(n, kind, (5, 2)), device(n, kind, (12, 1))]
    for other in runs[1:]:
        for name in ("Q", "A", "R", "K"):
            assert runs[0][name].tobytes() == other[name].tobytes(), name
        assert (runs[0]["parents"], runs[0]["order"], runs[0]["score"]) == (other["parents"], other["order"], other["score"])


EDGES = [("A", "C"), ("B", "C"), ("C", "D"), ("B", "E"), ("D", "F"), ("E", "F")]
NODES = list("ABCDEF")


@lru_cache(maxsize=None)
def frame():
    """2,000 rows sampled from a fixed binary network over EDGES."""
    rng = np.random.default_rng(7)
    cols = {}
    for v in NODES:  # NODES is a topological order of EDGES
        parents = [u for u, w in EDGES if w == v]
        code = sum(cols[u] << i for i, u in enumerate(parents)) if parents else 0
        p = np.array([0.15, 0.8, 0.7, 0.1])[:1 << len(parents)][code] if parents else 0.4
        cols[v] = (rng.random(2000) < p).astype(np.int64)
    return pd.DataFrame(cols)


@pytest.mark.parametrize("score_name", ["BIC", "BDeu"])
def test_estimate_end_to_end(score_name):
    import pgmpy_amd.estimators as est
    from pgmpy_amd.estimators.ExhaustiveSearch import enumerate_families

    data, n = frame(), len(NODES)
    scorer = getattr(est, score_name)(data)
    search = est.ExhaustiveSearch(data, scoring_method=scorer)
    model = search.estimate()
    assert nx.is_directed_acyclic_graph(model) and list(model.nodes()) == NODES and search.n_families == n * 2 ** (n - 1)
    fams = enumerate_families(n)
    scores = np.array(scorer.local_scores([(NODES[v], [NODES[u] for u in range(n) if m >> u & 1]) for v, m in fams]))
    nodes, masks = np.array([v for v, _ in fams], dtype=np.int32), np.array([m for _, m in fams], dtype=np.uint32)
    given = dict(zip(fams, scores))
    def tol_of(dag):  # n * 2^-52 * sum |terms| over the families of `dag`
        terms = [given[(v, sum(1 << NODES.index(u) for u in dag.predecessors(NODES[v])))] for v in range(n)]
        return n * 2.0 ** -52 * sum(abs(t) for t in terms)
    tol = tol_of(model)
    assert abs(search.best_score - C.brute_force(n, nodes, masks, scores)) <= tol
    assert abs(scorer.score(model) - search.best_score) <= tol
    hill = est.HillClimbSearch(data).estimate(scoring_method=scorer, show_progress=False)
    assert search.best_score >= scorer.score(hill) - tol_of(hill)
    # a forbidden and a required edge: honoured, and they cannot raise the score
    have = list(model.edges())[0]
    knowledge = est.ExpertKnowledge(forbidden_edges=[have], required_edges=[("F", "A")])
    bound = est.ExhaustiveSearch(data, scoring_method=scorer)
    constrained = bound.estimate(expert_knowledge=knowledge)
    assert not constrained.has_edge(*have) and constrained.has_edge("F", "A") and nx.is_directed_acyclic_graph(constrained)
    assert bound.best_score <= search.best_score and abs(scorer.score(constrained) - bound.best_score) <= tol_of(constrained)
    with pytest.raises(ValueError, match="no DAG meets"):
        bound.estimate(max_indegree=0, expert_knowledge=knowledge)
    # the host enumeration on three columns: its best score is the programme's
    small = est.ExhaustiveSearch(data[list("ABC")], scoring_method=getattr(est, score_name)(data[list("ABC")]))
    ranked = small.all_scores()
    totals = [t for t, _ in ranked]
    assert len(ranked) == 25 and totals == sorted(totals) and small.estimate() is not None
    assert abs(totals[-1] - small.best_score) <= 3 * 2.0 ** -52 * abs(totals[0])  # log scores: |worst| bounds sum |terms|
