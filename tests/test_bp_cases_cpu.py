"""tests/bp_cases.py checked without a device: the trees are junction trees, their impossible pattern has mass 0
and every other pattern mass > 0, the long-double closed form agrees with the fp64 message-passing oracle
(oracle.bp.calibrate) on every tree, pattern and operation, and the derived bound stays far below the
tolerances the older GPU tests use."""
import numpy as np
import pytest

from oracle import bp as OBP
from oracle.factor import OFactor
from tests import bp_cases as BC

NAMES = sorted(BC.TREES)


def test_long_double_is_extended():
    assert BC.HAVE_LD, "the reference needs an extended-precision np.longdouble"


@pytest.mark.parametrize("name", NAMES)
def test_tree_is_a_junction_tree_rooted_at_its_first_clique(name):
    import networkx as nx

    t = BC.TREES[name]
    assert BC.running_intersection(t)
    assert len(t["cliques"]) <= 25 and all(1 <= k <= 4 for k in t["card"].values())
    assert all(BC.prod(t["card"][v] for v in c) <= 256 for c in t["cliques"])
    # BatchedJunctionTree: root = the graph's first node, order = networkx's breadth-first edges from it
    g = nx.Graph()
    g.add_nodes_from(t["cliques"])
    g.add_edges_from(t["edges"])
    assert list(g.nodes())[0] == t["cliques"][0]
    assert list(nx.bfs_edges(g, t["cliques"][0])) == BC.rooted(t)[0]
    assert all(set(a) & set(b) for a, b in t["edges"])
    assert (set(t["want"]["any"]) | set(t["want"]["fused"]) | set(t["want"]["unfused"])) <= \
        set(BC.TRACE_NAMES) | set(BC.EXTRA_NAMES)


def test_potentials_have_hard_zeros_and_no_tiny_values():
    for t in BC.TREES.values():
        vals = np.concatenate([p.ravel() for p in t["pots"].values()])
        assert vals.min() == 0.0 and vals[vals > 0].min() >= 0.05 and vals.max() < 1.05
        if vals.size >= 100:
            assert 0.1 < np.mean(vals == 0) < 0.4, t["name"]


@pytest.mark.parametrize("name", NAMES)
def test_only_the_impossible_pattern_has_mass_zero(name):
    t = BC.TREES[name]
    pats = BC.patterns(t)
    for op in ("sum", "max"):
        mass = BC.reference(t, op)["mass"]
        for i, p in enumerate(pats):
            if t["ev_vars"] and i == 1:
                assert p == t["impossible"] and mass[i] == 0, (name, op)
                for m in BC.reference(t, op)["marginals"].values():
                    assert np.isnan(m[i]).all()
            else:
                assert mass[i] > 1e-30, (name, op, i, p)
    # every pattern appears in the smallest batch's first rows or later ones; the impossible one in all
    if t["ev_vars"]:
        assert 1 in BC.row_patterns(t, 3)
        c = BC.codes(t, len(pats))
        assert c.shape == (len(t["ev_vars"]), len(pats)) and (c[:, 0] == 255).all()
        assert all(c[j, 2] == t["witness"][0][v] for j, v in enumerate(t["ev_vars"]))


@pytest.mark.parametrize("op", ["sum", "max"])
@pytest.mark.parametrize("name", NAMES)
def test_reference_agrees_with_the_message_passing_oracle(name, op):
    """The closed form against oracle.bp.calibrate (fp64, two-pass belief update with 0/0 -> 0): the bound once
    for the schedule roundings of the oracle (it multiplies and sums what the device schedule does, in
    another order), once more for the reference's side: 2 x bound.  Identical zero patterns."""
    t = BC.TREES[name]
    ref = BC.reference(t, op)
    tol = 2 * BC.bound(t, op)
    worst = 0.0
    order = BC.rooted(t)[0]
    for i, p in enumerate(BC.patterns(t)):
        pots = {}
        for c in t["cliques"]:
            f = OFactor(list(c), [t["card"][v] for v in c], t["pots"][c])
            for v, s in p.items():
                if BC.first_clique(t, v) == c:
                    ind = np.zeros(t["card"][v])
                    ind[s] = 1.0
                    f = OFactor(list(c), f.card, f.product(OFactor([v], [t["card"][v]], ind)).aligned(list(c)))
            pots[c] = f
        beliefs, seps = OBP.calibrate(t["cliques"], t["edges"], pots, op=op)
        for c in t["cliques"]:
            worst = max(worst, BC.check(beliefs[c].aligned(list(c)).ravel(), ref["beliefs"][c][i], tol,
                                        f"{name} {op} pattern {i} clique {c}"))
        for pc in order:
            want, sl = ref["seps"][pc]
            worst = max(worst, BC.check(seps[frozenset(pc)].aligned(sl).ravel(), want[i], tol,
                                        f"{name} {op} pattern {i} sepset {pc}"))
    print(f"{name} {op}: worst oracle difference {worst:.3f} x (2 x bound = {tol:.3g})")


def test_bound_is_derived_small_and_counts_what_it_says():
    for t in BC.TREES.values():
        for op in ("sum", "max"):
            assert 0 < BC.bound(t, op) < 1e-12, (t["name"], op)
            for v in t["variables"]:
                assert BC.bound(t, op) < BC.marginal_bound(t, op, v) < 1e-11
        assert BC.bound(t, "max") <= BC.bound(t, "sum")
    # chain3 by hand: (a,b) 1 + 2 findings + 1 child + 2, r = 6 / 3; (b,c) 1 + 1 + 1 + 2, r = 12 / 3;
    # (c,d) 1 + 0 + 0 + 2, r = 8 / 4
    assert BC.roundings(BC.TREES["chain3"], "sum") == 2 * ((6 + 2) + (5 + 4) + (3 + 2)) + 2
    assert BC.roundings(BC.TREES["chain3"], "max") == 2 * (6 + 5 + 3) + 2


def test_fused_row_regimes():
    assert [BC.FUSED_ROWS(n) for n in (3, 64, 65, 66, 1030)] == [False, True, False, True, True]
    every = set()
    for t in BC.TREES.values():
        every |= t["want"]["any"] | t["want"]["fused"] | t["want"]["unfused"]
    # the table's names: each is planned by some tree (the knob's own name by the knob test)
    # (and the two-marginal passes by `pairs` at PAIR_ROWS rows)
    assert set(BC.TRACE_NAMES) - every == BC.KNOB_ONLY | BC.PAIR_NAMES
    assert BC.FUSED_ROWS(BC.PAIR_ROWS) and BC.PAIR_NAMES <= BC.FUSED_ONLY
