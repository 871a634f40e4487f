"""The cases of the Mplp tests and a plain numpy restatement of the algorithm (sequential model order, or any
order of the clusters given as `order`), in float64 or longdouble.

A case is (card, unary, clusters, n_trip): card[v]; unary[v] an array [card[v]]; clusters a list of (vars, theta)
with theta shaped by the cardinalities of vars, the last n_trip of them zero-theta tightening triplets.  The state
is laid out as the library lays it out: node objectives, cluster objectives, the messages in (cluster, set) order
each shaped like its set's objective, best primal, dual_lp, the best codes.
"""
import itertools
from collections import Counter

import numpy as np


def sets_of(clusters, n_trip):
    """Per cluster the intersection sets (kind, index, ax): a node ("n", v) or the objective of an edge cluster
    ("c", j); ax[i] is the position in the cluster of the set's i-th axis."""
    nf = len(clusters) - n_trip
    deg = Counter(v for vs, _ in clusters[:nf] for v in vs)
    out = []
    for i, (vs, _) in enumerate(clusters):
        if i < nf:
            out.append([("n", v, (p,)) for p, v in enumerate(vs) if deg[v] > 1])
            continue
        ss = []
        for pa, pb in itertools.combinations(range(3), 2):
            j = next(j for j in range(nf) if set(clusters[j][0]) == {vs[pa], vs[pb]})
            ss.append(("c", j, (pa, pb) if clusters[j][0][0] == vs[pa] else (pb, pa)))
        out.append(ss)
    return out


def lattice_sum(node_terms, cluster_terms, f):
    """The fixed order of the two sums of an iteration (include/pgmhip.h): 256 partial sums, term i of the nodes and
    then term i of the clusters added to partial i mod 256; a butterfly over each 64 of them; the four results in
    order.  The halvings make the terms inexact after some ten iterations, so the order has to be the library's."""
    part = np.zeros(256, dtype=f)
    for terms in (node_terms, cluster_terms):
        for i, x in enumerate(terms):
            part[i % 256] += x
    w = part.reshape(4, 64)
    for d in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ d]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def run(case, n_iter, dual_thr=0.0, gap_thr=0.0, dtype=np.float64, order=None, state=None):
    card, unary, clusters, n_trip = case
    f = dtype
    sets = sets_of(clusters, n_trip)
    theta = [np.asarray(t, dtype=f) for _, t in clusters]
    un = [np.asarray(u, dtype=f) for u in unary]
    obj = {("n", v): un[v].copy() for v in range(len(card))}
    obj.update({("c", j): t.copy() for j, t in enumerate(theta)})
    msg = {(j, i): np.zeros_like(obj[s[:2]]) for j, ss in enumerate(sets) for i, s in enumerate(ss)}
    keys = list(obj) + list(msg)
    best, best_codes = f(-np.inf), np.zeros(len(card), dtype=np.uint8)
    n = len(card)
    dual_of = lambda: lattice_sum([obj[("n", v)].max() for v in range(n)], [obj[("c", j)].max() for j in range(len(theta))], f)
    dual_lp = dual_of()
    if state is not None:
        at = 0
        for k in keys:
            tab = obj if k in obj else msg
            tab[k] = np.asarray(state[at:at + tab[k].size], dtype=f).reshape(tab[k].shape)
            at += tab[k].size
        best, dual_lp, best_codes = f(state[at]), f(state[at + 1]), np.asarray(state[at + 2:], dtype=np.uint8)
    dual_gap = int_gap = f(np.nan)
    trace, used = [], 0
    for it in range(n_iter):
        for j in (range(len(clusters)) if order is None else order):
            ss, shape = sets[j], theta[j].shape
            if not ss:
                continue

            def wide(s):  # the set's objective broadcast over the cluster
                t = obj[s[:2]] if list(s[2]) == sorted(s[2]) else obj[s[:2]].T
                return t.reshape([shape[p] if p in s[2] else 1 for p in range(len(shape))])

            S = obj[("c", j)].copy()
            for s in ss:
                S = S + wide(s)
            new = []
            for i, s in enumerate(ss):
                phi = S.max(axis=tuple(p for p in range(len(shape)) if p not in s[2])) * f(1.0 / len(ss))
                phi = phi if list(s[2]) == sorted(s[2]) else phi.T
                new.append((phi, phi - (obj[s[:2]] - msg[(j, i)])))
            total = theta[j].copy()
            for i, (s, (phi, m)) in enumerate(zip(ss, new)):
                msg[(j, i)], obj[s[:2]] = m, phi
            for i, s in enumerate(ss):
                t = msg[(j, i)] if list(s[2]) == sorted(s[2]) else msg[(j, i)].T
                total = total - t.reshape([shape[p] if p in s[2] else 1 for p in range(len(shape))])
            obj[("c", j)] = total
        codes = np.array([int(np.argmax(obj[("n", v)])) for v in range(len(card))], dtype=np.uint8)
        primal = lattice_sum([un[v][codes[v]] for v in range(n)], [t[tuple(codes[list(vs)])] for (vs, _), t in zip(clusters, theta)], f)
        if best < primal:
            best, best_codes = primal, codes
        new_dual = dual_of()
        dual_gap, int_gap = abs(dual_lp - new_dual), abs(dual_lp - best)
        conv = bool(dual_thr and dual_gap < dual_thr) or bool(gap_thr and int_gap < gap_thr)
        if not conv:
            dual_lp = new_dual
        top2 = min(np.diff(np.sort(obj[("n", v)])[-2:])[0] for v in range(len(card)) if card[v] > 1)
        trace.append((primal, new_dual, top2))
        used = it + 1
        if conv and it >= 16:
            break
    flat = np.concatenate([(obj[k] if k in obj else msg[k]).ravel() for k in keys] + [[best, dual_lp], best_codes.astype(f)])
    return dict(codes=best_codes, best=best, dual_lp=dual_lp, dual_gap=dual_gap, int_gap=int_gap, n_iter=used,
                state=flat, trace=trace)


def make(card, edges, seed, dyadic, trip=()):
    """A case over `edges` with random terms: multiples of 1/8 in [-4, 4] (dyadic) or normal deviates."""
    rng = np.random.default_rng(seed)
    draw = (lambda n: rng.integers(-32, 33, n) / 8.0) if dyadic else (lambda n: rng.normal(size=n))
    unary = [draw(k) for k in card]
    clusters = [(e, draw(card[e[0]] * card[e[1]]).reshape(card[e[0]], card[e[1]])) for e in edges]
    clusters += [(t, np.zeros([card[v] for v in t])) for t in trip]
    return card, unary, clusters, len(trip)


def grid_edges(rows, cols):
    at = lambda r, c: r * cols + c
    return [(at(r, c), at(r, c + 1)) for r in range(rows) for c in range(cols - 1)] + \
           [(at(r, c), at(r + 1, c)) for r in range(rows - 1) for c in range(cols)]


GRID_CARD = [2, 3, 4, 3, 2, 4, 4, 2, 3]
# a 4-cycle with the chord (0, 2), node 4 hanging off node 1 (k = 1) and the isolated edge (5, 6) (k = 0)
CHORD_EDGES = [(0, 1), (1, 2), (3, 2), (3, 0), (0, 2), (1, 4), (5, 6)]
EXACT = {"grid": make(GRID_CARD, grid_edges(3, 3), 1, True),
         "chord": make([2, 3, 4, 2, 3, 4, 2], CHORD_EDGES, 2, True)}

_S = lambda a, b: np.array([[a, b], [b, a]])
DOC = ([2] * 6, [np.array(u) for u in ([0.54577, 1.8323], [0.93894, 1.065], [0.89205, 1.121], [0.56292, 1.7765],
                                       [0.47117, 2.1224], [1.5093, 0.66257])],
       [((0, 1), _S(1.3207, 0.75717)), ((1, 2), _S(0.00024189, 4134.2)), ((2, 3), _S(0.0043227, 231.34)),
        ((4, 5), _S(31.228, 0.032023))], 0)
NEAR = {"doc": DOC, "grid": make(GRID_CARD, grid_edges(3, 3), 7, False)}


def triangle(n_trip=0):
    """A frustrated binary triangle: every edge pays 1 for disagreement; the pairwise relaxation is loose."""
    un = [np.array([0.1, 0.0]), np.array([0.0, 0.2]), np.array([0.05, 0.0])]
    clusters = [(e, _S(-1.0, 1.0)) for e in ((0, 1), (1, 2), (0, 2))] + [((0, 1, 2), np.zeros((2, 2, 2)))] * n_trip
    return [2, 2, 2], un, clusters, n_trip


def signs_2x3(seed=3):
    rng = np.random.default_rng(seed)
    un = [rng.normal(size=2) * 0.1 for _ in range(6)]
    return [2] * 6, un, [(e, _S(-1.0, 1.0) * rng.choice([-1.0, 1.0])) for e in grid_edges(2, 3)], 0


def brute_force(case):
    card, unary, clusters, _ = case
    return max(sum(unary[v][x[v]] for v in range(len(card))) + sum(t[tuple(x[v] for v in vs)] for vs, t in clusters)
               for x in itertools.product(*[range(k) for k in card]))


def figure(case, n_iter, thr=0.0002):
    """(longdouble run, the largest float64-against-longdouble difference of the restatement's primal and dual
    values over the iterations): what the order of a sum may move in this case."""
    lo, hi = run(case, n_iter, thr, thr), run(case, n_iter, thr, thr, dtype=np.longdouble)
    return hi, max(float(abs(a[i] - b[i])) for a, b in zip(lo["trace"], hi["trace"]) for i in (0, 1))


def batch_unaries(case, rows=130, strong=50, seed=5):
    """Dyadic node terms for `rows` instances of a case; row `strong` prefers state 0 of every node by 64 and stops at
    iteration 17, its neighbours 49 and 51 run all 40 iterations (the restatement says so; the test checks it)."""
    rng = np.random.default_rng(seed)
    un = rng.integers(-32, 33, (rows, sum(case[0]))) / 8.0
    un[strong] = np.concatenate([[64.0] + [0.0] * (k - 1) for k in case[0]])
    return un


def with_unary(case, row):
    return case[0], np.split(row, np.cumsum(case[0])[:-1]), case[2], case[3]
