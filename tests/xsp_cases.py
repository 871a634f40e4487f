"""Inputs and two plain numpy references for the exact edge posteriors (include/pgmhip.h "Exact edge posteriors"):
(a) `brute`, a sum over all n! orders that shares nothing with the lattice; (b) `recurrence`, the six steps as the
header states them, in float64 or longdouble.  `fams` are (nodes, masks, scores) as pgm_xs_posterior takes them."""
import functools
import itertools

import numpy as np

from tests.xs_cases import families as search_families, popcount, squeeze

LD = np.longdouble
FLOOR = 4 * 2.0 ** -52  # see `figure`


def lse2(a, b):
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    ok = d < np.inf
    return np.where(ok, np.maximum(a, b) + np.log1p(np.exp(-np.where(ok, d, 0))), np.maximum(a, b))


@functools.lru_cache(maxsize=None)
def families(n, kind):
    """"full": every family, N(0, 2), in a shuffled list.  "pruned": at most two parents, 0 -> 1 and 1 -> 2 forbidden,
    0 -> 2 required (each where n has the nodes), a quarter of the families with parents at -inf; the order 0, 1, 2, ...
    stays possible.  "range" (n = 6): scores near -5e4 and 900 nats apart, node 0 with its empty family only, node 5
    with every family that lacks parent 1 at -inf.  "infeasible": the last node has no family."""
    rng = np.random.default_rng(77 * n + len(kind))
    nodes, masks, _ = search_families(n, "normal")
    scores = 2.0 * rng.standard_normal(len(nodes))
    keep = np.ones(len(nodes), dtype=bool)
    has = lambda u: (masks >> np.uint32(u)) & 1 == 1
    if kind == "pruned":
        keep = (popcount(masks) <= 2) & ~((nodes == 1) & has(0)) & ~((nodes == 2) & has(1)) & ~((nodes == 2) & ~has(0))
        scores[(rng.random(len(nodes)) < 0.25) & (masks != 0) & ~((nodes == 2) & (masks == 1))] = -np.inf
    if kind == "range":
        scores = -5e4 - 900.0 * rng.permutation(len(nodes))
        keep = (nodes != 0) | (masks == 0)
        scores[(nodes == 5) & ~has(1)] = -np.inf
    if kind == "infeasible":
        keep = nodes != n - 1
    return nodes[keep], masks[keep], scores[keep]


def brute(n, fams, dtype=LD):
    """Reference (a): {"edge_post", "mass", "log_z"}.  An order's weight is the product over the nodes of the summed
    weights of the listed parent sets inside the node's predecessors; Z and the edge sums are accumulated in `dtype`
    after a shift by each node's largest score."""
    per = [[(int(P), dtype(s)) for v, P, s in zip(*fams) if v == w and s > -np.inf] for w in range(n)]
    shift = [max((s for _, s in f), default=dtype(0)) for f in per]
    Z, edge, mass = dtype(0), np.zeros((n, n), dtype=dtype), np.zeros(n, dtype=dtype)
    for order in itertools.permutations(range(n)):
        before, local = 0, []
        for v in order:
            w = [(P, np.exp(s - shift[v])) for P, s in per[v] if P & ~before == 0]
            local.append((v, w, sum((x for _, x in w), dtype(0))))
            before |= 1 << v
        weight = np.prod([t for _, _, t in local], dtype=dtype)
        Z += weight
        for v, w, t in local if weight > 0 else ():
            mass[v] += weight
            for P, x in w:
                edge[[u for u in range(n) if P >> u & 1], v] += weight * x / t
    return {"edge_post": edge / Z, "mass": mass / Z, "log_z": np.log(Z) + sum(shift, dtype(0))}


def recurrence(n, fams, dtype=np.float64):
    """Reference (b): the six steps; also "alpha" [n, 2^(n-1)], "F", "B" [2^n]."""
    nodes, masks, scores = fams
    W, cells, full = n - 1, 1 << (n - 1), (1 << n) - 1
    given = scores > -np.inf
    v, P, s = nodes[given].astype(np.int64), masks[given].astype(np.int64), scores[given].astype(dtype)
    alpha = np.full((n, cells), -np.inf, dtype=dtype)
    alpha[v, squeeze(P, v)] = s
    T = np.arange(cells)
    for j in range(W):
        hi = T[(T >> j) & 1 == 1]
        alpha[:, hi] = lse2(alpha[:, hi], alpha[:, hi ^ (1 << j)])
    S = np.arange(1 << n)
    size = popcount(S.astype(np.uint32))
    F, B = np.full(1 << n, -np.inf, dtype=dtype), np.full(1 << n, -np.inf, dtype=dtype)
    F[0] = B[0] = 0
    for layer in range(1, n + 1):
        for u in range(n):
            sel = S[(size == layer) & ((S >> u) & 1 == 1)]
            prev = sel ^ (1 << u)
            F[sel] = lse2(F[sel], alpha[u, squeeze(prev, u)] + F[prev])
            B[sel] = lse2(B[sel], alpha[u, squeeze(full ^ sel, u)] + B[prev])
    gamma = np.empty((n, cells), dtype=dtype)
    for u in range(n):
        Su = (T & ((1 << u) - 1)) | ((T >> u) << (u + 1))
        gamma[u] = F[Su] + B[full ^ Su ^ (1 << u)]
    for j in range(W):
        lo = T[(T >> j) & 1 == 0]
        gamma[:, lo] = lse2(gamma[:, lo], gamma[:, lo | (1 << j)])
    edge, mass = np.zeros((n, n), dtype=dtype), np.zeros(n, dtype=dtype)
    with np.errstate(invalid="ignore"):
        term = np.exp(s + gamma[v, squeeze(P, v)] - F[full])
    np.add.at(mass, v, term)
    for u in range(n):
        np.add.at(edge[u], v[(P >> u) & 1 == 1], term[(P >> u) & 1 == 1])
    if F[full] == -np.inf:
        edge[:], mass[:] = np.nan, np.nan
    return {"edge_post": edge, "mass": mass, "log_z": np.array([F[full], B[full]]), "alpha": alpha, "F": F, "B": B}


def gaps(got, want):
    """The largest |difference| over edge_post and mass, and over log_z relative to max(1, |log Z|): the scores are of
    order 1, so a log Z that happens to lie near 0 was still rounded like a number of order 1."""
    ref = np.ravel(want["log_z"])[0]  # `brute` has one log Z, `recurrence` F[V] and B[V]: F[V] is the reference
    return max(float(np.abs(got["edge_post"] - want["edge_post"]).max()), float(np.abs(got["mass"] - want["mass"]).max()),
               float(np.abs(np.asarray(got["log_z"], dtype=LD) - ref).max() / max(1, abs(ref))))


def figure(n, fams):
    """(the longdouble run of `recurrence`, the bound of the case): 8 times the gap between its float64 and its
    longdouble run, which is what float64 costs this order of operations on this input.  Below FLOOR, FLOOR stands in:
    a small case can round to the longdouble value by luck, while the last step alone, exp(s + Gamma - log Z), rounds
    three operands and two adds, and libm's and the device's exp and log1p differ by an ulp each."""
    hi = recurrence(n, fams, LD)
    return hi, 8 * max(gaps(recurrence(n, fams), hi), FLOOR)
