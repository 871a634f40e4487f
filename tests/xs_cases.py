"""Inputs and two plain numpy references for the exact structure search (include/pgmhip.h): (a) `recurrence`, the three
steps as the header states them, vectorised per bit; (b) `brute_force`, the maximum over all n! node orderings."""
import functools
import itertools

import numpy as np

NONE = np.uint32(0xFFFFFFFF)


def squeeze(S, v):
    return (S & ((1 << v) - 1)) | ((S >> (v + 1)) << v)


def popcount(m):
    return np.unpackbits(np.ascontiguousarray(m, dtype=np.uint32).view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1).reshape(np.shape(m))


def better(sa, ma, sb, mb):
    pa, pb = popcount(ma), popcount(mb)
    return (sa > sb) | ((sa == sb) & ((pa < pb) | ((pa == pb) & (ma < mb))))


@functools.lru_cache(maxsize=None)
def families(n, kind, seed=0):
    """(nodes, masks, scores).  kind: "normal" (every family, N(0, 1)), "ties" (scores from {-3 .. 0}: both tie rules
    decide), "indegree2" (at most two parents), "nofamily" (the last node has none), "minf" (ties, a third -inf)."""
    rng = np.random.default_rng(1000 * n + seed)
    cells = 1 << (n - 1)
    nodes = np.repeat(np.arange(n, dtype=np.int32), cells)
    T = np.tile(np.arange(cells, dtype=np.uint32), n)
    low = (np.uint32(1) << nodes.astype(np.uint32)) - np.uint32(1)
    masks = (T & low) | ((T & ~low) << np.uint32(1))
    if kind in ("ties", "minf"):
        scores = rng.integers(-3, 1, size=len(nodes)).astype(np.float64)
        if kind == "minf":
            scores[rng.random(len(nodes)) < 1 / 3] = -np.inf
    else:
        scores = rng.standard_normal(len(nodes))
    keep = np.ones(len(nodes), dtype=bool)
    if kind == "indegree2":
        keep = popcount(masks) <= 2
    if kind == "nofamily":
        keep = nodes != n - 1
    order = rng.permutation(int(keep.sum()))  # the order of the list must not matter
    return nodes[keep][order], masks[keep][order], scores[keep][order]


def recurrence(n, nodes, masks, scores):
    """Reference (a): {"Q", "A" [n, 2^(n-1)], "R", "K" [2^n], "score", "parents", "order", "infeasible"}."""
    W, cells = n - 1, 1 << (n - 1)
    Q = np.full((n, cells), -np.inf)
    A = np.full((n, cells), NONE, dtype=np.uint32)
    given = scores > -np.inf
    v, P = nodes[given].astype(np.int64), masks[given].astype(np.int64)
    Q[v, squeeze(P, v)], A[v, squeeze(P, v)] = scores[given], masks[given]
    T = np.arange(cells)
    for j in range(W):
        hi = T[(T >> j) & 1 == 1]
        lo = hi ^ (1 << j)
        take = better(Q[:, lo], A[:, lo], Q[:, hi], A[:, hi])
        Q[:, hi], A[:, hi] = np.where(take, Q[:, lo], Q[:, hi]), np.where(take, A[:, lo], A[:, hi])
    S = np.arange(1 << n)
    R = np.full(1 << n, -np.inf)
    K = np.full(1 << n, NONE, dtype=np.uint32)
    R[0] = 0.0
    size = popcount(S.astype(np.uint32))
    for layer in range(1, n + 1):
        sets = S[size == layer]
        K[sets] = np.log2(sets & -sets).astype(np.uint32)  # the smallest member, kept when every candidate is -inf
        for v in range(n):
            sel = sets[(sets >> v) & 1 == 1]
            prev = sel ^ (1 << v)
            cand = R[prev] + Q[v, squeeze(prev, v)]
            win = cand > R[sel]
            R[sel[win]], K[sel[win]] = cand[win], v
    out = {"Q": Q, "A": A, "R": R, "K": K, "score": R[-1], "infeasible": R[-1] == -np.inf, "parents": [0] * n, "order": []}
    s = (1 << n) - 1
    for _ in range(n):
        v = int(K[s])
        s ^= 1 << v
        out["parents"][v] = int(A[v, squeeze(s, v)])
        out["order"].append(v)
    return out


def brute_force(n, nodes, masks, scores):
    """Reference (b): the best total over all orderings, in plain Python."""
    fams = [[] for _ in range(n)]
    for v, P, s in zip(nodes.tolist(), masks.tolist(), scores.tolist()):
        fams[v].append((P, s))
    best = -np.inf
    for order in itertools.permutations(range(n)):
        before, total = 0, 0.0
        for v in order:
            total += max((s for P, s in fams[v] if P & ~before == 0), default=-np.inf)
            before |= 1 << v
        best = max(best, total)
    return best
