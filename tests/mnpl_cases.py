"""The cases of the pseudo-likelihood tests (test_mnpl_cpu.py, test_mnpl_gpu.py) and their plain reference: PL and its
gradient by the definition, row by row over the code matrix, in numpy.longdouble.  Going row by row checks the
count-table reformulation of the kernel and not only its arithmetic."""
import itertools
from functools import lru_cache

import numpy as np

LD = np.longdouble
LDS_PAD = 64  # bytes of a workgroup's LDS beside the residual table (pgm_mnpl_info_t.lds_max holds both)


def star_leaves(lds_max):
    """The most binary leaves whose centre (binary) the plan accepts: a residual table of 2 * 2^leaves fp64."""
    return int(np.floor(np.log2((lds_max - LDS_PAD) // 16)))


def _case(name, card, scopes, n_rows, seed, theta_shift=None, missing=0.0):
    rng = np.random.default_rng(seed)
    codes = np.stack([rng.integers(0, k, n_rows) for k in card]).astype(np.uint8)
    if missing:
        codes[rng.random(codes.shape) < missing] = 255
    sizes = [int(np.prod([card[v] for v in s])) for s in scopes]
    theta = rng.uniform(-2.0, 2.0, sum(sizes))
    if theta_shift is not None:
        at = sum(sizes[:theta_shift])
        theta[at:at + sizes[theta_shift]] += 700.0
    return dict(name=name, card=list(card), scopes=[tuple(s) for s in scopes], codes=codes, theta=theta)


def grid_scopes(h, w):
    at = lambda r, c: r * w + c
    edges = [(at(r, c), at(r, c + 1)) for r in range(h) for c in range(w - 1)]
    edges += [(at(r, c), at(r + 1, c)) for r in range(h - 1) for c in range(w)]
    return [(v,) for v in range(h * w)] + sorted(edges)


CHAIN = ([2, 3, 2], [(0, 1), (1, 2)])
TRIANGLE = ([2, 3, 2], [(0, 1, 2), (2, 0), (1,)])  # the pair repeats two variables of the triple, in the other order


@lru_cache(maxsize=None)
def cases(lds_max):
    n = star_leaves(lds_max)
    out = [
        _case("unary", [3], [(0,)], 300, 1),
        _case("chain", *CHAIN, 300, 2),
        _case("triangle", *TRIANGLE, 300, 3),
        _case("grid", [3] * 9, grid_scopes(3, 3), 300, 4),
        _case("grid_shift", [3] * 9, grid_scopes(3, 3), 300, 4, theta_shift=12),
        _case("star", [2] * (n + 1), [(0, j) for j in range(1, n + 1)], 200, 5),
        _case("chain_missing", *CHAIN, 300, 6, missing=0.1),
        # beyond the issue's list: five tables over one wide scope do not fit in LDS beside the residual table, so
        # they are read through the caches (the other cases stage them)
        _case("wide_theta", [2, 45, 45], [(0, 1, 2)] * 5, 300, 7),
    ]
    return {c["name"]: c for c in out}


def joined(a, b):
    """Case a and case b side by side on disjoint columns, a's factors first (so their theta offsets stay)."""
    k = len(a["card"])
    return dict(name=a["name"] + "+" + b["name"], card=a["card"] + b["card"],
                scopes=a["scopes"] + [tuple(v + k for v in s) for s in b["scopes"]],
                codes=np.concatenate([a["codes"], b["codes"]]), theta=np.concatenate([a["theta"], b["theta"]]))


def family_data(card, scopes, seed):
    """(codes, log phi): every joint state x repeated prod_f phi_f(x_f) times for integer tables phi in 1 .. 3, so the
    empirical distribution lies exactly in the model family and log phi is a maximiser of PL."""
    rng = np.random.default_rng(seed)
    phi = [rng.integers(1, 4, [card[v] for v in s]) for s in scopes]
    rows = []
    for x in itertools.product(*[range(k) for k in card]):
        rows += [x] * int(np.prod([p[tuple(x[v] for v in s)] for p, s in zip(phi, scopes)]))
    return np.array(rows, dtype=np.uint8).T.copy(), np.concatenate([np.log(p.astype(np.float64)).ravel() for p in phi])


def blanket(scopes, i):
    return sorted({v for s in scopes if i in s for v in s} - {i})


def reference(card, scopes, codes, theta):
    """(value, node_values, grad, dev) in longdouble, row by row: a row counts for node i unless a cell of i or of its
    blanket is 255.  dev = the largest |logit - lse| met, which bounds a term of any of the sums."""
    sizes = [int(np.prod([card[v] for v in s])) for s in scopes]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    tabs = [np.asarray(theta[offs[f]:offs[f + 1]], dtype=LD).reshape([card[v] for v in s]) for f, s in enumerate(scopes)]
    grads = [np.zeros_like(t) for t in tabs]
    node_values, dev = np.zeros(len(card), dtype=LD), LD(0)
    for x in codes.T:
        for i in range(len(card)):
            if x[i] == 255 or any(x[j] == 255 for j in blanket(scopes, i)):
                continue
            at = [(f, tuple(slice(None) if v == i else int(x[v]) for v in s)) for f, s in enumerate(scopes) if i in s]
            logit = sum((tabs[f][idx] for f, idx in at), np.zeros(card[i], dtype=LD))
            top = logit.max()
            rel = logit - (top + np.log(np.exp(logit - top).sum()))
            dev = max(dev, np.abs(rel).max())
            node_values[i] += rel[x[i]]
            resid = -np.exp(rel)
            resid[x[i]] += 1
            for f, idx in at:
                grads[f][idx] += resid
    return node_values.sum(), node_values, np.concatenate([g.ravel() for g in grads]), dev


def atol(card, scopes, n_rows, dev, whole=False):
    """The issue's bound (T + 64) 2^-53 sum|term| with sum|term| <= 2 n_rows (1 + dev).  A node value adds the entries
    of the node's table card_i prod card_MB(i); a gradient entry adds, for each member of its factor, at most the
    configurations of that member's table: T = the largest node table times the widest scope covers both.  The
    whole value is every node's terms: T and the magnitude summed over the nodes."""
    tables = [card[i] * int(np.prod([card[j] for j in blanket(scopes, i)])) for i in range(len(card))]
    T, span = (sum(tables), len(card)) if whole else (max(tables) * max(len(s) for s in scopes), 1)
    return float((T + 64) * 2.0 ** -53 * span * 2 * n_rows * (1 + dev))
