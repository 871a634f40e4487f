"""The cases of the LoopyBeliefPropagation tests, a plain numpy restatement of the three phases of an iteration
(include/pgmhip.h "Marginals by loopy belief propagation") in float64 or longdouble, and a brute-force enumerator.

A case is (card, unary, factors): card[v]; unary[v] the node term, an array [card[v]]; factors a list of (vars, table)
with table shaped by the cardinalities of vars.  The state is the messages in (factor, position) order.
"""
import functools

import numpy as np

from tests.mplp_cases import grid_edges

LD = np.longdouble


def seq_sum(cols, f):  # the columns added one after the other, as the kernel adds them
    acc = np.zeros(cols.shape[0], dtype=f)
    for k in range(cols.shape[1]):
        acc = acc + cols[:, k]
    return acc


wide = lambda vec, pos, nv: vec.reshape([-1 if p == pos else 1 for p in range(nv)])  # vec along axis pos of nv

def run(case, n_iter, tol=0.0, damping=0.0, dtype=np.float64, state=None):
    card, unary, factors = case
    f = dtype
    un = [np.asarray(u, dtype=f) for u in unary]
    psi = [np.asarray(t, dtype=f) for _, t in factors]
    pairs = [(i, j) for i, (vs, _) in enumerate(factors) for j in range(len(vs))]
    node = {p: factors[p[0]][0][p[1]] for p in pairs}
    at = {v: [p for p in pairs if node[p] == v] for v in range(len(card))}
    msg = {p: np.full(card[node[p]], f(1) / f(card[node[p]]), dtype=f) for p in pairs}
    if state is not None:
        msg = dict(zip(pairs, np.split(np.asarray(state, dtype=f), np.cumsum([card[node[p]] for p in pairs])[:-1])))

    def cavities():
        out = {}
        for p in pairs:
            c = un[node[p]].copy()
            for q in at[node[p]]:
                c = c * msg[q] if q != p else c
            out[p] = c
        return out

    trace, used, bad, lam = [], 0, False, f(damping)
    for it in range(n_iter):
        cav, new, res = cavities(), {}, f(0)
        for i, j in pairs:
            nv, w = psi[i].ndim, psi[i]
            for o in range(nv):
                w = w * wide(cav[(i, o)], o, nv) if o != j else w
            raw = seq_sum(np.moveaxis(w, j, 0).reshape(card[node[(i, j)]], -1), f)
            z = seq_sum(raw[None, :], f)[0]
            if not z > 0:
                bad = True
                continue
            new[(i, j)] = (f(1) - lam) * (raw / z) + lam * msg[(i, j)]
            res = max(res, np.abs(new[(i, j)] - msg[(i, j)]).max())
        if bad:
            break
        msg, used = new, it + 1
        trace.append((np.concatenate([msg[p] for p in pairs]) if pairs else np.zeros(0, dtype=f), res))
        if res < tol:
            break
    cav, logz, marg, fbel = cavities(), f(0), [], []
    for v in range(len(card)):
        b = un[v].copy()
        for q in at[v]:
            b = b * msg[q]
        b = b / seq_sum(b[None, :], f)[0]
        marg.append(b)
        ok = b > 0
        logz += (b[ok] * (np.log(un[v][ok]) - f(1 - len(at[v])) * np.log(b[ok]))).sum()
    for i, (vs, _) in enumerate(factors):
        k = wide(cav[(i, 0)], 0, len(vs))
        for o in range(1, len(vs)):
            k = k * wide(cav[(i, o)], o, len(vs))
        u = psi[i] * k
        A, ok = u.sum(), u > 0
        fbel.append((u / A).ravel())
        logz += -(u[ok] * np.log(np.broadcast_to(k, u.shape)[ok])).sum() / A + np.log(A)
    flat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=f)
    return dict(marginals=flat(marg), factor_beliefs=flat(fbel), logz=logz, n_iter=-1 if bad else used, trace=trace,
                residual=trace[-1][1] if trace else f(np.nan), state=trace[-1][0] if trace else flat([msg[p] for p in pairs]))


def brute_force(case):
    """(marginals, factor beliefs, log Z) by enumeration in longdouble."""
    card, unary, factors = case
    n = len(card)
    joint = np.ones(card, dtype=LD)
    for vs, t in [((v,), unary[v]) for v in range(n)] + list(factors):
        tt = np.transpose(np.asarray(t, dtype=LD), np.argsort(vs))  # axes in ascending node order
        joint = joint * tt.reshape([card[v] if v in vs else 1 for v in range(n)])
    z = joint.sum()
    marg = [joint.sum(axis=tuple(u for u in range(n) if u != v)) / z for v in range(n)]
    fbel = []
    for vs, _ in factors:
        m = joint.sum(axis=tuple(u for u in range(n) if u not in vs)) / z  # axes in ascending node order
        fbel.append(np.transpose(m, np.argsort(np.argsort(vs))).ravel())
    return np.concatenate(marg), np.concatenate(fbel), np.log(z)


@functools.lru_cache(maxsize=None)
def figure(name, n_iter, damping=0.0):
    """(longdouble run at this damping, the case's figure: the largest float64-against-longdouble difference of the
    restatement's messages over the iterations, marginals, factor beliefs and log Z, over the case's runs without and
    with damping 0.5).  One figure per case: a single run's log Z can round to the longdouble value by luck."""
    gaps, his = [], {}
    for lam in (0.0, 0.5):
        lo, hi = run(CASES[name], n_iter, 0.0, lam), run(CASES[name], n_iter, 0.0, lam, dtype=LD)
        his[lam] = hi
        gaps += [np.abs(a[0] - b[0]).max() for a, b in zip(lo["trace"], hi["trace"]) if a[0].size]
        gaps += [np.abs(lo[k] - hi[k]).max() for k in ("marginals", "factor_beliefs") if lo[k].size]
        gaps.append(abs(lo["logz"] - hi["logz"]))
    return his[damping], float(max(gaps))


def make(card, scopes, seed, zero_at=None):
    """Random node terms in [0.5, 1.5] and tables in [0.5, 2]; zero_at = (factor, flat cell) puts a zero there."""
    rng = np.random.default_rng(seed)
    unary = [rng.uniform(0.5, 1.5, k) for k in card]
    factors = [(vs, rng.uniform(0.5, 2.0, [card[v] for v in vs])) for vs in scopes]
    if zero_at:
        factors[zero_at[0]][1].ravel()[zero_at[1]] = 0.0
    return card, unary, factors


# trees and their diameter: loopy BP is exact after diameter + 1 iterations (one for the unary factors' messages)
TREES = {"chain": 2, "star": 2, "triple": 2}
CASES = {
    "chain": make([2, 3, 2], [(0, 1), (2, 1), (0,), (2,)], 1),
    # centre 0 with leaves 1, 2, 3; node 4 has only its own term and a unary factor, node 5 only its own term
    "star": make([3, 2, 4, 2, 3, 2], [(0, 1), (2, 0), (0, 3), (1,), (0,), (4,)], 2),
    "triple": make([2, 3, 2, 3], [(1, 0, 2), (2, 3), (3,), (0,)], 3, zero_at=(0, 4)),
    "grid_2x3": make([2, 3, 2, 3, 2, 3], grid_edges(2, 3) + [(0,), (5,)], 4),
    "grid_6x6": make([3] * 36, grid_edges(6, 6), 5),
    "pair_70": make([70, 70], [(0, 1)], 6),
    "chain_120": make([120] * 3, [(0, 1), (1, 2)], 7),
}
CONTRADICTION = ([2, 2], [np.ones(2), np.ones(2)], [((0, 1), np.array([[0.0, 0.0], [1.0, 1.0]]))])
BATCH_TOL = 1e-6


@functools.lru_cache(maxsize=None)
def batch():
    """(node terms [5, 15] of the 2 x 3 grid, the float64 restatement of every row at BATCH_TOL and 40 iterations).  Row
    2 is one-hot on every node and stops after 2 iterations, row 0 after 7, the others after 8.  No residual of any
    row lies within a factor 2 of BATCH_TOL, so the rounding of another implementation cannot move a count."""
    case = CASES["grid_2x3"]
    un = np.random.default_rng(28).uniform(0.5, 1.5, (5, sum(case[0])))
    un[2] = np.concatenate([np.eye(k)[0] for k in case[0]])
    refs = [run((case[0], np.split(row, np.cumsum(case[0])[:-1]), case[2]), 40, BATCH_TOL) for row in un]
    assert all(not BATCH_TOL / 2 <= t[1] <= BATCH_TOL * 2 for r in refs for t in r["trace"])
    assert [r["n_iter"] for r in refs] == [7, 8, 2, 8, 8]
    return un, refs
