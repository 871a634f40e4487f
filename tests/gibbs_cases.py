"""Gibbs sampling restated in numpy, independently of the C++ (pgmpy_amd/csrc/pgm_sample.h, pgmgibbs.hip),
and the cases the CPU and GPU tests share.

The stream: the uniform of chain r, code column c and sweep j is Philox4x32-10 with counter
(r & 0xffffffff, r >> 32, c >> 1, j) and the forward sampler's key, word choice and 53-bit conversion
(tests/sample_cases.py); sweep 0 is the forward sampler's stream.

The sweep: columns in ascending order; a clamped column keeps its code.  For a column of cardinality K,
w_s is the product over its incident factors, in ascending factor order and starting from the first
factor's value, of the factor's entry at the chain's current codes with the column at s; running sums in
state order; with t = u * c_{K-1} the new code is min{s : c_s > t}, else min{s : c_s == c_{K-1}}.  Every
product and sum is a plain fp64 array operation, so each is rounded separately.  A conditional whose total
is not finite or not > 0 leaves the code and is reported; a chain holding a code that is not a state is
not advanced and is reported.
"""
import functools

import numpy as np

from tests import sample_cases as S
from tests.sample_cases import LO32, S32, philox4x32_10, running_sums, select


# ---------------------------------------------------------------------------- the stream
def uniform3_bits(seed, chains, col, sweep):
    """The 53-bit integers behind the uniforms of chains `chains` (uint64 array), column `col`, sweep `sweep`."""
    chains = np.asarray(chains, dtype=np.uint64)
    seed = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    zero = np.zeros_like(chains)
    x = philox4x32_10((chains & LO32, chains >> S32, zero + np.uint64(int(col) >> 1), zero + np.uint64(int(sweep))),
                      (seed & LO32, seed >> S32))
    hi, lo = (x[2], x[3]) if int(col) & 1 else (x[0], x[1])
    return (hi << np.uint64(21)) | (lo >> np.uint64(11))


def uniforms3(seed, chains, col, sweep):
    return uniform3_bits(seed, chains, col, sweep).astype(np.float64) * 2.0 ** -53  # < 2^53: exact


# ---------------------------------------------------------------------------- the sweep
def incident(factors, n_cols):
    """Per column: [(factor, position of the column in it)], factors ascending."""
    inc = [[] for _ in range(n_cols)]
    for f, (cols, _) in enumerate(factors):
        for pos, c in enumerate(cols):
            inc[c].append((f, pos))
    return inc


def strides(cards):
    out, size = [0] * len(cards), 1
    for v in range(len(cards) - 1, -1, -1):
        out[v] = size
        size *= int(cards[v])
    return out


def conditional(factors, tables, inc_c, codes, K):
    """[K, n] weights of one column for every chain: the product of the incident factors' entries."""
    w = None
    for f, pos in inc_c:
        cols, cards = factors[f]
        st = strides(cards)
        base = np.zeros(codes.shape[1], dtype=np.int64)
        for v, c in enumerate(cols):
            if v != pos:
                base = base + codes[c].astype(np.int64) * st[v]
        flat = np.asarray(tables[f], dtype=np.float64).reshape(-1)
        val = flat[base[None, :] + (np.arange(K, dtype=np.int64) * st[pos])[:, None]]
        w = val if w is None else w * val  # one rounded fp64 multiplication per factor
    return w


def gibbs_ref(factors, tables, card, codes, n_sweeps, seed=0, first_chain=0, first_sweep=1, clamp=None, explicit=None,
              thin=None):
    """(codes [n_cols, n] uint8 after the sweeps, records: the states after every thin-th local sweep,
    undrawn: a conditional had no drawable total, bad: a chain held a code that is not a state).

    codes: uint8 [n_cols, n], the start states; explicit: fp64 [n_sweeps, n_cols, n] uniforms that replace
    the generator."""
    codes = np.array(codes, dtype=np.uint8)
    n_cols, n = codes.shape
    assert n_cols == len(card)
    inc = incident(factors, n_cols)
    live = (codes < np.asarray(card, dtype=np.int64)[:, None]).all(axis=0)
    bad = bool((~live).any())
    chains = np.uint64(first_chain) + np.arange(n, dtype=np.uint64)[live]
    cur = codes[:, live]
    undrawn = False
    records = []
    for j in range(1, n_sweeps + 1):
        sweep = first_sweep + j - 1
        for c in range(n_cols):
            if clamp is not None and clamp[c]:
                continue
            K = int(card[c])
            w = conditional(factors, tables, inc[c], cur, K)
            cdf = running_sums(w)  # one rounded fp64 addition per state
            u = np.asarray(explicit[j - 1, c], dtype=np.float64)[live] if explicit is not None else uniforms3(seed, chains, c, sweep)
            total = cdf[-1]
            ok = (total > 0) & np.isfinite(total)
            undrawn |= bool((~ok).any())
            with np.errstate(invalid="ignore"):
                new = select(cdf, u)
            cur[c] = np.where(ok, new, cur[c]).astype(np.uint8)
        if thin and j % thin == 0:
            rec = codes.copy()
            rec[:, live] = cur
            records.append(rec)
    out = codes.copy()
    out[:, live] = cur
    return out, records, undrawn, bad


def start_ref(card, n, seed=0, first_chain=0):
    """The start state of a model that cannot be forward-sampled: floor(u * card) from the sweep-0 uniform."""
    chains = np.uint64(first_chain) + np.arange(n, dtype=np.uint64)
    out = np.empty((len(card), n), dtype=np.uint8)
    for c, K in enumerate(card):
        out[c] = np.minimum((uniforms3(seed, chains, c, 0) * float(K)).astype(np.int64), K - 1)
    return out


# ---------------------------------------------------------------------------- models
def bn_factors(model):
    """(nodes, factors, tables, card) of a Bayesian network: the forward sampler's plan (columns sorted, CPD
    factors [node, parents...] in topological order) and the cardinality of every column."""
    nodes, order, fams, tables = S.model_plan(model)
    card = [0] * len(nodes)
    for cols, cards in fams:
        card[cols[0]] = int(cards[0])
    return nodes, fams, tables, card


def triangle_model():
    """A triangle Markov network with cardinalities 2, 3, 2 and positive potentials."""
    from pgmpy_amd.factors.discrete import DiscreteFactor
    from pgmpy_amd.models import DiscreteMarkovNetwork

    m = DiscreteMarkovNetwork([("A", "B"), ("B", "C"), ("A", "C")])
    m.add_factors(DiscreteFactor(["A", "B"], [2, 3], [1.0, 2.5, 0.7, 3.0, 0.4, 1.6]),
                  DiscreteFactor(["B", "C"], [3, 2], [0.9, 2.0, 1.5, 0.5, 2.2, 1.1]),
                  DiscreteFactor(["C", "A"], [2, 2], [1.3, 0.6, 0.8, 2.4]))
    return m


def mn_factors(model):
    nodes = sorted(model.nodes())
    col = {v: i for i, v in enumerate(nodes)}
    cardinality = model.get_cardinality()
    card = [int(cardinality[v]) for v in nodes]
    factors = [([col[u] for u in f.variables], [int(k) for k in f.cardinality]) for f in model.factors]
    tables = [np.array(f._values_readonly(), dtype=np.float64).reshape(-1) for f in model.factors]
    return nodes, factors, tables, card


def chain_network(n, seed=0):
    """An n-variable binary chain X0 -> X1 -> ... with random CPDs in [0.1, 0.9]: (factors, tables, card)."""
    rng = np.random.default_rng(seed)
    factors, tables = [([0], [2])], []
    p = rng.uniform(0.1, 0.9)
    tables.append(np.array([p, 1 - p]))
    for v in range(1, n):
        factors.append(([v, v - 1], [2, 2]))
        p = rng.uniform(0.1, 0.9, size=2)
        tables.append(np.array([p, 1 - p]).reshape(-1))
    return factors, tables, [2] * n


# ---------------------------------------------------------------------------- exact distribution
def joint_of_factors(factors, tables, card):
    """The normalised joint over the code columns (axis = column), by enumeration."""
    joint = np.ones(card, dtype=np.float64)
    for (cols, cards), table in zip(factors, tables):
        t = np.asarray(table, dtype=np.float64).reshape(cards)
        t = np.transpose(t, np.argsort(cols))
        expand = [1] * len(card)
        for c in cols:
            expand[c] = card[c]
        joint = joint * t.reshape(expand)
    return joint / joint.sum()


def sweep_matrix(joint, free):
    """The exact transition matrix of one systematic-scan sweep over the columns `free` (ascending) of a
    joint whose other axes were already sliced away: [states, states], row = from."""
    shape = joint.shape
    n = joint.size
    T = np.eye(n)
    idx = np.arange(n).reshape(shape)
    for c in free:
        cond = joint / joint.sum(axis=c, keepdims=True)  # p(x_c | rest)
        step = np.zeros((n, n))
        for s in range(shape[c]):
            # from any state to the state with x_c = s and the rest unchanged
            to = np.take(idx, [s], axis=c)
            to = np.broadcast_to(to, shape).reshape(-1)
            step[np.arange(n), to] = np.broadcast_to(np.take(cond, [s], axis=c), shape).reshape(-1)
        T = T @ step
    return T


def burn_in_for(joint, free, tol=1e-6, limit=4096):
    """The smallest B with max over start states of TV(T^B[start], posterior) < tol."""
    T = sweep_matrix(joint, free)
    pi = joint.reshape(-1)
    P = np.eye(joint.size)
    for b in range(1, limit + 1):
        P = P @ T
        if 0.5 * np.abs(P - pi[None, :]).sum(axis=1).max() < tol:
            return b
    raise AssertionError(f"the chain has not mixed after {limit} sweeps")


@functools.lru_cache(maxsize=None)
def hand_posterior():
    """hand_model() with D = d0: (nodes, factors, tables, card, posterior over A, B, C, burn-in B)."""
    nodes, fams, tables, card = bn_factors(S.hand_model())
    joint = joint_of_factors(fams, tables, card)[..., 0]
    joint = joint / joint.sum()
    return nodes, fams, tables, card, joint, burn_in_for(joint, [0, 1, 2])


@functools.lru_cache(maxsize=None)
def triangle_posterior():
    nodes, factors, tables, card = mn_factors(triangle_model())
    joint = joint_of_factors(factors, tables, card)
    return nodes, factors, tables, card, joint, burn_in_for(joint, [0, 1, 2])


N_DIST = 8192
SEED_DIST = 20261020


# ---------------------------------------------------------------------------- rounding and boundaries
def boundary_case(K, seed=0):
    """A variable of cardinality K (column 0) with four incident factors over it and three binary
    neighbours; full-mantissa random values, exact zeros at the first, a middle and the last state of the
    product: (factors, tables, card)."""
    rng = np.random.default_rng(seed)
    factors = [([0], [K]), ([0, 1], [K, 2]), ([2, 0], [2, K]), ([1, 0, 3], [2, K, 2]), ([1], [2]), ([2, 3], [2, 2])]
    tables = [rng.uniform(0.05, 1.0, size=int(np.prod(cards))) for _, cards in factors]
    t0 = tables[0]
    t0[0] = 0.0            # the first state
    t0[K // 2] = 0.0       # a middle state
    tables[1].reshape(K, 2)[K - 1, :] = 0.0  # the last state, through another factor
    return factors, tables, [K, 2, 2, 2]


def boundary_uniforms(factors, tables, card, codes1):
    """Explicit uniforms for column 0 of one chain state `codes1` [n_cols]: at every c_s / c_{K-1}, one ulp
    below it, one and two ulps above it, 0 and 1 - 2^-53."""
    inc = incident(factors, len(card))
    w = conditional(factors, tables, inc[0], np.asarray(codes1, dtype=np.uint8).reshape(-1, 1), card[0])
    cdf = running_sums(w)[:, 0]
    us = [0.0, 1.0 - 2.0 ** -53]
    for c in cdf:
        b = c / cdf[-1]
        up = np.nextafter(b, 1.0)
        for u in (b, np.nextafter(b, 0.0), up, np.nextafter(up, 1.0)):
            if 0.0 <= u < 1.0:
                us.append(float(u))
    return np.array(us, dtype=np.float64)
