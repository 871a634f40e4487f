"""Shared by test_em_cpu.py and test_em_gpu.py (and by tests/golden/make_golden_em.py): a numpy restatement
of the E-step kernel (pgm_fit_estep) and of k iterations of ExpectationMaximization, the kernel case table,
the error bounds and the per-case tolerances of the golden pins.

A family is (columns, cardinalities), the node first; the flat layout is pgm_fit_plan_create's: families end
to end, each [node_card, prod(parent_card)] in C order.  Latent columns are virtual: `codes` has no row for
them.  Latent configuration l counts the latents' states in the order of `latent_cols`, the last fastest.
"""
import itertools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR = 1e-10  # PGM_EM_FLOOR
MISSING = 255  # PGM_EV_MISSING
RTOL = 1e-5    # np.allclose's rtol in TabularCPD.__eq__(atol=)


def layout(families):
    """(offsets, sizes, strides) of the flat buffers."""
    offsets, sizes, strides, off = [], [], [], 0
    for _, cards in families:
        st = [int(np.prod(cards[v + 1:], dtype=np.int64)) for v in range(len(cards))]
        size = int(np.prod(cards, dtype=np.int64))
        offsets.append(off), sizes.append(size), strides.append(st)
        off += size
    return offsets, sizes, strides


def total_bins(families):
    return sum(layout(families)[1])


def estep_ref(families, latent_cols, values, codes, dtype=np.longdouble):
    """What pgm_fit_estep adds to zeroed tables for the rows of codes [n_cols, n] (uint8), in `dtype`:
    (tables, loglik [n], counted [n] bool, bad: whether a code is neither missing nor a state)."""
    latent_cols = [int(c) for c in latent_cols]
    offsets, sizes, strides = layout(families)
    n = codes.shape[1]
    values = np.asarray(values).astype(dtype)
    counted = np.ones(n, dtype=bool)
    bad = False
    card_of = {}
    for cols, cards in families:
        for c, k in zip(cols, cards):
            if c in latent_cols:
                card_of[c] = k
            else:
                counted &= codes[c] < k
                bad |= bool(((codes[c] >= k) & (codes[c] != MISSING)).any())
    rows = np.nonzero(counted)[0]
    obs, lat_fams = [], []
    for f, (cols, cards) in enumerate(families):
        idx = np.zeros(len(rows), dtype=np.int64)
        for c, st in zip(cols, strides[f]):
            if c not in latent_cols:
                idx += codes[c, rows].astype(np.int64) * st
        obs.append(idx)
        if any(c in latent_cols for c in cols):
            lat_fams.append(f)
    configs = list(itertools.product(*[range(card_of[c]) for c in latent_cols]))
    entries = np.empty((len(configs), len(lat_fams), len(rows)), dtype=np.int64)
    P = np.empty((len(configs), len(rows)), dtype=dtype)
    for li, cfg in enumerate(configs):
        p = np.ones(len(rows), dtype=dtype)
        for k, f in enumerate(lat_fams):
            add = sum(cfg[latent_cols.index(c)] * st for c, st in zip(families[f][0], strides[f]) if c in latent_cols)
            entries[li, k] = offsets[f] + obs[f] + add
            p = p * np.maximum(values[entries[li, k]], dtype(FLOOR))
        P[li] = p
    Z = P.sum(axis=0)
    W = P / Z
    tables = np.zeros(sum(sizes), dtype=dtype)
    for li in range(len(configs)):
        for k in range(len(lat_fams)):
            np.add.at(tables, entries[li, k], W[li])
    ll = np.log(Z)
    for f in range(len(families)):
        if f not in lat_fams:
            np.add.at(tables, offsets[f] + obs[f], dtype(1))
            ll = ll + np.log(np.maximum(values[offsets[f] + obs[f]], dtype(FLOOR)))
    loglik = np.zeros(n, dtype=dtype)
    loglik[rows] = ll
    return tables, loglik, counted, bad


def finish_ref(families, tables, pseudo=None, bayes=False):
    """pgm_fit_finish | PGM_FIT_WEIGHTED: values = normalise(tables + pseudo) per CPD column."""
    offsets, sizes, _ = layout(families)
    out = np.empty_like(tables)
    for f, (_, cards) in enumerate(families):
        t = tables[offsets[f]:offsets[f] + sizes[f]].reshape(cards[0], -1)
        if pseudo is not None:
            t = t + pseudo[offsets[f]:offsets[f] + sizes[f]].reshape(cards[0], -1).astype(t.dtype)
        if not bayes:
            t = np.where((t == 0).all(axis=0, keepdims=True), np.ones_like(t), t)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[offsets[f]:offsets[f] + sizes[f]] = (t / t.sum(axis=0)).reshape(-1)
    return out


def allclose_excess(old, new):
    """max(|old - new| - RTOL |new|): the iteration has converged when this is <= atol."""
    old, new = np.asarray(old, dtype=np.float64), np.asarray(new, dtype=np.float64)
    return float(np.max(np.abs(old - new) - RTOL * np.abs(new)))


def em_ref(families, latent_cols, values, codes, max_iter, atol=None, pseudo=None, bayes=False, dtype=np.longdouble):
    """max_iter iterations of EM from `values` (fewer when atol is given and the iteration converges):
    (values, [log-likelihood the iteration started from], iterations run)."""
    values = np.asarray(values).astype(dtype)
    lls, n_iter = [], 0
    for _ in range(max_iter):
        tables, loglik, _, _ = estep_ref(families, latent_cols, values, codes, dtype=dtype)
        new = finish_ref(families, tables, None if pseudo is None else np.asarray(pseudo), bayes)
        lls.append(loglik.sum())
        done = atol is not None and allclose_excess(values, new) <= atol
        values, n_iter = new, n_iter + 1
        if done:
            break
    return values, lls, n_iter


def bound(n_rows, n_fam, L, T):
    """The error allowed in a table bin whose expected count is T.  Every term is non-negative, so a sum of
    n of them in any order is within (n - 1) 2^-53 relative; a weight costs n_fam multiplications, L
    additions and a division; the factor 2 covers rounding the long-double reference to fp64."""
    return (n_rows + n_fam + L + 8) * 2.0 ** -52 * T


def bound_loglik(n_fam, L, loglik):
    return (n_fam + L + 8) * 2.0 ** -52 * (1.0 + np.abs(np.asarray(loglik, dtype=np.float64)))


# ----------------------------------------------------------------------------- the kernel cases
# name -> (families, latent_cols, n_rows); columns 0 .. n_obs - 1 are observed, the latents follow.
def _chain(n_lat, card):
    """n_lat latents of `card` states in a chain, each with one observed binary child."""
    fams = []
    for j in range(n_lat):
        fams.append(([n_lat + j] + ([n_lat + j - 1] if j else []), [card] + ([card] if j else [])))
        fams.append(([j, n_lat + j], [2, card]))
    return fams, list(range(n_lat, 2 * n_lat))


def kernel_cases():
    cases = {}
    one = ([([2], [3]), ([0, 2], [2, 3]), ([1, 2, 0], [3, 3, 2])], [2])  # H; X0 | H; X1 | H, X0
    for n in (1, 3, 4, 255, 256, 257, 4096, 4097):
        cases[f"rows{n}"] = (*one, n)
    cases["one_child"] = ([([1], [4]), ([0, 1], [3, 4])], [1], 300)
    cases["shared_child"] = ([([2], [3]), ([3], [2]), ([0, 2, 3], [3, 3, 2]), ([1, 2], [2, 3])], [2, 3], 300)
    cases["latent_parent"] = ([([2], [2]), ([3, 2], [3, 2]), ([0, 3], [2, 3]), ([1, 3, 0], [3, 3, 2])], [2, 3], 300)
    # column 2 has an observed child, column 3 (a child of column 2 and of the observed column 1) has none
    cases["no_observed_child"] = ([([2], [3]), ([3, 2, 1], [2, 3, 2]), ([0, 2], [2, 3]), ([1], [2])], [2, 3], 300)
    cases["three_latents"] = ([([3], [3]), ([4], [2]), ([5, 3], [4, 3]), ([0, 3, 4], [2, 3, 2]), ([1, 5], [3, 4]),
                               ([2, 4, 5], [2, 2, 4])], [3, 4, 5], 300)
    cases["eight_latents"] = (*_chain(8, 2), 300)
    cases["configs4096"] = (*_chain(4, 8), 5)
    # 32 families with a latent: the latent's own and 31 children; one more family without
    cases["families32"] = ([([32], [2])] + [([j, 32], [2, 2]) for j in range(31)] + [([31], [3])], [32], 300)
    # two families of 2,940 bins: two LDS groups; the second latent family is in the second group
    cases["two_groups"] = ([([4], [3]), ([0, 4, 1, 2], [5, 3, 14, 14]), ([3, 4, 1, 2], [5, 3, 14, 14])], [4], 600)
    # 5,880 bins: the global path, beside a tile group
    cases["global_family"] = ([([4], [3]), ([0, 4, 1, 2, 3], [5, 3, 14, 14, 2]), ([3, 4], [2, 3])], [4], 600)
    cases["mixed"] = ([([0], [2]), ([4], [3]), ([1, 0], [3, 2]), ([2, 4, 0], [2, 3, 2]), ([5, 4], [2, 3]),
                       ([3, 5, 1], [3, 2, 3])], [4, 5], 700)
    return cases


def case_inputs(name, seed=0, row0=0, pad=0):
    """(families, latent_cols, values, codes [n_obs, row0 + n + pad]) of a kernel case: positive random CPD
    values, uniform random codes."""
    families, latent_cols, n = kernel_cases()[name]
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    values = np.concatenate([finish_ref([fam], rng.random(total_bins([fam])) + 0.05) for fam in families])
    card = {}
    for cols, cards in families:
        card.update({c: k for c, k in zip(cols, cards) if c not in latent_cols})
    n_obs = max(card) + 1 if card else 1
    assert all(c >= n_obs for c in latent_cols)
    codes = np.zeros((n_obs, row0 + n + pad), dtype=np.uint8)
    for c, k in card.items():
        codes[c] = rng.integers(0, k, size=codes.shape[1])
    return families, latent_cols, values, codes


# ----------------------------------------------------------------------------- the goldens
# d: the largest difference between em_ref in plain fp64 and the reference's CPDs over every recorded
# iteration count of the case, measured when the goldens were generated; the pins allow 64 d.
GOLDEN_D = {
    "a": 1.121e-14,  # 100 iterations (never stops: the excess is 4.2e-3 at iteration 100)
    "b": 1.082e-14,  # 100 iterations (1.4e-3)
    "c": 5.551e-16,  # stops at iteration 2
    "d": 6.553e-14,  # 100 iterations (9.6e-3)
}


def golden_tolerance(case):
    tol = 64 * GOLDEN_D[case]
    assert tol <= 1e-10, f"case {case} is ill-conditioned"
    return tol


def load_golden():
    with open(os.path.join(GOLDEN, "em_cases.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "em_cases.npz"))


def golden_problem(meta, arrays, case):
    """A golden EM case as the restatement reads it: (nodes of the plan, families, latent_cols, initial
    values, codes, pseudo or None).  Observed node i of meta['observed'] is code column i."""
    c = meta[case]
    observed, latents = c["observed"], c["latents"]
    col_of = {v: j for j, v in enumerate(observed + latents)}
    card = dict(c["cardinality"])
    nodes = c["em_nodes"]
    families = [([col_of[v] for v in [n] + c["parents"][n]], [card[v] for v in [n] + c["parents"][n]]) for n in nodes]
    values = arrays[f"{case}_init"]
    pseudo = arrays[f"{case}_pseudo"] if f"{case}_pseudo" in arrays.files else None
    return nodes, families, [col_of[v] for v in latents], values, arrays[f"{c['frame']}_codes"], pseudo
