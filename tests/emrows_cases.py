"""Shared by test_emrows_cpu.py and test_emrows_gpu.py: the case table of the rows E-step (pgm_fit_estep_rows),
its brute-force restatement in long double and the derived error bounds.

The restatement does NOT split a row's unobserved variables into components: it enumerates their full joint,
multiplies EVERY family of the plan, normalises, adds the weights to the touched families and takes
loglik = log of the sum.  So the factorisation the kernel relies on is itself under test.  A family is
(columns, cardinalities), the node first; the flat layout is tests/em_cases.layout's.
"""
import functools

import numpy as np

from tests.em_cases import FLOOR, MISSING, finish_ref, layout


def _chain(cards, order=None):
    """X0 -> X1 -> ...; order[i] is the code column of Xi."""
    o = list(range(len(cards))) if order is None else order
    return [([o[0]], [cards[0]])] + [([o[i], o[i - 1]], [cards[i], cards[i - 1]]) for i in range(1, len(cards))]


def _stars(sizes):
    fam, roots = [], []
    for k in sizes:
        roots.append(len(fam))
        fam += [([roots[-1]], [2])] + [([roots[-1] + 1 + i, roots[-1]], [2, 2]) for i in range(k)]
    return fam, roots


_ABC = _chain([2, 3, 2])
_LATENT = [([4], [3]), ([0, 4], [2, 3]), ([1, 4], [3, 3]), ([2, 4], [2, 3]), ([3, 0], [2, 2])]  # H (column 4) -> A, B, C; A -> D
_BAYES = [([0], [2])] + [([i, 0], [2, 2]) for i in range(1, 14)]
_STARS, _ROOTS = _stars(  # one root -> that many leaves each: (families, the roots' columns)
    [31, 32] + [26] * 5)
_EACH4 = [([c], 0.2) for c in range(4)]
# name: (families, rows, [(columns set missing together, share of the rows)], [(columns, one row) set missing], L: the
# largest component, options: latent, row0 / n_rows, skip (rows past a limit), tile (False: global-atomic tier), no_floor)
CASES = {
    "singleton": (_ABC, 200, [([1], 0.3)], [], 3, {}),
    "pair": (_ABC, 200, [([0, 1], 0.3)], [], 6, {}),
    "vstructure": ([([0], [2]), ([1], [3]), ([2, 0, 1], [2, 2, 3])], 200, [([0, 1], 0.4), ([2], 0.2)], [], 12, {}),  # A -> C <- B
    "disjoint": ([([0], [2]), ([1, 0], [3, 2]), ([2], [2]), ([3, 2], [4, 2])], 200, [([1, 3], 0.4)], [], 4, {}),
    # the smallest label (column 0) sits mid-path and travels three hops; row 0: every column missing
    "path6": (_chain([2] * 6, [5, 3, 1, 0, 2, 4]), 150, [([c], 0.3) for c in range(6)], [(range(6), 0)], 64, {}),
    "latent_missing": (_LATENT, 200, _EACH4, [], 36, dict(latent=[4])),
    "complete": (_ABC, 200, [], [], 1, {}),
    "mixed_radix": (_chain([2, 3, 5, 2]), 200, [([1, 2], 0.4), ([0], 0.2)], [], 30, {}),
    "ternary4": (_chain([3, 3, 3, 3, 2]), 100, [([0, 1, 2, 3], 0.5)], [], 81, {}),  # 81 configurations: lanes loop past 64
    # naive Bayes: class + 11 features missing is 4,096 configurations (counted), + 12 is 8,192 (skipped)
    "config_cap": (_BAYES, 6, [], [(range(12), 1), (range(12), 4), (range(13), 2)], 4096, dict(skip=(2,))),
    # 32 families in a component (counted) / 33 (skipped); 108 touched families in a row (counted) / 135 (skipped)
    "family_caps": (_STARS, 4, [], [(_ROOTS[:1], 0), (_ROOTS[1:2], 1), (_ROOTS[2:6], 2), (_ROOTS[2:], 3)], 2, dict(skip=(1, 3))),
    "chain70": (_chain([2] * 70), 64, [([c], 0.05) for c in range(70)], [], 8, {}),  # lanes stride past 64 columns; runs of <= 3
    "unobserved33": (_chain([2] * 70), 64, [([c], 0.05) for c in range(70)], [(range(33), 5)], 8, {}),
    "big_family": ([([i], [5]) for i in range(5)] + [([5, 0, 1, 2, 3, 4], [5] * 6)], 150,  # 5^6 bins: past the LDS tile
                   [([5], 0.25), ([0], 0.25), ([3], 0.25)], [], 125, dict(tile=False)),
    "window": (_LATENT, 208, _EACH4, [], 36, dict(latent=[4], row0=3, n_rows=200)),
    # P(B = 1 | A) = 0.  B = 1 where A is missing: Z_c = 0 without the floor.  Row 0: A seen, B = 1, C missing, so
    # the zero sits in B's family, which that row leaves untouched
    "zero_floor": (_chain([2, 2, 2]), 100, [([0], 0.5)], [], 2, dict(zero=True)),
    "zero_no_floor": (_chain([2, 2, 2]), 100, [([0], 0.5)], [], 2, dict(zero=True, no_floor=True)),
}
NAMES = tuple(CASES)


def cpds(families, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.dirichlet(np.full(cards[0], 2.0), size=int(np.prod(cards[1:], dtype=np.int64))).T.reshape(-1)
                           for _, cards in families])


@functools.lru_cache(maxsize=None)
def case(name):
    fam, n, blanks, cells, L, opt = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name.split("_")[0])))
    c = dict(dict(latent=[], row0=0, n_rows=n, no_floor=False, skip=(), tile=True), **opt)
    card = {col: k for cols, cards in fam for col, k in zip(cols, cards) if col not in c["latent"]}
    codes = np.stack([rng.integers(0, card[col], n) for col in range(len(card))]).astype(np.uint8)
    for cols, share in blanks:
        codes[np.ix_(list(cols), np.nonzero(rng.random(n) < share)[0])] = MISSING
    for cols, row in cells:
        codes[list(cols), row] = MISSING
    values = cpds(fam, 7)
    if opt.get("zero"):
        values[2:6] = [1.0, 1.0, 0.0, 0.0]
        codes[1, codes[0] != MISSING] = 0
        codes[:, 0] = [0, 1, MISSING]
    if c["row0"]:  # the rows around the window are not states
        codes[:, :c["row0"]], codes[:, c["row0"] + c["n_rows"]:] = 200, 200
    c.update(families=fam, values=values, codes=codes, L=L)
    return c


def brute_force(families, latent, values, codes, no_floor=False, skip=(), every_family=False, dtype=np.longdouble):
    """(tables, loglik [n], status [n], adds: the weights added per table entry, logsum [n]: an upper bound of
    sum |log term| per row).  every_family: the untouched families get the row's whole weight, 1, too."""
    offsets, sizes, strides = layout(families)
    card = {c: k for cols, cards in families for c, k in zip(cols, cards)}
    vals = np.asarray(values).astype(dtype)
    vals = vals if no_floor else np.maximum(vals, dtype(FLOOR))
    n = codes.shape[1]
    tables, adds = np.zeros(sum(sizes), dtype=dtype), np.zeros(sum(sizes))
    loglik, status, logsum = np.full(n, np.nan, dtype=dtype), np.zeros(n, dtype=np.uint8), np.zeros(n)
    for r in range(n):
        U = sorted(c for c in card if c in latent or codes[c, r] == MISSING)
        if any(c not in U and codes[c, r] >= card[c] for c in card):
            status[r] = 4
        if len(U) > 32 or r in skip:  # PGM_EMR_MAX_UNOBSERVED, or a cap the case names
            status[r] = 2
        if status[r]:
            continue
        grid = np.indices([card[u] for u in U]).reshape(len(U), -1) if U else np.zeros((0, 1), dtype=np.int64)
        p, entries = np.ones(grid.shape[1], dtype=dtype), []
        for f, (cols, _) in enumerate(families):
            e = offsets[f] + sum((grid[U.index(col)] if col in U else int(codes[col, r])) * st for col, st in zip(cols, strides[f]))
            e = np.broadcast_to(e, p.shape)
            p = p * vals[e]
            with np.errstate(divide="ignore"):
                logs = np.abs(np.log(vals[e].astype(np.float64)))
            logsum[r] += float(np.max(logs[np.isfinite(logs)], initial=0.0))
            if every_family or any(col in U for col in cols):
                entries.append(e)
        Z = p.sum()
        if Z == 0:
            status[r], loglik[r] = 3, -np.inf
            continue
        status[r], loglik[r] = (1 if U else 0), np.log(Z)
        for e in entries:
            np.add.at(tables, e, p / Z)
            np.add.at(adds, e, 1)
    return tables, loglik, status, adds, logsum


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    return brute_force(c["families"], c["latent"], c["values"], c["codes"][:, c["row0"]:c["row0"] + c["n_rows"]], c["no_floor"], c["skip"])


def atol(c, want, adds):
    """Per table entry: T weights are summed (adds: counted by the restatement over the full joint, so never fewer
    than the kernel's), each the quotient of a product of F factors and a sum of L terms taken as ceil(L / 64) per
    lane and a 6-step butterfly (64 covers it and the division): (T + F + ceil(L / 64) + 64) 2^-53 sum |term|, the
    terms being positive, so their sum is the entry itself."""
    return (adds + len(c["families"]) + -(-c["L"] // 64) + 64) * 2.0 ** -53 * np.abs(want)


def atol_loglik(c, logsum):
    """Per row: at most 2 F terms (a log per component and per untouched family) plus the ceil(L / 64) + 64 of a
    Z_c: (n_terms + 64) 2^-52 (1 + sum |log term|)."""
    return (2 * len(c["families"]) + -(-c["L"] // 64) + 64) * 2.0 ** -52 * (1.0 + logsum)


# ---------------------------------------------------------------------------- EM end to end
# H -> A, B; A -> C; B -> D (code columns A .. D = 0 .. 3, the latent H = 4), 300 rows, 20 % of the cells missing
EM_FAMILIES = [([4], [2]), ([0, 4], [2, 2]), ([1, 4], [3, 2]), ([2, 0], [2, 2]), ([3, 1], [2, 3])]
# max |em_ref(dtype=np.float64) - em_ref()| over the values after three iterations, both on the CPU; the device is
# allowed 64 x this, the rule of em_cases.GOLDEN_D
EM_FP64_VS_LONGDOUBLE = 3.48e-16


def em_problem():
    rng = np.random.default_rng(2026)
    codes = np.stack([rng.integers(0, k, 300) for k in (2, 3, 2, 2)]).astype(np.uint8)
    codes[rng.random(codes.shape) < 0.2] = MISSING
    return codes, cpds(EM_FAMILIES, 11)


def em_ref(families, latent, codes, values, iters, dtype=np.longdouble):
    """iters iterations of E-step (every family) and finish -> (values, [log-likelihood each iteration started from])."""
    values, lls = np.asarray(values).astype(dtype), []
    for _ in range(iters):
        tables, loglik, _, _, _ = brute_force(families, latent, values, codes, every_family=True, dtype=dtype)
        lls.append(loglik.sum())
        values = finish_ref(families, tables)
    return values, lls
