"""The per-row log-probability restated in numpy long double, independently of the C++
(pgmpy_amd/csrc/pgmlogp.hip, pgmfit_plan.cpp), and the plans the CPU and GPU tests share.

Per row: log in np.longdouble of every family's entry, added in plan order in np.longdouble, rounded once
to fp64.  A row that holds 255 (missing) or any other code >= its cardinality in a column a family reads
is NaN ("skipped").

The total, bit for bit (`total_fixed_order`): the device adds the fp64 row values it wrote, a skipped row
counting +0.0.  With R = 1024 rows per workgroup and B = 256 work-items: workgroup b holds the window's
rows [b R, (b + 1) R), padded with +0.0; work-item t adds its rows t, t + B, t + 2 B, t + 3 B in that order;
a tree adds the work-items' sums (w = B / 2, B / 4 .. 1: item t < w adds item t + w).  The block partials,
padded with +0.0 to a multiple of B, are added the same way: work-item t adds the partials t, t + B, ...
in index order, then the same tree.  Every addition is one fp64 addition.

The tolerance of a device row against the long-double sum (`row_bound`): n_fam * 2^-52 * sum_f |log theta_f|.
One ulp per device logarithm gives at most 2^-52 sum |l_f|; the n_fam - 1 additions of the running sum
give at most (n_fam - 1) 2^-53 sum |l_f| (each partial sum is at most sum |l_f|); together
(n_fam + 1) / 2 * 2^-52 sum |l_f| <= n_fam 2^-52 sum |l_f|.  The long-double sum's own error (2^-64
relative per operation) is far below that.  Against fp64 values that were themselves rounded (the
reference's recorded ones) the tests use twice the bound.
"""
import functools

import numpy as np

MISSING = 255
BLOCK, ROWS_PER_BLOCK = 256, 1024
EPS52 = 2.0 ** -52


def flat_values(tables):
    return np.concatenate([np.asarray(t, dtype=np.float64).ravel() for t in tables])


def normalized(tables):
    """Every column [card, parent configurations] divided by its total in fp64, the state-order sum: what
    BayesianModelProbability (and the reference's _reduce_marg) does before the logarithm."""
    out = []
    for t in tables:
        t = np.asarray(t, dtype=np.float64)
        total = np.zeros(t.shape[1], dtype=np.float64)
        for s in range(t.shape[0]):
            total = total + t[s]
        out.append(t / total)
    return out


def family_index(cols, cards, codes):
    """(flat index into the family's table [card, parents in C order], rows that hold a code that is no state)."""
    idx = np.zeros(codes.shape[1], dtype=np.int64)
    bad = np.zeros(codes.shape[1], dtype=bool)
    for c, k in zip(cols, cards):
        x = codes[c].astype(np.int64)
        bad |= x >= int(k)
        idx = idx * int(k) + np.where(x >= int(k), 0, x)
    return idx, bad


def restate(families, tables, codes):
    """(fp64 row values, NaN where skipped; the long-double sums they were rounded from; long-double
    sum_f |log theta_f| per row; skipped mask; whether a code was neither a state nor 255)."""
    codes = np.asarray(codes, dtype=np.uint8)
    n = codes.shape[1]
    acc = np.zeros(n, dtype=np.longdouble)
    mag = np.zeros(n, dtype=np.longdouble)
    skipped = np.zeros(n, dtype=bool)
    invalid = False
    for (cols, cards), table in zip(families, tables):
        t = np.asarray(table, dtype=np.float64).ravel()
        idx, bad = family_index(cols, cards, codes)
        for c, k in zip(cols, cards):
            invalid |= bool(((codes[c] >= int(k)) & (codes[c] != MISSING)).any())
        with np.errstate(divide="ignore"):
            lg = np.log(t.astype(np.longdouble))[idx]
        acc = acc + lg
        mag = mag + np.abs(lg)
        skipped |= bad
    out = acc.astype(np.float64)
    out[skipped] = np.nan
    return out, acc, mag, skipped, invalid


def row_bound(n_fam, mag):
    return n_fam * EPS52 * np.asarray(mag, dtype=np.longdouble)


def _tree(v):
    """The workgroup's fixed tree over BLOCK fp64 values (a copy is folded in halves)."""
    v = np.array(v, dtype=np.float64)
    w = BLOCK // 2
    while w > 0:
        v[:w] = v[:w] + v[w:2 * w]
        w //= 2
    return v[0]


def _strided(v):
    """Work-item t adds v[t], v[t + BLOCK], ... in index order (v padded with +0.0), then the tree."""
    v = np.asarray(v, dtype=np.float64)
    pad = -len(v) % BLOCK
    v = np.concatenate([v, np.zeros(pad)]).reshape(-1, BLOCK)
    acc = v[0].copy()
    for k in range(1, v.shape[0]):
        acc = acc + v[k]
    return _tree(acc)


def total_fixed_order(row_values):
    """The device's total of a window's fp64 row values (NaN = skipped), bit for bit (module docstring)."""
    v = np.asarray(row_values, dtype=np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    with np.errstate(invalid="ignore"):
        parts = [_strided(np.concatenate([v[b:b + ROWS_PER_BLOCK], np.zeros(-len(v[b:b + ROWS_PER_BLOCK]) % ROWS_PER_BLOCK)]))
                 for b in range(0, len(v), ROWS_PER_BLOCK)]
        return np.float64(_strided(parts)) if parts else np.float64(0.0)


# ---------------------------------------------------------------------------- plans
def random_tables(families, rng, zeros=0.0):
    tables = []
    for cols, cards in families:
        t = rng.random((cards[0], int(np.prod(cards[1:], dtype=np.int64)))) + 0.05
        if zeros:
            t[rng.random(t.shape) < zeros] = 0.0
            t[0, t.sum(axis=0) == 0] = 1.0
        tables.append(t / t.sum(axis=0, keepdims=True))
    return tables


def random_codes(families, n, rng, n_cols=None):
    """uint8 [n_cols, n]: every column uniform over its states (a column's cardinality is the one its
    families give it)."""
    card = {}
    for cols, cards in families:
        for c, k in zip(cols, cards):
            assert card.setdefault(c, int(k)) == int(k)
    n_cols = 1 + max(card) if n_cols is None else n_cols
    codes = np.zeros((n_cols, n), dtype=np.uint8)
    for c, k in card.items():
        codes[c] = rng.integers(0, k, size=n)
    return codes


PLANS = ["single", "max_parents", "card_1", "card_254", "chain_300", "alarm", "zeros"]


@functools.lru_cache(maxsize=None)
def plan(name):
    """(families, tables) of a named plan.  A node with PGM_MAX_DIMS - 1 = 31 BINARY parents cannot exist: its
    table would have 2^32 entries, past the 2^31 - 1 the fit plan's layout allows (tests/test_sample_gpu.py);
    max_parents has 31 parents of which 12 are binary and 19 have one state."""
    rng = np.random.default_rng(17)
    if name == "single":
        fams = [([0], [3])]
    elif name == "max_parents":
        cards = [2] * 12 + [1] * 19
        order = rng.permutation(31)
        fams = [([int(v)], [cards[v]]) for v in range(31)]
        fams.append(([31] + [int(v) for v in order], [3] + [cards[v] for v in order]))
    elif name == "card_1":
        fams = [([0], [1]), ([1, 0], [4, 1]), ([2, 1, 0], [1, 4, 1]), ([3, 2], [3, 1])]
    elif name == "card_254":
        fams = [([1], [3]), ([0, 1], [254, 3]), ([2, 0], [2, 254])]
    elif name == "chain_300":
        cards = [int(k) for k in rng.integers(2, 5, size=300)]
        cols = [int(c) for c in rng.permutation(300)]
        fams = [([cols[0]], [cards[0]])]
        fams += [([cols[i], cols[i - 1]], [cards[i], cards[i - 1]]) for i in range(1, 300)]
    elif name == "alarm":
        from pgmpy_amd.utils import get_example_model

        from tests import sample_cases as S

        _, _, fams, tables = S.model_plan(get_example_model("alarm"))
        return fams, tables
    elif name == "zeros":  # exact zeros in a third of the cells
        fams = [([2], [3]), ([0, 2], [4, 3]), ([1, 0, 2], [5, 4, 3])]
        return fams, random_tables(fams, rng, zeros=0.34)
    else:
        raise KeyError(name)
    return fams, random_tables(fams, rng)
