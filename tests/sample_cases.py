"""Forward sampling restated in numpy, independently of the C++ (pgmpy_amd/csrc/pgm_sample.h,
pgmsample.hip), and the cases the CPU and GPU tests share.

The stream: the uniform of stream row r and code column c is Philox4x32-10 with counter
(r & 0xffffffff, r >> 32, c >> 1, 0) and key (seed & 0xffffffff, seed >> 32); words (x0, x1) for an even
column, (x2, x3) for an odd one; u = ((hi << 21) | (lo >> 11)) * 2^-53.  Integer parts are uint64.

The sampler: families in plan order, each ``(columns, cardinalities)`` (node first, then the parents in
the CPD's order) with its values ``[card, parent configurations]``.  Running sums in state order; with
t = u * c_{K-1} the state is min{s : c_s > t}, else min{s : c_s == c_{K-1}}.  Modes 0 FREE, 1 GIVEN,
2 OBSERVED (the weight is multiplied by value / column total, in np.longdouble); a given 255 is drawn; a
given code that is not a state kills the row (later nodes 255, weight 0) and is reported.
"""
import numpy as np

MISSING = 255
FREE, GIVEN, OBSERVED = 0, 1, 2
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
LO32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

KNOWN_ANSWERS = [  # counter, key -> output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """Four uint64 arrays (values < 2^32) from counter words c0..c3 and key words k0, k1 (array-likes)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & LO32 for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & LO32 for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & LO32, (p0 >> S32) ^ c3 ^ k1, p0 & LO32
        k0, k1 = (k0 + W0) & LO32, (k1 + W1) & LO32
    return c0, c1, c2, c3


def uniform_bits(seed, rows, col):
    """The 53-bit integers behind the uniforms of stream rows `rows` (uint64 array) and code column `col`."""
    rows = np.asarray(rows, dtype=np.uint64)
    seed = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    zero = np.zeros_like(rows)
    x = philox4x32_10((rows & LO32, rows >> S32, zero + np.uint64(int(col) >> 1), zero), (seed & LO32, seed >> S32))
    hi, lo = (x[2], x[3]) if int(col) & 1 else (x[0], x[1])
    return (hi << np.uint64(21)) | (lo >> np.uint64(11))


def uniforms(seed, rows, col):
    return uniform_bits(seed, rows, col).astype(np.float64) * 2.0 ** -53  # < 2^53: exact


def running_sums(table):
    """[card, columns] running sums in state order, one fp64 addition per state."""
    table = np.asarray(table, dtype=np.float64)
    out = np.empty_like(table)
    acc = np.zeros(table.shape[1], dtype=np.float64)
    for s in range(table.shape[0]):
        acc = acc + table[s]
        out[s] = acc
    return out


def select(cdf_cols, u):
    """The state of each row: cdf_cols [card, n] (the row's own column), u [n]."""
    total = cdf_cols[-1]
    t = u * total
    above = cdf_cols > t[None, :]
    return np.where(above.any(axis=0), above.argmax(axis=0), (cdf_cols == total[None, :]).argmax(axis=0))


def sample_ref(families, tables, n_rows, seed=0, first_row=0, n_cols=None, given=None, modes=None, explicit=None,
               weights=False):
    """(codes [n_cols, n_rows] uint8, weights longdouble or None, bad: a given code was not a state).

    given: uint8 [n_cols, n_rows], the buffer's content before the call (read in GIVEN / OBSERVED columns);
    explicit: fp64 [n_cols, n_rows] uniforms that replace the generator."""
    n_cols = 1 + max(c for cols, _ in families for c in cols) if n_cols is None else n_cols
    codes = np.full((n_cols, n_rows), MISSING, dtype=np.uint8) if given is None else np.array(given, dtype=np.uint8)
    modes = [FREE] * len(families) if modes is None else list(modes)
    w = np.ones(n_rows, dtype=np.longdouble)
    dead = np.zeros(n_rows, dtype=bool)
    rows = np.uint64(first_row) + np.arange(n_rows, dtype=np.uint64)
    for (cols, cards), table, mode in zip(families, tables, modes):
        card = int(cards[0])
        table = np.asarray(table, dtype=np.float64).reshape(card, -1)
        cdf = running_sums(table)
        col = np.zeros(n_rows, dtype=np.int64)
        for c, k in zip(cols[1:], cards[1:]):
            col = col * int(k) + codes[c]
        col[dead] = 0
        assert dead.all() or col[~dead].max(initial=0) < table.shape[1]
        g = codes[cols[0]].astype(np.int64) if mode != FREE else np.full(n_rows, MISSING, dtype=np.int64)
        u = np.asarray(explicit[cols[0]], dtype=np.float64) if explicit is not None else uniforms(seed, rows, cols[0])
        drawn = select(cdf[:, col], u)
        bad = ~dead & (g != MISSING) & (g >= card)
        ok = ~dead & (g < card)
        out = np.where(g == MISSING, drawn, g)
        if weights and mode == OBSERVED and ok.any():
            w[ok] *= table[g[ok], col[ok]].astype(np.longdouble) / cdf[-1, col[ok]].astype(np.longdouble)
        dead_before = dead
        dead = dead | bad
        w[bad] = 0
        out = np.where(dead_before, MISSING, out)
        codes[cols[0]] = out.astype(np.uint8)
    return codes, (w if weights else None), bool(dead.any())


# ---------------------------------------------------------------------------- models
def model_plan(model, nodes=None):
    """(nodes, plan order, families, tables) of a model: columns sorted(model.nodes()) unless given; the
    order is topological with ties broken by column; a family lists the CPD's own variable order."""
    import networkx as nx

    nodes = sorted(model.nodes()) if nodes is None else list(nodes)
    col = {v: i for i, v in enumerate(nodes)}
    order = list(nx.lexicographical_topological_sort(model, key=col.__getitem__))
    families, tables = [], []
    for v in order:
        cpd = model.get_cpds(v)
        families.append(([col[u] for u in cpd.variables], [int(k) for k in cpd.cardinality]))
        tables.append(np.array(cpd._values_readonly(), dtype=np.float64).reshape(int(cpd.cardinality[0]), -1))
    return nodes, order, families, tables


def frame_of(model, codes, nodes, columns=None):
    """State names of codes [n_nodes, n]; columns default to model.nodes() order."""
    import pandas as pd

    states = model.states
    pos = {v: i for i, v in enumerate(nodes)}
    columns = list(model.nodes()) if columns is None else list(columns)
    data = {}
    for v in columns:
        lut = np.empty(len(states[v]), dtype=object)
        lut[:] = list(states[v])
        data[v] = lut[codes[pos[v]]]
    return pd.DataFrame(data, columns=columns)


def hand_model():
    """A -> C <- B, C -> D: 2 x 3 x 2 x 3 = 36 joint cells, each of probability >= 0.0032."""
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.models import DiscreteBayesianNetwork

    m = DiscreteBayesianNetwork([("A", "C"), ("B", "C"), ("C", "D")])
    m.add_cpds(
        TabularCPD("A", 2, [[0.6], [0.4]], state_names={"A": ["a0", "a1"]}),
        TabularCPD("B", 3, [[0.5], [0.3], [0.2]], state_names={"B": ["b0", "b1", "b2"]}),
        TabularCPD("C", 2, [[0.7, 0.4, 0.2, 0.5, 0.8, 0.3], [0.3, 0.6, 0.8, 0.5, 0.2, 0.7]], evidence=["A", "B"],
                   evidence_card=[2, 3], state_names={"C": ["c0", "c1"], "A": ["a0", "a1"], "B": ["b0", "b1", "b2"]}),
        TabularCPD("D", 3, [[0.2, 0.5], [0.3, 0.3], [0.5, 0.2]], evidence=["C"], evidence_card=[2],
                   state_names={"D": ["d0", "d1", "d2"], "C": ["c0", "c1"]}),
    )
    return m


def joint_of(families, tables, shape):
    """The joint distribution over the code columns (axis = column), by enumeration."""
    joint = np.ones(shape, dtype=np.float64)
    for (cols, cards), table in zip(families, tables):
        t = np.asarray(table, dtype=np.float64).reshape(cards)
        t = t / t.sum(axis=0, keepdims=True)
        expand = [1] * len(shape)
        perm = np.argsort(cols)
        t = np.transpose(t, perm)
        for c in cols:
            expand[c] = shape[c]
        joint = joint * t.reshape(expand)
    return joint


def six_sigma_cells(codes, joint, n):
    """Every joint cell count within 6 sqrt(N p (1 - p)) of N p; returns the worst ratio."""
    shape = joint.shape
    flat = np.ravel_multi_index(tuple(codes[c].astype(np.int64) for c in range(len(shape))), shape)
    counts = np.bincount(flat, minlength=joint.size).reshape(shape)
    p = joint
    dev = np.abs(counts - n * p) / np.sqrt(n * p * (1 - p))
    return float(dev.max())


# the selection rule at the boundaries of the running sums: (name, probabilities of one column)
BOUNDARY_COLUMNS = [
    ("plain", [0.25, 0.5, 0.25]),
    ("zero_first", [0.0, 0.5, 0.5]),
    ("zero_middle", [0.5, 0.0, 0.5]),
    ("zero_last", [0.5, 0.5, 0.0]),
    ("zeros_around", [0.0, 0.0, 1.0, 0.0, 0.0]),
    ("sums_to_3", [1.5, 0.75, 0.75]),
    ("card_1", [1.0]),
    ("tenths", [0.1] * 10),
]


def boundary_uniforms(p):
    """u at every boundary c_s / total, just below and just above it, 0 and 1 - 2^-53."""
    cdf = running_sums(np.asarray(p, dtype=np.float64).reshape(-1, 1))[:, 0]
    us = [0.0, 1.0 - 2.0 ** -53, 0.5]
    for c in cdf:
        b = c / cdf[-1]
        for u in (b, np.nextafter(b, 0.0), np.nextafter(b, 1.0), np.nextafter(np.nextafter(b, 0.0), 0.0)):
            if 0.0 <= u < 1.0:
                us.append(float(u))
    return np.array(us, dtype=np.float64)


def expected_state(p, u):
    """The rule, spelled out per value in plain Python floats."""
    c, acc = [], 0.0
    for x in p:
        acc = acc + float(x)
        c.append(acc)
    t = float(u) * c[-1]
    for s, cs in enumerate(c):
        if cs > t:
            return s
    return next(s for s, cs in enumerate(c) if cs == c[-1])
