"""Parameter learning: the numpy restatement of the device kernels and the case list of their tests.

A family is ``(columns, cardinalities)``: the code column and cardinality of the node, then of each
parent.  Its table is the CPD's ``[node_card, prod(parent_card)]`` in C order; the tables of a set of
families lie end to end in one flat buffer (``layout``).  The restatement:

  count_ref    np.add.at per family over codes[col, row0 + row]; a row holding 255 in any column of the
               family is skipped for that family only; a code that is neither 255 nor a state raises
               IndexError (``bad="skip"`` skips it instead, which is what the kernel leaves behind)
  finish_ref   counts (+ pseudo-counts), the MLE fill of all-zero columns with ones, values / values.sum(axis=0)

kernel_cases(tile, rows_per_block) lists the shapes the count kernel's tests run: every row count at
which the launch changes (one wave's rows +- 1, one workgroup's rows +- 1, three workgroups and a tail), a
row window inside a larger buffer, no parents and the maximum number of parents, tables one bin below,
at and one bin above the LDS tile, families grouped in one workgroup around a global one, one hot bin,
missing codes, cardinalities 1 and 254.
"""
import math

import numpy as np

MISSING = 255
MAX_DIMS = 32
LD = np.longdouble
HAVE_LD = np.finfo(LD).eps < 2.0 ** -60


def layout(families):
    """(offsets, sizes, strides) of the flat buffer: strides per family, node first, last parent fastest."""
    offsets, sizes, strides, off = [], [], [], 0
    for cols, cards in families:
        st, size = [0] * len(cards), 1
        for v in range(len(cards) - 1, -1, -1):
            st[v] = size
            size *= int(cards[v])
        offsets.append(off)
        sizes.append(size)
        strides.append(st)
        off += size
    return offsets, sizes, strides


def count_ref(codes, families, row0=0, n_rows=None, weights=None, bad="raise"):
    """Flat count tables: int64, or per-bin sums of `weights` in long double (math.fsum where long
    double is no wider than double) with the per-bin number of addends and sum of |w| beside them."""
    codes = np.asarray(codes)
    n_rows = codes.shape[1] - row0 if n_rows is None else n_rows
    offsets, sizes, strides = layout(families)
    total = offsets[-1] + sizes[-1]
    out = np.zeros(total, dtype=np.int64 if weights is None else LD)
    n_add = np.zeros(total, dtype=np.int64)
    mag = np.zeros(total, dtype=LD)
    for f, (cols, cards) in enumerate(families):
        win = codes[list(cols), row0:row0 + n_rows].astype(np.int64)
        card = np.asarray(cards, dtype=np.int64)[:, None]
        wrong = (win != MISSING) & (win >= card)
        if wrong.any() and bad == "raise":
            raise IndexError("a state code is >= its variable's cardinality")
        valid = ~((win == MISSING) | wrong).any(axis=0)
        idx = offsets[f] + (win[:, valid] * np.asarray(strides[f], dtype=np.int64)[:, None]).sum(axis=0)
        if weights is None:
            np.add.at(out, idx, 1)
            continue
        w = np.asarray(weights, dtype=np.float64)[row0:row0 + n_rows][valid]
        np.add.at(n_add, idx, 1)
        np.add.at(mag, idx, np.abs(w).astype(LD))
        if HAVE_LD:
            np.add.at(out, idx, w.astype(LD))
        else:
            for b in np.unique(idx):
                out[b] = math.fsum(w[idx == b])
    return out if weights is None else (out, n_add, mag)


def finish_ref(counts, families, pseudo=None, bayes=False):
    """Flat fp64 CPD values from flat counts (+ flat pseudo-counts)."""
    offsets, sizes, _ = layout(families)
    out = np.empty(offsets[-1] + sizes[-1], dtype=np.float64)
    for f, (cols, cards) in enumerate(families):
        sl = slice(offsets[f], offsets[f] + sizes[f])
        v = np.asarray(counts[sl], dtype=np.float64).reshape(int(cards[0]), -1)
        if pseudo is not None:
            v = v + np.asarray(pseudo[sl], dtype=np.float64).reshape(v.shape)
        else:
            v = v.copy()
        if not bayes:
            v[:, (v == 0).all(axis=0)] = 1.0
        with np.errstate(invalid="ignore", divide="ignore"):
            out[sl] = (v / v.sum(axis=0)).ravel()
    return out


def pseudo_ref(families, kind, value=None):
    """Flat pseudo-counts: "k2" (ones), "bdeu" (value / table size), "dirichlet" (a scalar)."""
    offsets, sizes, _ = layout(families)
    out = np.empty(offsets[-1] + sizes[-1], dtype=np.float64)
    for f in range(len(families)):
        sl = slice(offsets[f], offsets[f] + sizes[f])
        out[sl] = {"k2": 1.0, "bdeu": (float(value) / sizes[f]) if kind == "bdeu" else 0.0,
                   "dirichlet": float(value) if kind == "dirichlet" else 0.0}[kind]
    return out


# ---------------------------------------------------------------------------- kernel cases
def _random_codes(rng, n_cols, ld, cards_of_col, missing=0.0):
    codes = np.empty((n_cols, ld), dtype=np.uint8)
    for c in range(n_cols):
        codes[c] = rng.integers(0, cards_of_col[c], ld)
        if missing:
            codes[c, rng.random(ld) < missing] = MISSING
    return codes


def _col_cards(families, n_cols):
    cc = [2] * n_cols
    for cols, cards in families:
        for c, k in zip(cols, cards):
            cc[c] = k
    return cc


# five families over six columns sharing one LDS tile: no parents, one, two and three parents, a repeat
MIXED = [([0], [3]), ([1, 0], [2, 3]), ([2, 0, 1], [4, 3, 2]), ([3, 2, 1, 0], [5, 4, 2, 3]), ([4, 5], [2, 6])]


def kernel_cases(tile, rows_per_block):
    """[{name, families, codes [n_cols, ld] uint8, row0, n_rows}] (seeded; built once per call)."""
    rng = np.random.default_rng(2024)
    cases = []

    def add(name, families, n_rows, n_cols=None, missing=0.0, ld=None, row0=0, codes=None):
        n_cols = 1 + max(c for cols, _ in families for c in cols) if n_cols is None else n_cols
        ld = n_rows + row0 if ld is None else ld
        if codes is None:
            codes = _random_codes(rng, n_cols, ld, _col_cards(families, n_cols), missing)
        cases.append({"name": name, "families": families, "codes": codes, "row0": row0, "n_rows": n_rows})
        return codes

    for n in (1, 63, 64, 65, rows_per_block - 1, rows_per_block, rows_per_block + 1, 3 * rows_per_block + 77):
        add(f"rows_{n}", MIXED, n, missing=0.1)
    # the same row counts in a buffer whose leading dimension is a multiple of 4: the four-rows-per-lane
    # kernel and its one-row tail (ld = n_rows above takes the one-row kernel unless n_rows % 4 == 0)
    for n in (1, 3, 5, 63, 65, 255 * 4 + 2, rows_per_block - 1, rows_per_block + 1, 3 * rows_per_block + 77):
        add(f"rows_{n}_ld4", MIXED, n, ld=(n + 3) // 4 * 4 + 4, missing=0.1)
    # a window of a larger buffer: rows before and after it, and columns no family reads, hold valid
    # codes that must not be counted
    add("window", MIXED, rows_per_block + 5, n_cols=8, ld=rows_per_block + 300, row0=131, missing=0.05)
    add("window_ld4", MIXED, rows_per_block + 5, n_cols=8, ld=rows_per_block + 300, row0=132, missing=0.05)
    # the maximum number of parents (31): ten of cardinality 2, the rest of cardinality 1; in LDS, and
    # with twelve of cardinality 2 (12,288 bins) in global memory
    for name, twos in (("max_parents_lds", 10), ("max_parents_global", 12)):
        cards = [3] + [2] * twos + [1] * (MAX_DIMS - 1 - twos)
        add(name, [(list(range(MAX_DIMS)), cards), ([5], [2])], 1500, missing=0.01)
    assert tile == 4096, "the tile-edge families below are factorised for a 4,096-bin tile"
    for sfx, ld in (("", None), ("_ld4", 2 * rows_per_block + 12)):
        add("tile_minus_1" + sfx, [([0, 1, 2, 3, 4], [13, 3, 3, 5, 7])], 2 * rows_per_block + 9, ld=ld)  # 4,095 bins: LDS
        add("tile_exact" + sfx, [([0, 1, 2], [16, 16, 16])], 2 * rows_per_block + 9, ld=ld)             # 4,096 bins: LDS
        add("tile_plus_1" + sfx, [([0, 1], [17, 241])], 2 * rows_per_block + 9, ld=ld, missing=0.02)    # 4,097: global
    # groups around a global family: [two small][global][two small, the first filling its tile with the next]
    add("groups_around_global", [([0], [3]), ([1, 0], [2, 3]), ([2, 3, 4], [20, 20, 20]), ([5, 0], [100, 3]),
                                 ([6, 5], [30, 100]), ([7, 6], [40, 30])], rows_per_block + 123, missing=0.05)
    # every row in the same bin
    hot = np.full((6, 2 * rows_per_block + 1), 1, dtype=np.uint8)
    add("one_bin", MIXED, hot.shape[1], codes=hot)
    add("one_bin_ld4", MIXED, 2 * rows_per_block, codes=hot[:, :2 * rows_per_block].copy())
    hot_g = np.full((2, rows_per_block + 3), 7, dtype=np.uint8)
    add("one_bin_global", [([0, 1], [17, 241])], hot_g.shape[1], codes=hot_g)
    # missing codes: in the child only, in one parent only, everywhere
    fam = [([0, 1, 2], [3, 4, 5]), ([1], [4]), ([2, 1], [5, 4])]
    for name, rows_missing in (("missing_child", [0]), ("missing_parent", [2]), ("missing_all", [0, 1, 2])):
        c = _random_codes(rng, 3, 700, [3, 4, 5])
        for r in rows_missing:
            c[r, :] = MISSING
        add(name, fam, 700, codes=c)
    add("card_1_and_254", [([0, 1], [254, 1]), ([1, 0], [1, 254]), ([1], [1]), ([0], [254])], 3000, missing=0.1)
    return cases


# ---------------------------------------------------------------------------- golden cases (tests/golden)
def load_golden():
    import json
    import os

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "fit_cases.json")) as f:
        cases = json.load(f)
    return cases, np.load(os.path.join(here, "fit_alarm.npz"))


def golden_frame(case):
    """The case's input DataFrame (null -> NaN; all-number columns keep a numeric dtype)."""
    import pandas as pd

    cols = {}
    for name, vals in case["frame"].items():
        if all(v is None or isinstance(v, (int, float)) for v in vals):
            cols[name] = np.array([np.nan if v is None else v for v in vals],
                                  dtype=np.float64 if any(v is None or isinstance(v, float) for v in vals) else np.int64)
        else:
            cols[name] = np.array([np.nan if v is None else v for v in vals], dtype=object)
    return pd.DataFrame(cols)


def golden_runs(cases):
    """[(id, case, run key, estimator, kwargs of get_parameters, state_names or None, weighted)] for
    every estimator call recorded in fit_cases.json."""
    a, b, c, d = cases["a"], cases["b"], cases["c"], cases["d"]
    arrays = {v: np.asarray(x) for v, x in c["pseudo_arrays"].items()}
    bayes5 = {"prior_type": "BDeu", "equivalent_sample_size": 5}
    c_case = dict(b, **c)
    return [
        ("a-mle", a, "mle", "mle", {}, None, False),
        ("a-bdeu5", a, "bdeu5", "bayes", bayes5, None, False),
        ("b-mle", b, "mle", "mle", {}, b["state_names"], False),
        ("b-mle-collected", b, "mle_collected", "mle", {}, None, False),
        ("b-bdeu5", b, "bdeu5", "bayes", bayes5, b["state_names"], False),
        ("c-k2", c_case, "k2", "bayes", {"prior_type": "K2"}, b["state_names"], False),
        ("c-dirichlet-scalar", c_case, "dirichlet_scalar", "bayes", {"prior_type": "dirichlet", "pseudo_counts": 3},
         b["state_names"], False),
        ("c-dirichlet-arrays", c_case, "dirichlet_arrays", "bayes", {"prior_type": "dirichlet", "pseudo_counts": arrays},
         b["state_names"], False),
        ("c-bdeu-per-node", c_case, "bdeu_per_node", "bayes",
         {"prior_type": "BDeu", "equivalent_sample_size": {"X": 1, "Y": 2.5, "Z": 10, "W": 4}}, b["state_names"], False),
        ("d-mle-weighted", d, "mle_weighted", "mle", {}, None, True),
    ]


def parents_of(edges, node):
    return sorted(u for u, v in edges if v == node)


def collected_states(df, given=None):
    """The estimators' state names: the caller's, else sorted(unique non-NaN values) (base.py:44-65)."""
    out = {}
    for var in df.columns:
        if given and var in given:
            out[var] = list(given[var])
        else:
            out[var] = sorted(df[var].dropna().unique())
    return out


def restate_run(case, est, kwargs, state_names, weighted):
    """The restatement of one recorded estimator call: {node: (counts 2-D, cpd values 2-D)}, from
    host-encoded codes (pgmpy_amd.inference.batch.encode_states) through count_ref / finish_ref."""
    from pgmpy_amd.inference.batch import encode_states

    df = golden_frame(case)
    nodes, edges = case["nodes"], [tuple(e) for e in case["edges"]]
    states = collected_states(df, state_names)
    codes = encode_states({v: states[v] for v in nodes}, df, nodes)
    families = [([nodes.index(v) for v in [n] + parents_of(edges, n)],
                 [len(states[v]) for v in [n] + parents_of(edges, n)]) for n in nodes]
    w = df["_weight"].to_numpy(dtype=np.float64) if weighted else None
    counts = count_ref(codes, families, weights=w)
    if weighted:
        counts = counts[0].astype(np.float64)
    offsets, sizes, _ = layout(families)
    pseudo = None
    if est == "bayes":
        pseudo = np.empty(offsets[-1] + sizes[-1])
        for f, n in enumerate(nodes):
            kind = kwargs["prior_type"].lower()
            if kind == "k2":
                p = 1.0
            elif kind == "bdeu":
                ess = kwargs["equivalent_sample_size"]
                p = float(ess[n] if isinstance(ess, dict) else ess) / sizes[f]
            else:
                pc = kwargs["pseudo_counts"]
                p = np.asarray(pc[n], dtype=np.float64).ravel() if isinstance(pc, dict) else float(pc)
            pseudo[offsets[f]:offsets[f] + sizes[f]] = p
    values = finish_ref(counts, families, pseudo=pseudo, bayes=est == "bayes")
    return {n: (counts[offsets[f]:offsets[f] + sizes[f]].reshape(families[f][1][0], -1),
                values[offsets[f]:offsets[f] + sizes[f]].reshape(families[f][1][0], -1)) for f, n in enumerate(nodes)}


def alarm_families(model, nodes):
    """Families of the alarm model over codes whose rows are `nodes` (sorted), parents sorted."""
    col = {v: i for i, v in enumerate(nodes)}
    states = model.states
    fams = []
    for n in nodes:
        scope = [n] + sorted(model.get_parents(n))
        fams.append(([col[v] for v in scope], [len(states[v]) for v in scope]))
    return fams
