"""The likelihood-weighted posterior (pgm_sample_posterior) restated in numpy on top of
tests/sample_cases.sample_ref, independently of the C++ (pgmpy_amd/csrc/pgmlw.hip), and the cases the CPU
and GPU tests share.

`posterior_ref` replicates an evidence row S times, takes sample_ref's codes and long-double weights and
histograms them in long double, without any quantisation.  `acc_ref` is the integer version the kernel's
contract states (q = rint(ldexp(exp(lw - M), K)), lw summed in fp64 in plan order): it agrees with the
device up to the last bits of log / exp and is for checking the fixed-point scheme itself.

The tolerance of `post` against the unquantised restatement is derived, not tuned: quantisation is at
most half a unit per sample relative to the row's largest weight (S * 2^-K / 2 in the numerator and in the
denominator), and log / exp may differ by a couple of ulp per observed term:
    atol = S * 2^(1 - K) + 4e-13 * n_observed
and for log_evidence the same expression, relative.
"""
import numpy as np

from tests import sample_cases as SC

MISSING, FREE, GIVEN, OBSERVED = SC.MISSING, SC.FREE, SC.GIVEN, SC.OBSERVED
CHUNK = 1024  # PGM_LW_CHUNK (asserted against pgm_sample_posterior_info in the tests)
SAMPLE_COUNTS = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]


def k_of(S):
    """K = min(52, 62 - ceil(log2 S))."""
    return min(52, 62 - (int(S) - 1).bit_length())


def tolerance(S, n_observed):
    return S * 2.0 ** (1 - k_of(S)) + 4e-13 * n_observed


def target_layout(targets):
    """[(offset, size)] of the target tables laid end to end, and the total."""
    out, off = [], 0
    for cols, cards in targets:
        size = int(np.prod(cards))
        out.append((off, size))
        off += size
    return out, off


def target_bins(targets, codes):
    """[n_targets, n] flat bin of every sample: the first column slowest (the fit layout)."""
    layout, _ = target_layout(targets)
    bins = np.empty((len(targets), codes.shape[1]), dtype=np.int64)
    for t, ((cols, cards), (off, _)) in enumerate(zip(targets, layout)):
        b = np.zeros(codes.shape[1], dtype=np.int64)
        for c, k in zip(cols, cards):
            b = b * int(k) + codes[c].astype(np.int64)
        bins[t] = off + b
    return bins


def n_observed(families, modes, evidence_row):
    """OBSERVED families whose evidence code is not 255."""
    return sum(1 for (cols, _), m in zip(families, modes) if m == OBSERVED and evidence_row[cols[0]] != MISSING)


def posterior_ref(families, tables, modes, evidence, targets, S, seed=0, first_row=0):
    """Per evidence row (a column of `evidence` [n_cols, R]) a dict: post (long double [total_bins]),
    log_evidence, ess (long double), bad, and the samples' codes and weights."""
    evidence = np.asarray(evidence, dtype=np.uint8)
    layout, total = target_layout(targets)
    rows = []
    for r in range(evidence.shape[1]):
        given = np.repeat(evidence[:, r:r + 1], S, axis=1)
        codes, w, bad = SC.sample_ref(families, tables, S, seed=seed, first_row=first_row + r * S,
                                      n_cols=evidence.shape[0], given=given, modes=modes, weights=True)
        if bad:
            rows.append({"bad": True, "post": np.full(total, np.nan), "log_evidence": np.nan, "ess": 0.0,
                         "codes": codes, "w": w})
            continue
        hist = np.zeros(total, dtype=np.longdouble)
        bins = target_bins(targets, codes)
        for t in range(len(targets)):
            np.add.at(hist, bins[t], w)
        sw = w.sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            post = hist / sw
            le = np.log(sw / np.longdouble(S))
            ess = sw * sw / (w * w).sum() if sw > 0 else np.longdouble(0)
        rows.append({"bad": False, "post": post, "log_evidence": le, "ess": ess, "codes": codes, "w": w})
    return rows


def log_weights64(families, tables, modes, evidence_row, codes):
    """The samples' log-weights as the kernel states them: fp64, +0.0 start, per OBSERVED family whose code
    is a state one division, one log and one addition, in plan order."""
    lw = np.zeros(codes.shape[1], dtype=np.float64)
    for (cols, cards), table, mode in zip(families, tables, modes):
        g = int(evidence_row[cols[0]])
        if mode != OBSERVED or g == MISSING:
            continue
        table = np.asarray(table, dtype=np.float64).reshape(int(cards[0]), -1)
        cdf = SC.running_sums(table)
        col = np.zeros(codes.shape[1], dtype=np.int64)
        for c, k in zip(cols[1:], cards[1:]):
            col = col * int(k) + codes[c]
        with np.errstate(divide="ignore"):
            lw = lw + np.log(table[g, col] / cdf[-1, col])
    return lw


def acc_ref(families, tables, modes, evidence_row, targets, codes):
    """(acc uint64 [total_bins], M, sum q, sum q', sum q'^2) of one row from its samples' codes."""
    S = codes.shape[1]
    K = k_of(S)
    lw = log_weights64(families, tables, modes, evidence_row, codes)
    M = lw.max()
    _, total = target_layout(targets)
    acc = np.zeros(total, dtype=np.uint64)
    if M == -np.inf:
        return acc, M, 0, 0, 0
    q = np.rint(np.ldexp(np.exp(lw - M), K)).astype(np.uint64)
    bins = target_bins(targets, codes)
    for t in range(len(targets)):
        np.add.at(acc, bins[t], q)
    q1 = q >> np.uint64(max(K - 20, 0))
    return acc, M, int(q.sum()), int(q1.sum()), int((q1 * q1).sum())


# ---------------------------------------------------------------------------- the nets of the GPU cases
def plan_order_net():
    """Four nodes, cards 2 / 3 / 4 / 2, D with two parents.  Code columns: A 3, B 0, C 2, D 1, so the plan
    order (A, B, C, D: columns 3, 0, 2, 1) differs from the column order and both Philox words of the
    pairs (0, 1) and (2, 3) are used.  Returns (families, tables, n_cols)."""
    A, B, C, D = 3, 0, 2, 1
    fams = [([A], [2]), ([B, A], [3, 2]), ([C, B], [4, 3]), ([D, A, C], [2, 2, 4])]
    rng = np.random.default_rng(20260)
    tables = []
    for cols, cards in fams:
        t = rng.uniform(0.05, 1.0, size=(cards[0], int(np.prod(cards[1:]))))
        tables.append(t / t.sum(axis=0, keepdims=True))
    return fams, tables, 4


PLAN_ORDER_EVIDENCE = np.array([  # rows: B, D, C, A (columns 0..3); one evidence row per column below
    # nothing   everything   leaf D    root A    an inner node only (255 in the other OBSERVED columns)   mixed
    [MISSING, 2, MISSING, MISSING, 0, 1],   # B (column 0)
    [MISSING, 1, 0, MISSING, MISSING, 1],         # D (column 1)
    [MISSING, 3, MISSING, MISSING, MISSING, MISSING],  # C (column 2)
    [MISSING, 0, MISSING, 1, MISSING, 0],         # A (column 3)
], dtype=np.uint8)
PLAN_ORDER_MODES = [OBSERVED, OBSERVED, OBSERVED, OBSERVED]
PLAN_ORDER_TARGETS = [([0], [3]), ([1], [2]), ([2], [4]), ([3], [2]), ([2, 3, 1], [4, 2, 2])]


def chain_net(n=320, n_obs=300, p=1e-3):
    """A chain X0 -> X1 -> ... of binary nodes, column i = node i.  P(X_i = 1 | parent) is about p (it
    varies a little with i and the parent), and the first n_obs nodes are observed at 1: lw is about
    n_obs * log(p)."""
    fams, tables = [], []
    for i in range(n):
        if i == 0:
            fams.append(([0], [2]))
            tables.append(np.array([[1 - p], [p]]))
        else:
            fams.append(([i, i - 1], [2, 2]))
            a, b = p * (1 + 0.25 * np.sin(i)), p * (1.5 + 0.25 * np.cos(i))
            tables.append(np.array([[1 - a, 1 - b], [a, b]]))
    ev = np.full((n, 2), MISSING, dtype=np.uint8)
    ev[:n_obs, 0] = 1
    ev[:n_obs, 1] = 1
    ev[7, 1] = 0  # the two rows differ
    return fams, tables, ev


def zero_net():
    """A -> B with an exact 0: P(B = 1 | A = 0) = 0.  Evidence B = 1 with A = 0 given has weight 0 in
    every sample; B = 1 alone has weight 0 in the samples that draw A = 0."""
    fams = [([0], [2]), ([1, 0], [2, 2])]
    tables = [np.array([[0.5], [0.5]]), np.array([[1.0, 0.25], [0.0, 0.75]])]
    ev = np.array([[0, MISSING], [1, 1]], dtype=np.uint8)  # columns: row 0 (A = 0, B = 1), row 1 (B = 1)
    return fams, tables, ev


# ---------------------------------------------------------------------------- the public-API case on alarm
API_SEED = 17  # chosen on the CPU (tests/test_lw_cpu.py) so that no row's top two joint cells are near a tie
API_S = 4096
API_ROWS = 16
API_DROPPED = ["CVP", "HRBP"]  # two observed columns of the golden frame that the case drops


def ess_tolerance(S, sum_q1):
    """Relative tolerance of ess = (sum q')^2 / sum q'^2 when every q' may be off by one unit: the numerator
    moves by at most 2 S / sum q' and, with sum q'^2 >= (sum q')^2 / S, the denominator by at most
    (2 sum q' + S) S / (sum q')^2."""
    return 2.0 * S / sum_q1 + (2.0 * sum_q1 + S) * S / (sum_q1 * sum_q1)


def ess_ref(w):
    """(ess, sum q') of long-double weights with q' = floor(w / max w * 2^20), as the kernel's q >> (K - 20)."""
    q1 = np.floor(w / w.max() * np.longdouble(2.0 ** 20)).astype(np.float64)
    return float(q1.sum() ** 2 / (q1 * q1).sum()), float(q1.sum())


def alarm_api_case():
    """(model, golden, nodes, families, tables, kept columns, missing variables, evidence [n_nodes, API_ROWS])
    of the first API_ROWS rows of tests/golden/alarm_predict.json without the API_DROPPED columns."""
    import json
    import os

    from pgmpy_amd.utils import get_example_model

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alarm_predict.json")) as f:
        g = json.load(f)
    m = get_example_model("alarm")
    nodes, _, fams, tables = SC.model_plan(m)
    keep = [c for c in g["columns"] if c not in API_DROPPED]
    assert len(keep) == len(g["columns"]) - len(API_DROPPED)
    ev = np.full((len(nodes), API_ROWS), MISSING, dtype=np.uint8)
    for r, row in enumerate(g["rows"][:API_ROWS]):
        for v, s in zip(g["columns"], row):
            if v in keep and s is not None:
                ev[nodes.index(v), r] = list(m.states[v]).index(s)
    missing = [v for v in m.nodes() if v not in keep]
    return m, g, nodes, fams, tables, keep, missing, ev
