"""The dynamic-network filter restated in numpy, independently of the C++ (pgmpy_amd/csrc/pgmdbn.hip and
pgmdbn_plan.cpp), brute-force enumeration of the unrolled network, the tolerance of the comparisons and the
seeded cases the CPU and GPU tests share.

A SPEC is a two-slice network over n nodes in sorted name order: ``card``; ``fam0[v] = (cols, table)`` the
slice-0 family of node v, cols over 0 .. n - 1, the node first; ``fam1[v]`` its transition family over the
two-slice window, column c < n being node c of slice t and column n + c node c of slice t + 1; ``table`` has one
axis per column.  EVIDENCE of one sequence is a uint8 array [T + 1, n], 255 = not observed.  A CASE adds the
clamped names and a code matrix [(T + 1) n, B] in the layout the kernel reads.

``recursion(spec, clamped, ev, dtype)`` is the recursion of include/pgmhip.h ("dynamic Bayesian networks") with
whole-array numpy sums: the joint x of the free nodes, the message over the free interface, scaling by c_t,
beta backwards.  ``fault=`` applies one of the structural errors of ``FAULTS`` to it: tests/test_dbn_cpu.py shows
with them that the tolerance below sees such an error on every case (``fault_table``).  ``enumerate_unrolled`` multiplies every CPD of the unrolled network into one array and sums
it, for prod card^(T + 1) <= 2^20.  Both return marginals of EVERY node, [T + 1, sum card].

Tolerance (``tolerance``).  The device adds the same terms as the fp64 run of ``recursion`` in another but fixed
order.  d, the largest deviation of the fp64 run from the long-double one relative to the largest entry, measures
what a summation order costs on that case; the device is allowed 16 d, and never less than 64 * 2^-53.  d is a
property of numpy's arithmetic alone (``deviation``; ``GOLDEN_D`` caches it per case): no device result enters.

Cases.  ``kernel_cases()`` has the smallest shape for each branch of the kernel; ``path_cases()`` the smallest that
reach what those stop short of (dynamic LDS above 64 KiB from both sides, the benchmarked HMM, two sequences per
wave, 254 states, n = 255), each with the plan geometry it expects.  ``reference(case, b)`` is the long-double run
of a sequence, computed once and shared.
"""
import functools
import json
import os

import numpy as np

MISSING = 255
U = 2.0 ** -53
LD = np.longdouble


# ------------------------------------------------------------------------------------------------ specs
def make_spec(names, card, intra, inter, seed, deterministic=()):
    """Random CPDs for the structure: intra = [(parent, child)] within a slice (copied to both slices), inter =
    [(node of slice t, node of slice t + 1)].  A node in `deterministic` gets one-hot columns (zeros)."""
    assert list(names) == sorted(names)
    n, idx = len(names), {v: i for i, v in enumerate(names)}
    rng = np.random.default_rng(seed)

    def table(v, cols):
        shape = [card[c % n] for c in cols]
        t = rng.random(shape) + 0.05
        if names[v] in deterministic:
            hot = rng.integers(0, shape[0], size=shape[1:])
            t = (np.arange(shape[0]).reshape([-1] + [1] * (len(shape) - 1)) == hot[None]).astype(np.float64)
        return t / t.sum(axis=0, keepdims=True)

    fam0, fam1 = [], []
    for v in range(n):
        pa = [idx[p] for p, c in intra if idx[c] == v]
        prev = [idx[p] for p, c in inter if idx[c] == v]
        fam0.append(([v] + pa, table(v, [v] + pa)))
        cols1 = [n + v] + [n + p for p in pa] + prev
        fam1.append((cols1, table(v, cols1)))
    order = _topological(n, [(idx[p], idx[c]) for p, c in intra])
    return {"names": list(names), "card": [int(k) for k in card], "fam0": fam0, "fam1": fam1, "order": order,
            "intra": list(intra), "inter": list(inter)}


def _topological(n, edges):
    order, left = [], set(range(n))
    while left:
        ready = sorted(v for v in left if not any(c == v and p in left for p, c in edges))
        assert ready, "the intra-slice graph has a cycle"
        order += ready
        left -= set(ready)
    return order


def sample(spec, T, B, seed):
    """Forward samples [B, T + 1, n] (uint8) of the unrolled network."""
    rng = np.random.default_rng(seed)
    n = len(spec["card"])
    out = np.zeros((B, T + 1, n), dtype=np.uint8)
    for b in range(B):
        for t in range(T + 1):
            for v in spec["order"]:
                cols, tab = spec["fam1"][v] if t else spec["fam0"][v]
                at = tuple(int(out[b, t - 1, c] if (t and c < n) else out[b, t, c % n]) for c in cols[1:])
                p = tab[(slice(None),) + at]
                out[b, t, v] = rng.choice(len(p), p=p / p.sum())
    return out


def to_codes(ev):
    """[B, T + 1, n] evidence -> the kernel's [(T + 1) n, B]."""
    B, T1, n = ev.shape
    return np.ascontiguousarray(ev.reshape(B, T1 * n).T)


def to_model(spec):
    """The pgmpy_amd DynamicBayesianNetwork of a spec (both slices' CPDs given)."""
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.models import DynamicBayesianNetwork

    names, card, n = spec["names"], spec["card"], len(spec["card"])
    m = DynamicBayesianNetwork()
    m.add_nodes_from(names)
    m.add_edges_from([((p, 0), (c, 0)) for p, c in spec["intra"]] + [((p, 0), (c, 1)) for p, c in spec["inter"]])
    for h, fams in enumerate((spec["fam0"], spec["fam1"])):
        for v, (cols, tab) in enumerate(fams):
            var = [(names[c % n], (c // n) if h else 0) for c in cols]
            m.add_cpds(TabularCPD(var[0], card[v], tab.reshape(card[v], -1), evidence=var[1:] or None,
                                  evidence_card=[card[c % n] for c in cols[1:]] or None))
    m.check_model()
    return m


def offsets(spec):
    """Column offset of every node in the marginal axis, and its length."""
    off = np.concatenate([[0], np.cumsum(spec["card"])])
    return off[:-1], int(off[-1])


# ------------------------------------------------------------------------------------------------ the recursion
# the structural errors ``recursion(fault=...)`` can make, each one a slip a kernel or its plan could make
FAULTS = {
    "clamped_parent_slice": "a clamped slice-t parent is read from slice t instead of t - 1",
    "message_group": "the message is summed over the wrong interface group (a reversed)",
    "beta_index": "gamma takes beta at the wrong interface state (the next one)",
    "beta_no_local": "local is left out of the beta update",
    "mask_slice0": "the evidence mask is ignored at slice 0",
    "digit_order": "the table lookups take the free nodes' digits first-fastest instead of last-fastest",
    "drop_prev_family": "the first transition family with a free slice-t parent is left out of the product",
}


def recursion(spec, clamped, ev, dtype=LD, fault=None):
    """(filter [T + 1, Q], smooth [T + 1, Q], loglik, impossible) of one sequence; Q over every node.
    fault: None or a key of FAULTS."""
    assert fault is None or fault in FAULTS
    card, n = spec["card"], len(spec["card"])
    names = spec["names"]
    is_clamped = [names[v] in clamped for v in range(n)]
    free = [v for v in range(n) if not is_clamped[v]]
    iface = [v for v in free if any(c == v for cols, _ in spec["fam1"] for c in cols[1:])]
    fshape = [card[v] for v in free]
    J = int(np.prod(fshape)) if free else 1
    S = int(np.prod([card[v] for v in iface])) if iface else 1
    dig = dict(zip(free, np.unravel_index(np.arange(J), fshape))) if free else {}
    ishape = [card[v] for v in iface]
    idig = dict(zip(iface, np.unravel_index(np.arange(S), ishape))) if iface else {}
    ix = np.ravel_multi_index([dig[v] for v in iface], ishape) if iface else np.zeros(J, dtype=np.int64)
    # the digits a table lookup takes: the mask, the marginals and I(x) keep the right ones
    tdig = dig
    if fault == "digit_order" and free:
        tdig = dict(zip(free, np.unravel_index(np.arange(J), fshape, order="F")))
    T1 = ev.shape[0]
    ev = ev.astype(np.int64)
    for t in range(T1):
        for v in range(n):
            assert ev[t, v] < card[v] or (ev[t, v] == MISSING and not is_clamped[v]), "bad code in a restated case"

    def lookup(cols, tab, t, with_prev):
        """The family's factor as [S or 1, J]; with_prev: whether it has a free slice-t parent."""
        at = []
        for c in cols:
            v = c % n
            before = t > 0 and c < n
            if is_clamped[v]:
                at.append(ev[t - 1, v] if before and fault != "clamped_parent_slice" else ev[t, v])
            elif before:
                at.append(idig[v][:, None])
            else:
                at.append(tdig[v][None, :])
        return np.broadcast_to(tab.astype(dtype)[tuple(at)], (S if with_prev else 1, J))

    def mask(t):
        m = np.ones(J, dtype=bool)
        if fault == "mask_slice0" and t == 0:
            return m
        for v in free:
            if ev[t, v] != MISSING:
                m &= dig[v] == ev[t, v]
        return m

    def factors(t):
        """(local [J], trans [S, J]) of slice t, the evidence mask folded into local."""
        local, trans = np.ones((1, J), dtype=dtype), np.ones((S, J), dtype=dtype)
        drop = fault == "drop_prev_family"
        for cols, tab in (spec["fam1"] if t else spec["fam0"]):
            prev = t > 0 and any(c < n and not is_clamped[c] for c in cols[1:])
            if prev and drop:
                drop = False
            elif prev:
                trans = trans * lookup(cols, tab, t, True)
            else:
                local = local * lookup(cols, tab, t, False)
        return np.where(mask(t), local[0], dtype(0)), trans

    off, Q = offsets(spec)

    def marginals(g, t):
        out = np.zeros(Q, dtype=dtype)
        for v in range(n):
            for k in range(card[v]):
                out[off[v] + k] = dtype(ev[t, v] == k) if is_clamped[v] else g[dig[v] == k].sum()
        return out

    alpha, msgs, cs = [], [], []
    filt = np.full((T1, Q), np.nan, dtype=dtype)
    loglik, dead = dtype(0), False
    for t in range(T1):
        local, trans = factors(t)
        if t:
            a = np.array([alpha[-1][ix == i].sum() for i in range(S)], dtype=dtype)
            if fault == "message_group":
                a = a[::-1].copy()
            msgs.append(a)
            un = local * (a[:, None] * trans).sum(axis=0)
        else:
            un = local
        c = un.sum()
        if not c > 0:
            dead = True
            break
        cs.append(c)
        alpha.append(un / c)
        loglik = loglik + np.log(c)
        filt[t] = marginals(alpha[-1], t)
    smooth = np.full((T1, Q), np.nan, dtype=dtype)
    if dead:
        return filt, smooth, dtype(-np.inf), True
    beta = np.ones(S, dtype=dtype)
    for t in range(T1 - 1, -1, -1):
        g = alpha[t] * beta[(ix + 1) % S if fault == "beta_index" else ix]
        smooth[t] = marginals(g / g.sum(), t)
        if t:
            local, trans = factors(t)
            w = beta[ix] / cs[t] if fault == "beta_no_local" else local * beta[ix] / cs[t]
            beta = (trans * w[None, :]).sum(axis=1)
    return filt, smooth, loglik, False


# ------------------------------------------------------------------------------------------------ enumeration
def enumerate_unrolled(spec, ev, smooth_only=False):
    """(filter, smooth, loglik) by summing the joint of the unrolled network in long double."""
    card, n = spec["card"], len(spec["card"])
    T1 = ev.shape[0]
    assert float(np.prod(np.asarray(card, dtype=np.float64))) ** T1 <= 2 ** 20, "too large to enumerate"
    off, Q = offsets(spec)

    def joint(last):
        """The joint of slices 0 .. last with their evidence applied, axes (t, v)."""
        axes = (last + 1) * n
        j = np.ones([1] * axes, dtype=LD)
        for t in range(last + 1):
            for cols, tab in (spec["fam1"] if t else spec["fam0"]):
                where = [(t - 1) * n + c if (t and c < n) else t * n + c % n for c in cols]
                shape = [1] * axes
                for w, k in zip(where, tab.shape):
                    shape[w] = k
                j = j * np.transpose(tab.astype(LD), np.argsort(where)).reshape(shape)
        for t in range(last + 1):
            for v in range(n):
                if ev[t, v] != MISSING:
                    keep = np.zeros(card[v], dtype=LD)
                    keep[ev[t, v]] = 1
                    shape = [1] * axes
                    shape[t * n + v] = card[v]
                    j = j * keep.reshape(shape)
        return j

    def marg(j, t):
        out = np.zeros(Q, dtype=LD)
        for v in range(n):
            others = tuple(a for a in range(j.ndim) if a != t * n + v)
            out[off[v]:off[v] + card[v]] = j.sum(axis=others)
        return out / j.sum()

    full = joint(T1 - 1)
    smooth = np.stack([marg(full, t) for t in range(T1)])
    filt = None if smooth_only else np.stack([marg(joint(t), t) for t in range(T1)])
    return filt, smooth, np.log(full.sum())


# ------------------------------------------------------------------------------------------------ tolerance
def deviation(spec, clamped, ev):
    """d of one sequence: (marginals, loglik) deviation of the fp64 recursion from the long-double one, the
    marginals' relative to their largest entry (1 at most), the log-likelihood's relative to max(|loglik|, 1): it
    is a sum of log c_t, and a c_t next to 1 (no evidence in the slice) gives a term next to 0 whose error is u of
    c_t, not of the term."""
    return _deviation(recursion(spec, clamped, ev, np.float64), recursion(spec, clamped, ev, LD))


def _deviation(run64, run_ld):
    (f64, s64, l64, _), (fld, sld, lld, dead) = run64, run_ld
    if dead:
        return 0.0, 0.0
    dm = max(float(np.nanmax(np.abs(f64 - fld))), float(np.nanmax(np.abs(s64 - sld))))
    dl = float(abs(l64 - lld) / max(abs(lld), LD(1)))
    return dm, dl


def tolerance(d):
    return max(16.0 * d, 64.0 * U)


GOLDEN_D = {}  # case name -> (d of the marginals, d of the log-likelihood), the largest over its sequences
GOLDEN_REF = {}  # (case name, b) -> recursion(..., LD) of sequence b: computed once, shared, never written to


def reference(case, b):
    """The long-double run of sequence b of a case (a case's name stands for its evidence: a changed copy of a
    case takes another name before it comes here)."""
    key = (case["name"], int(b))
    if key not in GOLDEN_REF:
        GOLDEN_REF[key] = recursion(case["spec"], case["clamped"], case["ev"][b])
    return GOLDEN_REF[key]


def golden_d(case):
    if case["name"] not in GOLDEN_D:
        ds = [_deviation(recursion(case["spec"], case["clamped"], e, np.float64), reference(case, b))
              for b, e in enumerate(case["ev"])]
        GOLDEN_D[case["name"]] = (max(d[0] for d in ds), max(d[1] for d in ds))
    return GOLDEN_D[case["name"]]


def differs(run, ref, tol_m, tol_l):
    """Whether a run (filter, smooth, loglik, impossible) leaves the long-double one by more than the tolerance:
    another NaN pattern or outcome, a marginal more than tol_m off, the log-likelihood more than tol_l (relative
    to max(|loglik|, 1))."""
    (f, s, l, dead), (wf, ws, wl, wdead) = run, ref
    if dead != wdead:
        return True
    for got, want in ((f, wf), (s, ws)):
        if not np.array_equal(np.isnan(got), np.isnan(want)):
            return True
        ok = ~np.isnan(want)
        if ok.any() and float(np.abs(got[ok] - want[ok]).max()) > tol_m:
            return True
    return (not dead) and float(abs(l - wl) / max(abs(wl), LD(1))) > tol_l


# ------------------------------------------------------------------------------------------------ cases
def _case(name, spec, clamped, T, B, seed, hide=0.5, predict=0):
    """Sampled sequences; a free node's cell is hidden with probability `hide`; the last `predict` slices are
    hidden altogether (free nodes only: a clamped node is observed in every cell)."""
    full = sample(spec, T, B, seed)
    rng = np.random.default_rng(seed + 1)
    ev = full.copy()
    for v, nm in enumerate(spec["names"]):
        if nm in clamped:
            continue
        gone = rng.random((B, T + 1)) < hide
        if predict:
            gone[:, T + 1 - predict:] = True
        ev[:, :, v][gone] = MISSING
    return {"name": name, "spec": spec, "clamped": list(clamped), "T": T, "B": B, "ev": ev, "codes": to_codes(ev)}


DOC = dict(names=["X", "Y", "Z"], card=[2, 2, 2], intra=[("Z", "X"), ("X", "Y")], inter=[("Z", "Z")])
TWO_IFACE = dict(names=["W", "X", "Y", "Z"], card=[2, 2, 2, 2], intra=[("Z", "X"), ("W", "X"), ("X", "Y")],
                 inter=[("Z", "Z"), ("W", "W"), ("Z", "W")])
CROSS = dict(names=["X", "Y", "Z"], card=[2, 2, 2], intra=[("Z", "X"), ("X", "Y")], inter=[("Z", "Z"), ("Z", "X")])


def doc_spec():
    """The docstring network with the docstring's CPDs."""
    s = make_spec(seed=0, **DOC)
    n = 3
    s["fam0"] = [([0, 2], np.array([[0.6, 0.9], [0.4, 0.1]])), ([1, 0], np.array([[0.2, 0.3], [0.8, 0.7]])),
                 ([2], np.array([0.5, 0.5]))]
    s["fam1"] = [([n + 0, n + 2], s["fam0"][0][1]), ([n + 1, n + 0], s["fam0"][1][1]),
                 ([n + 2, 2], np.array([[0.4, 0.7], [0.6, 0.3]]))]
    return s


def _chains(k, card=2, obs=True):
    """k independent hidden chains H0 .. Hk-1 (each Hi_t -> Hi_t+1) and, with obs, one observed child O of all."""
    hidden = [f"H{i:02d}" for i in range(k)]
    names = hidden + (["O"] if obs else [])
    cards = ([card] * k if isinstance(card, int) else list(card)) + ([3] if obs else [])
    intra = [(h, "O") for h in hidden] if obs else []
    return dict(names=names, card=cards, intra=intra, inter=[(h, h) for h in hidden])


@functools.lru_cache(maxsize=None)
def kernel_cases():
    """name -> case: the smallest shapes at which each branch of the kernel can go wrong."""
    out = []
    doc = doc_spec()
    # J = 2 (Z free), T = 0, 1, 2 and batch sizes that are no multiple of the 32 sequences of a wave
    # (the seed of the one-sequence case is one that observes Z: with Z hidden no fault of FAULTS shows at T = 0)
    for T, B, seed in ((0, 1, 13), (1, 63, 11), (2, 130, 12)):
        out.append(_case(f"doc_J2_T{T}_B{B}", doc, ["X", "Y"], T, B, seed, hide=0.3))
    # J = 1: everything clamped, the log-likelihood alone
    out.append(_case("all_clamped_J1", doc, ["X", "Y", "Z"], 2, 63, 20))
    # every node free: J = 8 > S = 2, cells observed and missing at random, then two slices of prediction
    out.append(_case("doc_free_J8_S2", doc, [], 2, 63, 21))
    out.append(_case("doc_predict", doc, [], 4, 5, 22, hide=0.4, predict=2))
    # J = 15 = 3 x 5: no power of two, idle lanes in a packed sequence; S = 3 < J, then S = J
    s15 = make_spec(names=["A", "B", "O"], card=[3, 5, 2], intra=[("A", "B"), ("B", "O")], inter=[("A", "A")], seed=30)
    out.append(_case("J15_S3", s15, ["O"], 2, 130, 31, hide=0.6))
    s15b = make_spec(names=["A", "B", "O"], card=[3, 5, 2], intra=[("A", "O"), ("B", "O")],
                     inter=[("A", "A"), ("B", "B"), ("A", "B")], seed=32)
    out.append(_case("J15_S15", s15b, ["O"], 2, 63, 33, hide=0.6))
    # the packing boundary: J = 64 (one sequence per wave, one x' per lane) and J = 65 (lanes stride)
    out.append(_case("J64_S64", make_spec(seed=40, **_chains(6)), ["O"], 2, 5, 41, hide=0.7))
    out.append(_case("J65_S65", make_spec(seed=42, **_chains(2, card=[5, 13])), ["O"], 2, 5, 43, hide=0.7))
    # nine families with a free slice-t parent: past the eight whose offsets the kernel keeps in registers
    out.append(_case("J512_S512_9fam", make_spec(seed=44, **_chains(9)), ["O"], 2, 2, 45, hide=0.8))
    # J = 4096: twelve binary free nodes, two of them the interface
    big = _chains(12, obs=False)
    big["inter"] = big["inter"][:2]
    big["intra"] = [(f"H{i:02d}", f"H{i + 1:02d}") for i in range(1, 11)]
    out.append(_case("J4096_S4", make_spec(seed=50, **big), [], 2, 2, 51, hide=0.8))
    # an interface node clamped beside a free one, cardinalities 2 and 3
    mix = make_spec(names=["A", "B", "O"], card=[2, 3, 2], intra=[("A", "O"), ("B", "O")],
                    inter=[("A", "A"), ("B", "B"), ("A", "B")], seed=60)
    out.append(_case("iface_clamped_2_3", mix, ["A", "O"], 2, 63, 61, hide=0.5))
    # an inter-slice edge into a node that is no interface node
    out.append(_case("cross_edge", make_spec(seed=70, **CROSS), ["Y"], 2, 63, 71, hide=0.5))
    out.append(_case("two_iface", make_spec(seed=72, **TWO_IFACE), [], 2, 63, 73, hide=0.5))
    # a deterministic CPD: zeros in the tables
    out.append(_case("deterministic", make_spec(seed=80, deterministic=("X",), **DOC), ["Y"], 2, 63, 81, hide=0.5))
    return {c["name"]: c for c in out}


def _n255_spec():
    """255 binary nodes: every node its own chain, every third an intra-slice parent of the next, every fifth an
    inter-slice parent of the node two on."""
    names = [f"N{i:03d}" for i in range(255)]
    intra = [(names[i], names[i + 1]) for i in range(0, 254, 3)]
    inter = [(nm, nm) for nm in names] + [(names[i], names[i + 2]) for i in range(1, 253, 5)]
    return make_spec(names=names, card=[2] * 255, intra=intra, inter=inter, seed=130)


@functools.lru_cache(maxsize=None)
def path_cases():
    """name -> case: the smallest shapes that reach the paths kernel_cases() stops short of.  ``expect`` is what
    makes a case the case it claims to be: the plan's J, S, sequences per wave, LDS bytes, families with / without a
    free slice-t parent.  The tests assert it from plan.info, so a shape that misses its path fails."""
    out = []

    def add(case, **expect):
        out.append(dict(case, expect=expect))

    # the benchmarked shape (tools/dbn_bench.py): 8 sequences per wave, 70 = 8 full waves and 6 of the ninth's 8
    hmm = hmm_spec()
    add(_case("hmm_J8_S8_n9", hmm, hmm["names"][1:], 3, 70, 110, hide=0.5),
        J=8, S=8, spw=8, lds=8 * (8 * 24 + 6 * 9), n_prev=1, n_cur=8)
    # P = 32 > J = 30: two sequences per wave, two idle lanes each; S = 6, R = 5; cardinalities 2, 3, 5
    mixed = make_spec(names=["A", "B", "C", "O"], card=[2, 3, 5, 2], intra=[("A", "C"), ("C", "O")],
                      inter=[("A", "A"), ("B", "B"), ("B", "C")], seed=112)
    add(_case("mixed_J30_S6", mixed, ["O"], 2, 5, 113, hide=0.5),
        J=30, S=6, spw=2, lds=2 * (8 * (30 + 12) + 6 * 4), n_prev=3, n_cur=1)
    # 254 states, the most a uint8 code holds beside MISSING; state 253 observed
    wide = make_spec(names=["H", "O"], card=[254, 2], intra=[("H", "O")], inter=[("H", "H")], seed=120)
    c254 = _case("card254", wide, ["O"], 2, 3, 121, hide=0.5)
    c254["ev"][0, 1, 0] = 253
    c254["codes"] = to_codes(c254["ev"])
    add(c254, J=254, S=254, spw=1, lds=8 * 3 * 254 + 6 * 2, n_prev=1, n_cur=1)
    # n at its limit, J = 1: 64 sequences per wave at 24 + 6 n bytes each, past 64 KiB of dynamic LDS
    n255 = _n255_spec()
    add(_case("n255_all_clamped", n255, n255["names"], 2, 70, 131),
        J=1, S=1, spw=64, lds=64 * (24 + 6 * 255), n_prev=0, n_cur=255)
    # past 64 KiB with one sequence per wave: J = S = 16 * 16 * 12, every free node in the interface
    big = make_spec(names=["A", "B", "C", "O"], card=[16, 16, 12, 2], intra=[("A", "O"), ("B", "O"), ("C", "O")],
                    inter=[("A", "A"), ("B", "B"), ("C", "C"), ("A", "B")], seed=140)
    add(_case("J3072_S3072", big, ["O"], 1, 2, 141, hide=0.5),
        J=3072, S=3072, spw=1, lds=8 * 3 * 3072 + 6 * 4, n_prev=3, n_cur=1)
    return {c["name"]: c for c in out}


def all_cases():
    """kernel_cases() and path_cases() in one table."""
    return {**kernel_cases(), **path_cases()}


def has_clamped_prev_parent(case):
    """Whether some transition family has a clamped slice-t parent."""
    spec, n = case["spec"], len(case["spec"]["card"])
    return any(c < n and spec["names"][c] in case["clamped"] for cols, _ in spec["fam1"] for c in cols[1:])


def has_free_interface(case):
    spec, n = case["spec"], len(case["spec"]["card"])
    return any(c < n and spec["names"][c] not in case["clamped"] for cols, _ in spec["fam1"] for c in cols[1:])


# the faults run on J3072_S3072 (one sequence), where a run of the restatement takes a second
CHEAP_FAULTS = ("message_group", "beta_index", "digit_order")
FAULT_TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dbn_fault_table.json")


def faults_of(case):
    """The faults that can be applied to a case."""
    names = [f for f in FAULTS if f != "clamped_parent_slice" or has_clamped_prev_parent(case)]
    return [f for f in names if f in CHEAP_FAULTS] if case["name"] == "J3072_S3072" else names


def fault_row(case):
    """{fault: whether tolerance(golden_d(case)) tells the faulted fp64 run from the long-double one on one of the
    first 16 sequences of the case (J3072_S3072: the first)}."""
    dm, dl = golden_d(case)
    tol_m, tol_l = tolerance(dm), tolerance(dl)
    rows = range(1 if case["name"] == "J3072_S3072" else min(case["B"], 16))
    with np.errstate(all="ignore"):
        return {f: any(differs(recursion(case["spec"], case["clamped"], case["ev"][b], np.float64, fault=f),
                               reference(case, b), tol_m, tol_l) for b in rows) for f in faults_of(case)}


def fault_table():
    """{case: fault_row(case)} over all_cases(): what profiles/dbn_fault_table.json records (a fault that cannot
    be applied to a case is absent from its row).  ``python -m tests.dbn_cases`` writes the file."""
    return {name: fault_row(case) for name, case in all_cases().items()}


def small_cases():
    """The cases small enough to enumerate, a few sequences of each."""
    keep = ("doc_J2_T2_B130", "doc_free_J8_S2", "doc_predict", "iface_clamped_2_3", "cross_edge", "two_iface",
            "deterministic", "all_clamped_J1")
    return [kernel_cases()[k] for k in keep]


# the two sequences on which the reference's backward pass is wrong (an interface node observed at t >= 1, an
# earlier slice queried): (spec, evidence {(name, t): state}, query).  The reference's values were recorded from
# pgmpy's DBNInference.query; the enumerated ones are recomputed by the tests.
def interface_evidence_cases():
    two = make_spec(seed=72, **TWO_IFACE)
    return [
        {"name": "doc", "spec": doc_spec(), "evidence": {("Z", 1): 1, ("Y", 2): 0}, "query": ("Z", 0)},
        {"name": "two_iface", "spec": two, "evidence": {("Z", 1): 1, ("W", 2): 0, ("Y", 2): 0}, "query": ("Z", 0)},
    ]


def evidence_array(spec, evidence, T):
    ev = np.full((T + 1, len(spec["card"])), MISSING, dtype=np.uint8)
    for (name, t), s in evidence.items():
        ev[t, spec["names"].index(name)] = s
    return ev


def hmm_spec(states=8, n_obs=8, seed=100):
    """The benchmark's HMM shape: one hidden node H of `states` states and n_obs binary observed children."""
    obs = [f"O{i}" for i in range(n_obs)]
    return make_spec(names=["H"] + obs, card=[states] + [2] * n_obs, intra=[("H", o) for o in obs],
                     inter=[("H", "H")], seed=seed)


# ------------------------------------------------------------------------------------------------ goldens
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_networks():
    """The networks tests/golden/make_golden_dbn.py runs the reference on."""
    return {"doc": doc_spec(), "two_iface": make_spec(seed=72, **TWO_IFACE)}


@functools.lru_cache(maxsize=None)
def load_golden():
    with open(os.path.join(GOLDEN, "dbn_cases.json")) as f:
        return json.load(f)


def load_golden_arrays():
    return np.load(os.path.join(GOLDEN, "dbn_cases.npz"))


def golden_spec(golden, name):
    """A recorded network as a spec: the tables are the recorded ones, not a builder's."""
    g = golden["networks"][name]
    n = len(g["card"])
    spec = {"names": g["names"], "card": g["card"], "intra": [tuple(e) for e in g["intra"]],
            "inter": [tuple(e) for e in g["inter"]],
            "fam0": [(f["cols"], np.asarray(f["table"], dtype=np.float64)) for f in g["fam0"]],
            "fam1": [(f["cols"], np.asarray(f["table"], dtype=np.float64)) for f in g["fam1"]]}
    spec["order"] = _topological(n, [(g["names"].index(p), g["names"].index(c)) for p, c in g["intra"]])
    return spec


def fault_table_record():
    """The content of profiles/dbn_fault_table.json."""
    return {"what": "whether dbn_cases.tolerance(golden_d(case)) tells recursion(fp64, fault=...) from the long-double "
                    "run on one of the first 16 sequences of a case; a fault that cannot be applied to a case is absent",
            "faults": FAULTS, "table": fault_table()}


if __name__ == "__main__":
    with open(FAULT_TABLE, "w") as out:
        json.dump(fault_table_record(), out, indent=1)
        out.write("\n")
    print(f"wrote {FAULT_TABLE}")
