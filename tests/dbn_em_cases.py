"""Shared by test_dbn_em_cpu.py and test_dbn_em_gpu.py: the E-step of the dynamic-network EM (pgm_dbn_estep,
include/pgmhip.h "dynamic Bayesian networks: expected counts") restated in numpy from its contract, independently
of the C++; brute-force enumeration of the unrolled network; k iterations of EM; the bounds of the comparisons.

Specs, evidence and cases are those of tests/dbn_cases.py.  A table set is FLAT: the families of the set in node
order, each family's table in C order over its columns (the node first), end to end: the layout of the CPD
values that DBNInference hands the kernel.  ``flat_values(spec)`` gives the two value buffers in that layout.

``estep_ref`` runs the scaled forward-backward recursion per sequence with whole-array sums and adds
gamma_0 / gs to the slice-0 families, gamma_t / gs to the transition families without a free slice-t parent and
xi_t / gs to those with one.  Beside the tables it counts, per entry, the non-zero terms that reached it: the N
of the bound.  ``estep_enumerate`` multiplies the unrolled network out and sums each family's posterior directly.

Bound (``table_bound``), after em_cases.bound and dbn_cases.tolerance.  An entry whose reference value is E, a sum
of N non-negative terms, may deviate by (N + 8) 2^-52 E + 16 d E_max: the first term is what any order of
summation of N non-negative terms costs (twice over, for rounding the long-double reference to fp64), the second
what the recursion that produced the terms costs: d is the deviation of the fp64 numpy run from the long-double
one relative to the largest entry, never less than 64 * 2^-53.  d is a property of numpy alone: no device number
enters.
"""
import numpy as np

from tests import dbn_cases as C

MISSING = C.MISSING
U = C.U
LD = np.longdouble
RTOL = 1e-5  # the relative part of the convergence test


# ------------------------------------------------------------------------------------------------ layout
def layout(spec):
    """(offsets0, offsets1, total0, total1): where each node's family starts in its flat set."""
    out = []
    for fams in (spec["fam0"], spec["fam1"]):
        sizes = [int(tab.size) for _, tab in fams]
        out.append(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    return out[0][:-1], out[1][:-1], int(out[0][-1]), int(out[1][-1])


def flat_values(spec, dtype=np.float64):
    return tuple(np.concatenate([np.asarray(tab, dtype=dtype).reshape(-1) for _, tab in fams])
                 for fams in (spec["fam0"], spec["fam1"]))


def with_values(spec, flat0, flat1):
    """A copy of the spec with the tables taken from two flat buffers."""
    out = dict(spec)
    for key, flat in (("fam0", flat0), ("fam1", flat1)):
        fams, at = [], 0
        for cols, tab in spec[key]:
            fams.append((cols, np.asarray(flat[at:at + tab.size]).reshape(tab.shape)))
            at += tab.size
        out[key] = fams
    return out


class _Geometry:
    """The joint x of the free nodes (the last fastest), the interface state i, and per family the flat entry
    its factor is read from at (i, x)."""

    def __init__(self, spec, clamped):
        self.spec = spec
        card, n = spec["card"], len(spec["card"])
        self.n = n
        self.is_clamped = [spec["names"][v] in clamped for v in range(n)]
        self.free = [v for v in range(n) if not self.is_clamped[v]]
        self.iface = [v for v in self.free if any(c == v for cols, _ in spec["fam1"] for c in cols[1:])]
        fshape, ishape = [card[v] for v in self.free], [card[v] for v in self.iface]
        self.J = int(np.prod(fshape)) if self.free else 1
        self.S = int(np.prod(ishape)) if self.iface else 1
        self.dig = dict(zip(self.free, np.unravel_index(np.arange(self.J), fshape))) if self.free else {}
        self.idig = dict(zip(self.iface, np.unravel_index(np.arange(self.S), ishape))) if self.iface else {}
        self.ix = (np.ravel_multi_index([self.dig[v] for v in self.iface], ishape) if self.iface
                   else np.zeros(self.J, dtype=np.int64))
        self.off = layout(spec)

    def entries(self, ev, t):
        """Per family of slice t (node order): (flat entries [S, J] or [1, J], whether it has a free slice-t parent)."""
        k, n = (1 if t else 0), self.n
        out = []
        for v, (cols, tab) in enumerate(self.spec["fam1"] if t else self.spec["fam0"]):
            strides = [int(np.prod(tab.shape[j + 1:], dtype=np.int64)) for j in range(tab.ndim)]
            idx = np.full((1, 1), self.off[k][v], dtype=np.int64)
            prev = False
            for c, st in zip(cols, strides):
                node, before = c % n, bool(t) and c < n
                if self.is_clamped[node]:
                    idx = idx + int(ev[t - 1 if before else t, node]) * st
                elif before:
                    idx, prev = idx + self.idig[node][:, None] * st, True
                else:
                    idx = idx + self.dig[node][None, :] * st
            out.append((np.broadcast_to(idx, (self.S if prev else 1, self.J)), prev))
        return out

    def mask(self, ev, t):
        m = np.ones(self.J, dtype=bool)
        for v in self.free:
            if ev[t, v] != MISSING:
                m &= self.dig[v] == ev[t, v]
        return m


def estep_ref(spec, clamped, ev_batch, dtype=LD):
    """What pgm_dbn_estep adds to zeroed tables for the sequences ev_batch [B, T + 1, n], in `dtype`:
    (tables0, tables1, loglik [B], impossible [B] bool, terms0, terms1): terms: per entry, the number of non-zero
    terms added to it."""
    g = _Geometry(spec, clamped)
    _, _, total0, total1 = g.off
    values = [v.astype(dtype) for v in flat_values(spec)]
    tables = [np.zeros(total0, dtype=dtype), np.zeros(total1, dtype=dtype)]
    terms = [np.zeros(total0, dtype=np.int64), np.zeros(total1, dtype=np.int64)]
    B, T1 = ev_batch.shape[0], ev_batch.shape[1]
    loglik, impossible = np.zeros(B, dtype=dtype), np.zeros(B, dtype=bool)

    def add(k, idx, w):
        np.add.at(tables[k], idx.reshape(-1), w.reshape(-1))
        np.add.at(terms[k], idx.reshape(-1), (w.reshape(-1) != 0).astype(np.int64))

    for b in range(B):
        ev = ev_batch[b].astype(np.int64)
        for t in range(T1):
            for v in range(g.n):
                assert ev[t, v] < spec["card"][v] or (ev[t, v] == MISSING and not g.is_clamped[v]), "bad code"
        ent, local, trans, alpha, msgs, cs = [], [], [], [], [None], []
        ll, dead = dtype(0), False
        for t in range(T1):
            e = g.entries(ev, t)
            loc, tr = np.ones(g.J, dtype=dtype), np.ones((g.S, g.J), dtype=dtype)
            for idx, prev in e:
                if prev:
                    tr = tr * values[1][idx]
                else:
                    loc = loc * values[1 if t else 0][idx[0]]
            loc = np.where(g.mask(ev, t), loc, dtype(0))
            if t:
                a = np.array([alpha[-1][g.ix == i].sum() for i in range(g.S)], dtype=dtype)
                msgs.append(a)
                un = loc * (a[:, None] * tr).sum(axis=0)
            else:
                un = loc
            c = un.sum()
            if not c > 0:
                dead = True
                break
            ent.append(e), local.append(loc), trans.append(tr), cs.append(c), alpha.append(un / c)
            ll = ll + np.log(c)
        impossible[b] = dead
        loglik[b] = dtype(-np.inf) if dead else ll
        if dead:
            continue
        beta = np.ones(g.S, dtype=dtype)
        for t in range(T1 - 1, -1, -1):
            gamma = alpha[t] * beta[g.ix]
            gs = gamma.sum()
            xi = None
            if t:
                xi = local[t][None, :] * (msgs[t][:, None] * trans[t]) / cs[t] * beta[g.ix][None, :]
            for idx, prev in ent[t]:
                if prev:
                    add(1, idx, xi / gs)
                else:
                    add(1 if t else 0, idx[0], gamma / gs)
            if t:
                beta = (trans[t] * (local[t] * beta[g.ix] / cs[t])[None, :]).sum(axis=1)
    return tables[0], tables[1], loglik, impossible, terms[0], terms[1]


# ------------------------------------------------------------------------------------------------ enumeration
def estep_enumerate(spec, ev):
    """(tables0, tables1, loglik) of ONE sequence ev [T + 1, n] by multiplying the unrolled network out in long
    double (prod card^(T + 1) <= 2^20) and summing every family's posterior directly."""
    card, n = spec["card"], len(spec["card"])
    T1 = ev.shape[0]
    assert float(np.prod(np.asarray(card, dtype=np.float64))) ** T1 <= 2 ** 20, "too large to enumerate"
    axes = T1 * n

    def where_of(cols, t):
        return [(t - 1) * n + c if (t and c < n) else t * n + c % n for c in cols]

    joint = np.ones([1] * axes, dtype=LD)
    for t in range(T1):
        for cols, tab in (spec["fam1"] if t else spec["fam0"]):
            where = where_of(cols, t)
            shape = [1] * axes
            for w, k in zip(where, tab.shape):
                shape[w] = k
            joint = joint * np.transpose(tab.astype(LD), np.argsort(where)).reshape(shape)
    for t in range(T1):
        for v in range(n):
            if ev[t, v] != MISSING:
                keep = np.zeros(card[v], dtype=LD)
                keep[ev[t, v]] = 1
                shape = [1] * axes
                shape[t * n + v] = card[v]
                joint = joint * keep.reshape(shape)
    total = joint.sum()
    off0, off1, total0, total1 = layout(spec)
    tables = [np.zeros(total0, dtype=LD), np.zeros(total1, dtype=LD)]
    for t in range(T1):
        for v, (cols, tab) in enumerate(spec["fam1"] if t else spec["fam0"]):
            where = where_of(cols, t)
            post = joint.sum(axis=tuple(a for a in range(axes) if a not in where)) / total  # axes ascending
            post = np.transpose(post, np.argsort(np.argsort(where)))  # back to the family's column order
            at = (off1 if t else off0)[v]
            tables[1 if t else 0][at:at + tab.size] += post.reshape(-1)
    return tables[0], tables[1], np.log(total)


# ------------------------------------------------------------------------------------------------ EM
def normalise(spec, flat0, flat1):
    """The M-step: every family's table divided by its column sums (axis 0 is the node); a column that is all zero
    becomes uniform, as pgm_fit_finish's MLE mode makes it."""
    out = []
    for fams, flat in ((spec["fam0"], flat0), (spec["fam1"], flat1)):
        new, at = np.empty_like(flat), 0
        for _, tab in fams:
            t = flat[at:at + tab.size].reshape(tab.shape[0], -1)
            t = np.where((t == 0).all(axis=0, keepdims=True), np.ones_like(t), t)
            new[at:at + tab.size] = (t / t.sum(axis=0)).reshape(-1)
            at += tab.size
        out.append(new)
    return out


def em_ref(spec, clamped, ev_batch, k, dtype=LD):
    """k iterations of E-step plus column normalisation from the spec's tables: (values0, values1 after them,
    [the log-likelihood of the possible sequences under the values each iteration started from])."""
    flat = [v.astype(dtype) for v in flat_values(spec)]
    lls = []
    for _ in range(k):
        t0, t1, loglik, dead, _, _ = estep_ref(with_values(spec, *flat), clamped, ev_batch, dtype=dtype)
        lls.append(loglik[~dead].sum())
        flat = normalise(spec, t0, t1)
    return flat[0], flat[1], lls


# ------------------------------------------------------------------------------------------------ bounds
def deviation(run64, run_ld):
    """d: the largest deviation of the fp64 tables from the long-double ones, relative to the largest entry."""
    big = max(float(np.abs(run_ld[0]).max(initial=0)), float(np.abs(run_ld[1]).max(initial=0)))
    if big == 0:
        return 0.0
    return max(float(np.abs(run64[k].astype(LD) - run_ld[k]).max(initial=0)) for k in (0, 1)) / big


def table_bound(ref, terms, d, e_max):
    """Per entry: (N + 8) 2^-52 E + 16 max(d, 64 u) E_max."""
    return (terms + 8) * 2.0 ** -52 * np.abs(ref.astype(np.float64)) + 16.0 * max(d, 64.0 * U) * e_max


_REF = {}  # case name -> the long-double run and d, computed once, shared, never written to


def reference(case):
    """{'ld': estep_ref(long double), 'd': deviation of the fp64 run, 'e_max'} of a case (a case's name stands for
    its evidence and its spec)."""
    if case["name"] not in _REF:
        with np.errstate(all="ignore"):
            ld = estep_ref(case["spec"], case["clamped"], case["ev"], LD)
            f64 = estep_ref(case["spec"], case["clamped"], case["ev"], np.float64)
        e_max = max(float(ld[0].max(initial=0)), float(ld[1].max(initial=0)))
        _REF[case["name"]] = {"ld": ld, "d": deviation(f64, ld), "e_max": e_max}
    return _REF[case["name"]]


def reference_by_unique_rows(case):
    """reference() for a batch of many sequences of few kinds: the restatement runs once per distinct sequence and
    the tables are the runs' tables times their multiplicities, summed in long double (terms and d likewise)."""
    if case["name"] not in _REF:
        rows, counts = np.unique(case["ev"].reshape(case["B"], -1), axis=0, return_counts=True)
        sums = {dt: None for dt in (LD, np.float64)}
        for dt in sums:
            for row, k in zip(rows, counts):
                r = estep_ref(case["spec"], case["clamped"], row.reshape((1,) + case["ev"].shape[1:]), dt)
                assert not r[3].any()
                part = [r[0].astype(LD) * int(k), r[1].astype(LD) * int(k), None, None, r[4] * int(k), r[5] * int(k)]
                sums[dt] = part if sums[dt] is None else [a if a is None else a + b for a, b in zip(sums[dt], part)]
        ld = tuple(sums[LD])
        e_max = max(float(ld[0].max(initial=0)), float(ld[1].max(initial=0)))
        _REF[case["name"]] = {"ld": ld, "d": deviation(sums[np.float64], ld), "e_max": e_max}
    return _REF[case["name"]]


def loglik_slack(spec, clamped, n_sequences, n_slices, ll):
    """What rounding may take from a batch log-likelihood: it is a sum over sequences and slices of log c_t, c_t a
    sum of J S products of n + 1 factors (relative error (J S + n + 2) u, which the logarithm makes absolute), added
    up in n_sequences n_slices steps."""
    g = _Geometry(spec, clamped)
    steps = n_sequences * n_slices
    return steps * (g.J * g.S + g.n + 3) * U + steps * U * abs(float(ll))


def check_tables(case, got0, got1, label=""):
    """Assert device tables within table_bound of the case's long-double reference; prints the worst ratio."""
    ref = reference(case)
    t0, t1, _, _, n0, n1 = ref["ld"]
    worst = 0.0
    for got, want, terms in ((got0, t0, n0), (got1, t1, n1)):
        allowed = table_bound(want, terms, ref["d"], ref["e_max"])
        err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - want).astype(np.float64)
        if err.size:
            worst = max(worst, float((err / np.maximum(allowed, 1e-300)).max()))
    print(f"{case['name']}{label}: worst error / allowed {worst:.3g} (d {ref['d']:.3g}, E_max {ref['e_max']:.3g})")
    assert worst <= 1.0, (case["name"], label, worst)


# ------------------------------------------------------------------------------------------------ cases
def plan_of(spec, clamped):
    """The DbnPlan of a spec with the families in node order (the layout of flat_values); made from the spec alone,
    so that a node of 255 states, which the plan takes and DBNInference's uint8 frames do not, can be clamped."""
    from pgmpy_amd.inference._dbn import DbnPlan

    n = len(spec["card"])
    fams = [[(list(cols), [spec["card"][c % n] for c in cols]) for cols, _ in spec[key]] for key in ("fam0", "fam1")]
    return DbnPlan(spec["card"], [name in clamped for name in spec["names"]], [False] * n, fams[0], fams[1])


def large_table_case():
    """The smallest transition table that cannot tile: hidden X of 9 states, X' | X, C with C clamped at 255
    states: 9 * 9 * 255 = 20,655 entries, 165,240 bytes > 160 KiB.  B = 70, T = 3."""
    spec = C.make_spec(names=["C", "X"], card=[255, 9], intra=[("C", "X")], inter=[("X", "X")], seed=150)
    rng = np.random.default_rng(151)
    B, T = 70, 3
    ev = np.full((B, T + 1, 2), MISSING, dtype=np.uint8)
    ev[:, :, 0] = rng.integers(0, 255, size=(B, T + 1))
    seen = rng.random((B, T + 1)) < 0.3
    ev[:, :, 1][seen] = rng.integers(0, 9, size=int(seen.sum()))
    return {"name": "large_table_C255_X9", "spec": spec, "clamped": ["C"], "T": T, "B": B, "ev": ev, "codes": C.to_codes(ev)}


def with_impossible(case, rows):
    """A copy of the `deterministic` case in which the sequences `rows` contradict X's one-hot slice-0 CPD: Z is
    observed at slice 0 and X at a state that has probability 0 given it."""
    spec = case["spec"]
    x, z = spec["names"].index("X"), spec["names"].index("Z")
    cols, tab = spec["fam0"][x]
    assert cols == [x, z]
    ev = case["ev"].copy()
    for b in rows:
        zb = 0 if ev[b, 0, z] == MISSING else int(ev[b, 0, z])
        ev[b, 0, z] = zb
        ev[b, 0, x] = int(np.argmin(tab[:, zb]))
        assert tab[ev[b, 0, x], zb] == 0
    return dict(case, name=case["name"] + "_impossible", ev=ev, codes=C.to_codes(ev))


def observed_counts(spec, ev_batch):
    """The integer family counts of fully observed sequences by np.add.at: (tables0, tables1) in fp64."""
    n = len(spec["card"])
    off0, off1, total0, total1 = layout(spec)
    tables = [np.zeros(total0), np.zeros(total1)]
    ev = ev_batch.astype(np.int64)
    for t in range(ev.shape[1]):
        for v, (cols, tab) in enumerate(spec["fam1"] if t else spec["fam0"]):
            at = tuple(ev[:, t - 1, c] if (t and c < n) else ev[:, t, c % n] for c in cols)
            np.add.at(tables[1 if t else 0], (off1 if t else off0)[v] + np.ravel_multi_index(at, tab.shape), 1.0)
    return tables
