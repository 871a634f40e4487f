"""Viterbi decoding of a dynamic network (pgmpy_amd/csrc/pgmdbn.hip, k_dbn_viterbi) restated in numpy, independently
of the C++: the max-product recursion with backpointers and a backtrack, brute-force argmax over the unrolled
network, the rule a device result is held to, structural faults of the restatement, and the seeded cases the CPU and
GPU tests share.  Specs, evidence, cases and ``tolerance`` are those of tests/dbn_cases.py.

``viterbi(spec, clamped, ev, dtype, fault)`` follows include/pgmhip.h ("MAP sequences"): delta over the joint x of the
free nodes, the message m_t(i) = max over the x of interface state i with argx_t(i) the lowest x that attains it,
psi the lowest i that attains max_i m_t(i) prod(i, x'), bp = argx(psi), scaling by c_t = max delta_t, and the
backtrack from the lowest x that attains max delta_T.  It returns (path [T + 1, n], logmap, impossible, min_margin);
min_margin is the smallest relative gap (best - second) / best over every max it took whose winner is > 0 (a max over
one candidate has no gap).

The rule (``differs``).  impossible has to match; logmap within tolerance(d) relative to max(|logmap|, 1), d being the
fp64 restatement's deviation from the long-double one (``golden_d``), as for loglik in dbn_cases.  The path: a
candidate is a product of at most n table factors and one carried value, plus one division per slice, so its relative
error is at most (T + 1)(n + 3) u and two candidates can swap order only inside twice that; with min_margin >=
``margin_bound`` = 4 (T + 1)(n + 3) u the path has to EQUAL the long-double one.  Below that bound the path has to
keep every observed cell and its own log-probability (``path_logprob``, straight from the tables) has to be within
the same tolerance of the optimum.  ``exact=True`` (the power-of-two tie cases, where every product and every division
is exact in both precisions) asks for the equal path without a margin condition.
"""
import functools
import json
import os

import numpy as np

from tests import dbn_cases as C

MISSING, U, LD = C.MISSING, C.U, C.LD

FAULTS = {
    "sum_message": "the message is summed over the interface group instead of maxed",
    "argx_first": "argx is the first x of the interface group instead of the one that attains the max",
    "bp_psi": "the backpointer is stored as psi (an interface index) and followed as a full state",
    "ties_last": "ties go to the last index instead of the first",
    "mask_slice0": "the evidence mask is ignored at slice 0",
    "no_scale": "delta is not divided by c_t",
}


# ------------------------------------------------------------------------------------------------ the recursion
def _first_max(a, axis, last=False):
    """(max, index of the first -- or last -- entry that attains it, second largest or None) along an axis."""
    a = np.moveaxis(a, axis, 0)
    at = a.shape[0] - 1 - np.argmax(a[::-1], axis=0) if last else np.argmax(a, axis=0)
    best = np.take_along_axis(a, at[None], 0)[0]
    second = None
    if a.shape[0] > 1:
        b = a.copy()
        np.put_along_axis(b, at[None], -1, 0)
        second = b.max(axis=0)
    return best, at, second


def viterbi(spec, clamped, ev, dtype=LD, fault=None):
    """(path [T + 1, n] uint8, logmap, impossible, min_margin) of one sequence.  fault: None or a key of FAULTS."""
    assert fault is None or fault in FAULTS
    card, n, names = spec["card"], len(spec["card"]), spec["names"]
    is_clamped = [names[v] in clamped for v in range(n)]
    free = [v for v in range(n) if not is_clamped[v]]
    iface = [v for v in free if any(c == v for cols, _ in spec["fam1"] for c in cols[1:])]
    fshape, ishape = [card[v] for v in free], [card[v] for v in iface]
    J = int(np.prod(fshape)) if free else 1
    S = int(np.prod(ishape)) if iface else 1
    dig = dict(zip(free, np.unravel_index(np.arange(J), fshape))) if free else {}
    idig = dict(zip(iface, np.unravel_index(np.arange(S), ishape))) if iface else {}
    ix = np.ravel_multi_index([dig[v] for v in iface], ishape) if iface else np.zeros(J, dtype=np.int64)
    groups = np.argsort(ix, kind="stable").reshape(S, J // S)  # the x of interface state i, ascending
    T1 = ev.shape[0]
    ev = ev.astype(np.int64)
    for t in range(T1):
        for v in range(n):
            assert ev[t, v] < card[v] or (ev[t, v] == MISSING and not is_clamped[v]), "bad code in a restated case"
    last = fault == "ties_last"
    margin = [np.inf]

    def note(best, second):
        if second is None:
            return
        best, second = np.atleast_1d(best), np.atleast_1d(second)
        ok = best > 0
        if ok.any():
            margin[0] = min(margin[0], float(((best[ok] - second[ok]) / best[ok]).min()))

    def lookup(cols, tab, t):
        at = []
        for c in cols:
            v = c % n
            before = t > 0 and c < n
            if is_clamped[v]:
                at.append(ev[t - 1, v] if before else ev[t, v])
            elif before:
                at.append(idig[v][:, None])
            else:
                at.append(dig[v][None, :])
        return tab.astype(dtype)[tuple(at)]

    def mask(t):
        m = np.ones(J, dtype=bool)
        if fault == "mask_slice0" and t == 0:
            return m
        for v in free:
            if ev[t, v] != MISSING:
                m &= dig[v] == ev[t, v]
        return m

    delta, bps, logmap, dead = None, [], dtype(0), False
    for t in range(T1):
        local, prev = np.ones((1, J), dtype=dtype), []
        for cols, tab in (spec["fam1"] if t else spec["fam0"]):  # node order
            if t > 0 and any(c < n and not is_clamped[c] for c in cols[1:]):
                prev.append((cols, tab))
            else:
                local = local * np.broadcast_to(lookup(cols, tab, t), (1, J))
        local = np.where(mask(t), local[0], dtype(0))
        if t:
            grouped = delta[groups]  # [S, R]
            m, r, second = _first_max(grouped, 1, last)
            note(m, second)
            if fault == "sum_message":
                m = grouped.sum(axis=1)
            argx = groups[:, 0] if fault == "argx_first" else groups[np.arange(S), r]
            cand = np.broadcast_to(m[:, None], (S, J)).copy()
            for cols, tab in prev:
                cand *= lookup(cols, tab, t)
            carried, psi, second = _first_max(cand, 0, last)
            del cand
            un = local * carried
            seen = un > 0
            if second is not None:
                note(carried[seen], second[seen])
            bps.append(psi if fault == "bp_psi" else argx[psi])
        else:
            un = local
        c, at, second = _first_max(un, 0, last)
        if not c > 0:
            dead = True
            break
        note(c, second)
        logmap = logmap + np.log(c)
        delta = un if fault == "no_scale" else un / c
        best = int(at)
    path = np.full((T1, n), MISSING, dtype=np.uint8)
    for v in range(n):
        if is_clamped[v]:
            path[:, v] = ev[:, v]
    if dead:
        return path, dtype(-np.inf), True, margin[0]
    x = best
    for t in range(T1 - 1, -1, -1):
        for v in free:
            path[t, v] = dig[v][x % J]
        if t:
            x = int(bps[t - 1][x % J])
    return path, logmap, False, margin[0]


def path_logprob(spec, ev, path):
    """log P(path) straight from the tables in long double; -inf when the path contradicts the evidence or is not
    complete."""
    n = len(spec["card"])
    path = np.asarray(path).astype(np.int64)
    if (path >= np.asarray(spec["card"])[None, :]).any() or ((ev != MISSING) & (ev != path)).any():
        return LD(-np.inf)
    total = LD(0)
    with np.errstate(divide="ignore"):
        for t in range(path.shape[0]):
            for cols, tab in (spec["fam1"] if t else spec["fam0"]):
                at = tuple(int(path[t - 1, c] if (t and c < n) else path[t, c % n]) for c in cols)
                total = total + np.log(LD(tab[at]))
    return total


def enumerate_map(spec, ev):
    """(path [T + 1, n], logmap, gap) by brute force over the unrolled joint in long double: the first argmax in C
    order (slice-major, node order within a slice: the lowest state at the earliest differing cell), and the relative
    gap to the second largest entry."""
    card, n, T1 = spec["card"], len(spec["card"]), ev.shape[0]
    assert float(np.prod(np.asarray(card, dtype=np.float64))) ** T1 <= 2 ** 20, "too large to enumerate"
    axes = T1 * n
    j = np.ones([1] * axes, dtype=LD)
    for t in range(T1):
        for cols, tab in (spec["fam1"] if t else spec["fam0"]):
            where = [(t - 1) * n + c if (t and c < n) else t * n + c % n for c in cols]
            shape = [1] * axes
            for w, k in zip(where, tab.shape):
                shape[w] = k
            j = j * np.transpose(tab.astype(LD), np.argsort(where)).reshape(shape)
    for t in range(T1):
        for v in range(n):
            if ev[t, v] != MISSING:
                keep = np.zeros(card[v], dtype=LD)
                keep[ev[t, v]] = 1
                shape = [1] * axes
                shape[t * n + v] = card[v]
                j = j * keep.reshape(shape)
    flat = j.reshape(-1)
    at = int(np.argmax(flat))
    best = flat[at]
    rest = np.delete(flat, at)
    gap = float((best - rest.max()) / best) if rest.size and best > 0 else np.inf
    path = np.asarray(np.unravel_index(at, j.shape), dtype=np.uint8).reshape(T1, n)
    return path, np.log(best), gap


# ------------------------------------------------------------------------------------------------ the rule
def margin_bound(case):
    return 4.0 * (case["T"] + 1) * (len(case["spec"]["card"]) + 3) * U


GOLDEN_REF, GOLDEN_D = {}, {}


def reference(case, b):
    """The long-double run of sequence b of a case: computed once, shared, never written to."""
    key = (case["name"], int(b))
    if key not in GOLDEN_REF:
        GOLDEN_REF[key] = viterbi(case["spec"], case["clamped"], case["ev"][b])
    return GOLDEN_REF[key]


def _dev(run64, run_ld):
    return 0.0 if run_ld[2] or run64[2] else float(abs(run64[1] - run_ld[1]) / max(abs(run_ld[1]), LD(1)))


def golden_d(case, rows=None):
    """d of the log-probability: the fp64 restatement against the long-double one, the largest over the sequences."""
    key = (case["name"], None if rows is None else tuple(rows))
    if key not in GOLDEN_D:
        GOLDEN_D[key] = max(_dev(viterbi(case["spec"], case["clamped"], case["ev"][b], np.float64), reference(case, b))
                            for b in (range(case["B"]) if rows is None else rows))
    return GOLDEN_D[key]


def differs(case, b, got, tol, exact=False):
    """Why a result (path [T + 1, n], logmap, impossible) of sequence b breaks the rule, or None."""
    path, logmap, dead = got
    wpath, wl, wdead, margin = reference(case, b)
    ev = case["ev"][b]
    if bool(dead) != bool(wdead):
        return f"impossible {dead}, expected {wdead}"
    if wdead:
        if not np.array_equal(path, wpath):
            return "an impossible sequence's path is not 255 in the free cells and the codes in the clamped ones"
        return None if logmap == -np.inf else f"logmap {logmap} of an impossible sequence"
    if not abs(LD(logmap) - wl) / max(abs(wl), LD(1)) <= tol:
        return f"logmap {logmap} is {float(abs(LD(logmap) - wl) / max(abs(wl), LD(1))):.3g} off (allowed {tol:.3g})"
    if exact or margin >= margin_bound(case):
        return None if np.array_equal(path, wpath) else "the path is not the restatement's"
    if ((ev != MISSING) & (ev != path)).any():
        return "the path contradicts an observed cell"
    lp = path_logprob(case["spec"], ev, path)
    if not abs(lp - wl) / max(abs(wl), LD(1)) <= tol:
        return f"the path's own log-probability {float(lp)} is not the optimum {float(wl)}"
    return None


# the two cases on the docstring network's hand-written tables with Z free: P(Z_0) = (0.5, 0.5) makes exact ties in
# maxima off the best path, so some of their sequences are in the below-margin class.  Every other case that is no
# tie case has random tables and none of its sequences may be.
HAND_TABLES = ("doc_free_J8_S2", "doc_predict")


def below_margin(case, rows=None):
    """The sequences whose optimum is not separated by margin_bound(case)."""
    return [b for b in (range(case["B"]) if rows is None else rows)
            if not reference(case, b)[2] and reference(case, b)[3] < margin_bound(case)]


# ------------------------------------------------------------------------------------------------ cases
def pow2_spec(names, card, intra, inter, seed, uniform=False):
    """A spec whose tables hold powers of two only, every column normalised: cards 2 and 4, a column a permutation
    of (0.5, 0.5), (0.25,) * 4 or (0.5, 0.25, 0.125, 0.125).  uniform: the flat columns alone."""
    spec = C.make_spec(names=names, card=card, intra=intra, inter=inter, seed=seed)
    rng = np.random.default_rng(seed + 1000)

    def redo(tab):
        k = tab.shape[0]
        assert k in (2, 4)
        flat = np.empty((k, tab.size // k))
        for j in range(flat.shape[1]):
            col = np.full(k, 1.0 / k)
            if k == 4 and not uniform and rng.random() < 0.7:
                col = rng.permutation([0.5, 0.25, 0.125, 0.125])
            flat[:, j] = col
        return flat.reshape(tab.shape)

    spec["fam0"] = [(cols, redo(tab)) for cols, tab in spec["fam0"]]
    spec["fam1"] = [(cols, redo(tab)) for cols, tab in spec["fam1"]]
    return spec


TIE = dict(names=["A", "B", "O"], card=[4, 2, 4], intra=[("A", "O"), ("B", "O")], inter=[("A", "A"), ("B", "B"), ("A", "B")])
TIE_SMALL_IFACE = dict(names=["A", "B", "O"], card=[4, 4, 2], intra=[("A", "B"), ("B", "O")], inter=[("A", "A")])


@functools.lru_cache(maxsize=None)
def tie_cases():
    """name -> case: tables of powers of two, so that every product and every division by c_t is exact in fp64 and
    in long double alike and a tie is a tie on the device too."""
    out = [C._case("tie_uniform", pow2_spec(seed=200, uniform=True, **TIE), ["O"], 3, 9, 201, hide=0.7),
           C._case("tie_uniform_free", pow2_spec(seed=202, uniform=True, **TIE), [], 3, 9, 203, hide=0.8),
           C._case("tie_pow2_S8", pow2_spec(seed=204, **TIE), ["O"], 4, 70, 205, hide=0.7),
           C._case("tie_pow2_S4_R4", pow2_spec(seed=206, **TIE_SMALL_IFACE), ["O"], 4, 70, 207, hide=0.7),
           C._case("tie_pow2_free", pow2_spec(seed=208, **TIE_SMALL_IFACE), [], 4, 40, 209, hide=0.8)]
    return {c["name"]: c for c in out}


@functools.lru_cache(maxsize=None)
def shape_cases():
    """name -> case: the shapes of the issue that dbn_cases has no sequence set for; `expect` as in
    dbn_cases.path_cases()."""
    out = []
    hmm = C.hmm_spec()
    # 8 sequences per wave, 13 = one full wave and 5 of the second's 8
    out.append(dict(C._case("vit_hmm_T12_B13", hmm, hmm["names"][1:], 12, 13, 300, hide=0.5),
                    expect=dict(J=8, S=8, spw=8, lds=8 * (8 * 24 + 6 * 9), n_prev=1, n_cur=8)))
    mixed = C.path_cases()["mixed_J30_S6"]
    out.append(dict(C._case("vit_mixed_J30_T5_B7", mixed["spec"], ["O"], 5, 7, 302, hide=0.6), expect=mixed["expect"]))
    # lanes stride over x': J = S = 130 = 10 x 13, two full passes of the wave and two lanes of a third
    s130 = C.make_spec(seed=304, **C._chains(2, card=[10, 13]))
    out.append(dict(C._case("vit_J130_S130", s130, ["O"], 4, 3, 305, hide=0.7),
                    expect=dict(J=130, S=130, spw=1, lds=8 * 3 * 130 + 6 * 3, n_prev=2, n_cur=1)))
    big = C.path_cases()["J3072_S3072"]
    out.append(dict(C._case("vit_J3072_T3_B2", big["spec"], ["O"], 3, 2, 306, hide=0.5), expect=big["expect"]))
    # fully observed sequences of a model whose nodes are all free
    out.append(C._case("vit_doc_observed", C.doc_spec(), [], 4, 40, 308, hide=0.0))
    out.append(C._case("vit_two_iface_observed", C.make_spec(seed=72, **C.TWO_IFACE), [], 3, 40, 309, hide=0.0))
    return {c["name"]: c for c in out}


def long_case():
    """T = 2,000 on the HMM shape: without the division by c_t delta leaves fp64's range."""
    hmm = C.hmm_spec()
    return C._case("vit_hmm_T2000", hmm, hmm["names"][1:], 2000, 3, 310, hide=0.5)


def all_cases():
    """Every case a device run is compared with the restatement on, by the rule of ``differs``."""
    return {**C.all_cases(), **shape_cases(), **tie_cases()}


# the cases the fault table is computed on: every device case but the two whose restatement takes seconds per run
FAULT_SKIP = ("J3072_S3072", "vit_J3072_T3_B2")
FAULT_TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                           "dbn_viterbi_fault_table.json")


def fault_row(case, rows=None):
    """{fault: whether the rule tells the faulted fp64 run from the long-double one on one of the first 16
    sequences of the case}."""
    rows = range(min(case["B"], 16)) if rows is None else rows
    tol = C.tolerance(golden_d(case, tuple(rows)))
    exact = case["name"] in tie_cases()
    with np.errstate(all="ignore"):
        return {f: any(differs(case, b, viterbi(case["spec"], case["clamped"], case["ev"][b], np.float64, fault=f)[:3], tol,
                               exact) is not None for b in rows) for f in FAULTS}


def fault_table():
    table = {name: fault_row(case) for name, case in all_cases().items() if name not in FAULT_SKIP}
    table["vit_hmm_T2000"] = fault_row(long_case(), rows=(0,))
    return table


def fault_table_record():
    """The content of profiles/dbn_viterbi_fault_table.json."""
    return {"what": "whether viterbi_cases.differs (the rule of the device tests) tells viterbi(fp64, fault=...) from the "
                    "long-double run on one of the first 16 sequences of a case (vit_hmm_T2000: the first)",
            "faults": FAULTS, "table": fault_table()}


# ------------------------------------------------------------------------------------------------ goldens
GOLDEN = os.path.join(C.GOLDEN, "dbn_viterbi.json")


def golden_patterns(spec):
    """name -> {(node, t): state}: the evidence the reference's map_query is recorded on, T = 3."""
    iface = sorted({p for p, _ in spec["inter"]})
    return {
        "none": {},
        "leaf_gaps": {("Y", 0): 0, ("Y", 2): 1, ("Y", 3): 1},
        "leaf_all": {("Y", t): t % 2 for t in range(4)},
        "slice0": {**{(v, 0): 1 for v in iface}, ("Y", 0): 0},
        "iface_late": {(iface[0], 1): 1, ("Y", 2): 0, ("X", 3): 1},
        "iface_last": {(iface[-1], 3): 0, ("Y", 1): 1},
    }


@functools.lru_cache(maxsize=None)
def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    with open(FAULT_TABLE, "w") as out:
        json.dump(fault_table_record(), out, indent=1)
        out.write("\n")
    print(f"wrote {FAULT_TABLE}")
