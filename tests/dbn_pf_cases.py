"""The dynamic-network particle filter restated in numpy float64 and integers, independently of the C++
(pgmpy_amd/csrc/pgmdbn_pf.hip, pgmdbn_pf_plan.cpp), and the cases the CPU and GPU tests share.  ``run`` is the contract
of include/pgmhip.h ("dynamic Bayesian networks: the particle filter") for one sequence, on the forward sampler's stream
(tests/sample_cases).  A SPEC and its evidence [T, n] are tests/dbn_cases's.
"""
import functools

import numpy as np

from tests import dbn_cases as C
from tests import sample_cases as SC

MISSING = 255
RESAMPLE = 0x52534D50  # PGM_DBN_PF_RESAMPLE
IMPOSSIBLE, BAD = 1, 2


def plan_order(n, fams, base):
    """Kahn over the edges within the slice (parent columns base .. base + n - 1), the lowest ready node first."""
    order, done = [], set()
    while len(order) < n:
        v = min(v for v in range(n) if v not in done
                and all(c - base in done for c in fams[v][0][1:] if base <= c < base + n))
        order.append(v)
        done.add(v)
    return order


def run(spec, ev, N, seed, first_row=0, queried=None):
    """One sequence: dict(filter [T, Q], ess [T], loglik, flag, anc [T, N] uint16, traj [T, queried nodes, N] uint8)."""
    card, n = spec["card"], len(spec["card"])
    T = ev.shape[0]
    qnodes = [v for v in range(n) if queried is None or spec["names"][v] in queried]
    qoff = np.concatenate([[0], np.cumsum([card[v] for v in qnodes])]).astype(np.int64)
    out = {"filter": np.full((T, int(qoff[-1])), np.nan), "ess": np.full(T, np.nan), "loglik": 0.0, "flag": 0,
           "anc": np.tile(np.arange(N, dtype=np.uint16), (T, 1)), "traj": np.full((T, len(qnodes), N), MISSING, dtype=np.uint8)}
    if any(ev[t, v] != MISSING and ev[t, v] >= card[v] for t in range(T) for v in range(n)):
        out.update(loglik=np.nan, flag=BAD)
        return out
    orders = [plan_order(n, spec["fam0"], 0), plan_order(n, spec["fam1"], n)]
    rows = np.uint64(first_row) + np.arange(N, dtype=np.uint64)
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    prev = None
    for t in range(T):
        fams = spec["fam1"] if t else spec["fam0"]
        cur = np.zeros((n, N), dtype=np.int64)
        w = np.ones(N, dtype=np.float64)
        for v in orders[min(t, 1)]:
            cols, tab = fams[v]
            tab = np.asarray(tab, dtype=np.float64).reshape(card[v], -1)
            cdf = SC.running_sums(tab)
            col = np.zeros(N, dtype=np.int64)
            for c in cols[1:]:
                col = col * card[c % n] + (prev[c] if t and c < n else cur[c % n])
            g = int(ev[t, v])
            if g == MISSING:
                cur[v] = SC.select(cdf[:, col], SC.uniforms(seed, rows, t * n + v))
            else:
                cur[v] = g
                w = w * (tab[g, col] / cdf[-1, col])
        out["traj"][t] = cur[qnodes]
        wmax = float(w.max())
        if not wmax > 0:
            out.update(loglik=-np.inf, flag=IMPOSSIBLE)
            return out
        q = np.ldexp(w / wmax, 36).astype(np.uint64)  # truncation of a value <= 2^36
        scan = np.cumsum(q, dtype=np.uint64)
        Q = int(scan[-1])
        hist = np.zeros(int(qoff[-1]), dtype=np.uint64)
        for k, v in enumerate(qnodes):
            np.add.at(hist, qoff[k] + cur[v], q)
        out["filter"][t] = hist.astype(np.float64) / float(Q)
        q1 = q >> np.uint64(16)
        s1, s2 = int(q1.sum(dtype=np.uint64)), int((q1 * q1).sum(dtype=np.uint64))
        out["ess"][t] = float(s1) * float(s1) / float(s2)
        out["loglik"] = out["loglik"] + (np.log(wmax) + np.log(float(Q) * 2.0 ** -36 / N))
        r0 = int(first_row)
        x = SC.philox4x32_10((r0 & 0xFFFFFFFF, r0 >> 32, t, RESAMPLE), key)
        m = (int(x[0]) << 21) | (int(x[1]) >> 11)
        r = ((m << 11) * Q) >> 64
        thr = np.arange(N, dtype=np.uint64) * np.uint64(Q) + np.uint64(r)
        anc = np.searchsorted(np.uint64(N) * scan, thr, side="right")  # min{i : N C_i > j Q + r}
        out["anc"][t] = anc
        prev = cur[:, anc]
    return out


def trace(anc, traj):
    """[T queried nodes, N]: i_{T-1} = a_{T-1}[j], i_{t-1} = a_{t-1}[i_t]."""
    T, nq, N = traj.shape
    out, i = np.empty((T * nq, N), dtype=np.uint8), np.arange(N)
    for t in range(T - 1, -1, -1):
        i = anc[t][i].astype(np.int64)
        out[t * nq:(t + 1) * nq] = traj[t][:, i]
    return out


def margin(p, ess):
    """Six standard errors of a self-normalised importance estimate at the reported effective sample size, plus one
    particle.  Heuristic: a resampled filter has no closed-form error.  The restatement alone stays inside it on the
    seeds used (DESIGN.md "Dynamic networks" has the ratios); a miss means the filter is wrong, not the constant."""
    return 6.0 * np.sqrt(p * (1.0 - p) / ess) + 1.0 / ess


# ------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def specs():
    return {"doc": C.make_spec(seed=201, **C.DOC), "two_iface": C.make_spec(seed=202, **C.TWO_IFACE),
            "cross": C.make_spec(seed=203, **C.CROSS), "factorial2": C.make_spec(seed=204, **C._chains(2))}


@functools.lru_cache(maxsize=None)
def evidence(name, T, B=3):
    """[B, T, n] uint8: sampled sequences of spec `name`, every cell hidden with probability one half."""
    return C._case(name, specs()[name], [], T - 1, B, 210 + T, hide=0.5)["ev"]


@functools.lru_cache(maxsize=None)
def reference(name, T, N, seed=7, first_row=0, b=0):
    """The restatement of sequence b of evidence(name, T): computed once, shared, never written to."""
    return run(specs()[name], evidence(name, T)[b], N, seed, first_row=first_row)


def chain_spec(k):
    """k binary hidden chains H00 .., each with its own observed binary child O00 ..: J = 2^k hidden joint states,
    and given their own observations the chains are independent."""
    hidden, obs = [f"H{i:02d}" for i in range(k)], [f"O{i:02d}" for i in range(k)]
    return C.make_spec(names=hidden + obs, card=[2] * (2 * k), intra=list(zip(hidden, obs)),
                       inter=[(h, h) for h in hidden], seed=220)


def one_chain(spec, i, k):
    """The two-node spec (H, O) of chain i of chain_spec(k), with that chain's tables."""
    n = 2 * k
    sub = {"names": ["H", "O"], "card": [2, 2], "intra": [("H", "O")], "inter": [("H", "H")], "order": [0, 1]}
    sub["fam0"] = [([0], spec["fam0"][i][1]), ([1, 0], spec["fam0"][k + i][1])]
    sub["fam1"] = [([2, 0], spec["fam1"][i][1]), ([3, 2], spec["fam1"][k + i][1])]
    assert spec["fam1"][i][0] == [n + i, i] and spec["fam1"][k + i][0] == [n + k + i, n + i]
    return sub
