"""The crafted cases of tests/crafted_cases.py without a GPU: that every table holds what it is built for, the host
builds of the two p-value functions (pgm_chi2_sf through tools/ci_selftest.cpp --sf, pgm_ibeta_half through
pgm_lgs_ibeta_half) on the very grids the device runs in tests/test_crafted_gpu.py, and the negative controls of
the EMI tables."""
import ctypes
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import ci_cases as C
from tests import crafted_cases as K
from tests import fit_cases as F
from tests import pair_cases as PC
from tests import score_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- Q(a, x)
def test_gamma_q_is_mpmath_gammainc_where_that_answers():
    import mpmath as mp

    with mp.workdps(K.DPS):
        for a, x in ((0.5, 0.05), (0.5, 700.0), (1.0, 2.0), (5.0, 3.0), (50.0, 60.0), (500.0, 450.0), (2500.0, 2600.0)):
            q, p = K.gamma_q(a, x)
            want = mp.gammainc(a, x, mp.inf, regularized=True)
            assert abs(q - want) <= mp.mpf(10) ** -45 * want and abs(p + q - 1) <= mp.mpf(10) ** -45, (a, x)
        assert abs(K.gamma_q(1.0, 2.0)[0] - mp.exp(-2)) <= mp.mpf(10) ** -48


def test_chi2_grid_is_covered():
    """Every achieved stat / dof is within 10 % of its target, the tail points lie between the smallest normal fp64
    and 1e-300, the ratio 20 underflows to 0 from dof = 100 on, and the builder's formula (4 delta^2 / m per stratum,
    dof 1 each) is what ci_cases.ci_ref computes."""
    assert K.DOFS == (1, 2, 3, 10, 100, 1000, 5000, 20000, 65025, 100000)
    for dof in K.DOFS:
        cases = K.chi2_cases(dof)
        assert [c["target"] for c in cases[:10]] == K.ratios(dof) and int(np.prod(cases[0]["cards"][2:])) == dof
        for c in cases:
            assert abs(c["ratio"] - c["target"]) <= 0.1 * c["target"], (dof, c["target"], c["ratio"])
            assert c["table"].shape == (2, 2, dof) and c["table"].min() > 0
        if dof in K.TAIL_RATIOS:
            p, _ = K.q_tol(dof, cases[-1]["ratio"] * dof)
            assert K.TINY < p < 1e-300, (dof, p)
        p20, tol20 = K.q_tol(dof, cases[9]["ratio"] * dof)
        assert (p20 == 0.0 and tol20 == K.TINY) if dof >= 100 else p20 > 0.0
    for dof in (1, 3, 100):
        for c in K.chi2_cases(dof):
            stat, d, _, mag, cells = C.ci_ref(c["table"], 1.0, yates=False)
            assert d == dof and abs(float(stat) - c["ratio"] * dof) <= C.bound(cells, mag)
    for c in K.general_cases():
        t = c["table"][:, :, 0]
        assert c["dof"] == 253 ** 2 == 64009 and abs(c["ratio"] - c["target"]) <= 0.1 * c["target"]
        assert t.min() > 0 and (t.sum(axis=0) == 254 * K.M_SMALL).all() and (t.sum(axis=1) == 254 * K.M_SMALL).all()
        assert 254 + 254 > C.SMALL
        d = (t - K.M_SMALL).astype(np.float64)
        assert abs((d * d).sum() / K.M_SMALL - c["ratio"] * c["dof"]) <= 1e-9 * c["ratio"] * c["dof"]


def _host_chi2_sf(tmp_path, points):
    """pgm_chi2_sf(stat, dof) of the host build for [(dof, stat)], through tools/ci_selftest.cpp --sf."""
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe, args = str(tmp_path / "ci_selftest"), str(tmp_path / "args.txt")
    with open(args, "w") as f:
        for dof, stat in points:
            f.write(f"{float(dof).hex()} {float(stat).hex()}\n")
    csrc = os.path.join(ROOT, "pgmpy_amd", "csrc")
    built = subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                            os.path.join(ROOT, "tools", "ci_selftest.cpp"), os.path.join(csrc, "pgmfit_plan.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe, "--sf", args], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    got = [float.fromhex(line.split()[1]) for line in run.stdout.splitlines() if line.startswith("sf ")]
    assert len(got) == len(points)
    return got


def test_host_chi2_sf_stays_inside_q_tol(tmp_path):
    """The host build of pgm_chi2_sf against mpmath at 50 digits under crafted_cases.q_tol, on the grid the device
    runs (every dof and ratio of chi2_cases, the tails, the general-path dof 253^2) and at dof 10^6.  Measured
    2026-10-21 on the host libm: the worst error / bound is 0.30 (dof 100, stat 89.87); at dof 10^6 the error is
    2.6e-10 of p against a bound of 5.8e-9, at dof 5,000 1.7e-12 against 1.7e-11."""
    points = []
    for dof in K.DOFS:
        points += [(dof, c["ratio"] * dof) for c in K.chi2_cases(dof)]
    points += [(c["dof"], c["ratio"] * c["dof"]) for c in K.general_cases()]
    points += [(10 ** 6, r * 10 ** 6) for r in K.ratios(10 ** 6)]
    got = _host_chi2_sf(tmp_path, points)
    worst = {}
    for (dof, stat), p in zip(points, got):
        want, tol = K.q_tol(dof, stat)
        ratio = abs(p - want) / tol if tol else (0.0 if p == want else math.inf)
        if ratio >= worst.get(dof, (-1.0,))[0]:
            worst[dof] = (ratio, stat, p, want, tol)
    for dof, w in worst.items():
        print(f"host dof {dof}: worst error / bound {w[0]:.3g} at stat {w[1]!r}: {w[2]!r} against {w[3]!r}, bound {w[4]:.3g}")
    assert all(w[0] <= 1.0 for w in worst.values()), {d: w for d, w in worst.items() if w[0] > 1.0}
    assert got[0] == 1.0  # stat 0


# ---------------------------------------------------------------------------- large-count CI tables
def test_large_ci_cases_are_past_2_to_the_53():
    cases = K.large_ci_cases()
    assert [c["cards"] for c in cases[-2:]] == [[3, 3, 130], [9, 8, 3]]
    assert 3 + 3 <= C.SMALL < 9 + 8 and 130 > C.CHUNK
    for c in cases:
        t = c["table"]
        R, Cc = t.sum(axis=1), t.sum(axis=0)
        assert t.min() > 0 and int(R.min()) * int(Cc.min()) > 2 ** 53 and int(t.sum(axis=(0, 1)).max()) < 2 ** 53
    ref = K.large_ci_reference(1.0, False)
    for c, (stat, dof, _, _, _) in zip(cases, ref):
        assert dof == c["dof"]
        if c["ratio"] is not None:
            assert abs(float(stat) - c["ratio"] * dof) <= 1e-9 * float(stat)
        else:
            assert 0.5 < float(stat) / dof < 2.0


# ---------------------------------------------------------------------------- bad codes
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("ld_kind", ["odd", "mult4"])
@pytest.mark.parametrize("path", ["lds", "global"])
def test_bad_code_case_holds_a_missing_code_before_the_bad_one(path, ld_kind, where):
    fams, codes, n_rows, row = K.bad_code_case(path, ld_kind, where)
    assert (codes.shape[1] % 4 == 0) == (ld_kind == "mult4") and codes.shape[1] % 2 == (ld_kind == "odd")
    assert row == (0 if where == "first" else n_rows - 1) and (ld_kind == "odd" or n_rows % 4 == 3)
    assert (max(F.layout(fams)[1]) > 4096) == (path == "global")
    fam = next((cols, cards) for cols, cards in fams if codes[cols[-1], row] == cards[-1])
    assert codes[fam[0][0], row] == F.MISSING and len(fam[0]) == 2
    with pytest.raises(IndexError):
        F.count_ref(codes, fams, n_rows=n_rows)
    codes[fam[0][1], row] = 0
    F.count_ref(codes, fams, n_rows=n_rows)  # it was the only bad code


# ---------------------------------------------------------------------------- EMI tables
def test_pair_tables_hold_the_starts_they_are_named_for():
    def shifts(t):
        t = np.asarray(t)
        return sorted(int(a + b - t.sum()) for a in t.sum(axis=1) for b in t.sum(axis=0) if a > 0 and b > 0)

    assert max(shifts(K.PAIR_TABLES["shift_is_1"])) == 1 and max(shifts(K.PAIR_TABLES["shift_is_2"])) == 2
    assert np.asarray(K.PAIR_TABLES["marginal_is_N"]).sum(axis=1)[0] == np.asarray(K.PAIR_TABLES["marginal_is_N"]).sum()
    assert max(shifts(K.PAIR_TABLES["t10"])) == 5 and max(shifts(K.PAIR_TABLES["t50"])) == 17
    assert max(shifts(K.PAIR_TABLES["t1000"])) == 890
    for name, t in K.scale_tables().items():
        assert t.shape == (4, 4) and t.sum() == K.SCALE_N == 1 << 20 and t.min() > 0
        assert (max(shifts(t)) > 1) == (name == "scale_skewed")


@pytest.mark.parametrize("name", list(K.PAIR_TABLES))
def test_emi_without_the_first_term_of_a_shifted_cell_is_outside_the_bound(name):
    """The negative control of the EMI bound on the small tables: the restatement's sum with the term at n = a + b - N
    of a cell left out (what a start one step late does) differs from it by more than pair_cases.emi_bound.
    shift_is_1 takes the cell whose a + b - N is exactly 1.  Where a marginal is N the EMI and each of its terms are
    exactly 0 (log N + log b - log N - log b), so that table has no control: its value is 0 whatever the start."""
    st = K.pair_reference(name)
    bound = PC.emi_bound(st["emi"])
    terms = K.first_terms(K.PAIR_TABLES[name], least=1 if name == "shift_is_1" else 2)
    print(name, "emi", float(st["emi"][0]), "bound", bound, "first terms", {k: float(v) for k, v in terms.items()})
    assert terms
    if name == "marginal_is_N":
        assert float(st["emi"][0]) == 0.0 and all(float(v) == 0.0 for v in terms.values())
        return
    assert max(abs(float(v)) for v in terms.values()) > 1e4 * bound


def test_emi_bound_at_scale_is_of_the_size_of_the_emi():
    """At N = 2^20 the signed terms of the EMI cancel: the bound (taken from the sum of their magnitudes) is of the
    value's own size, so the scale tables guard the scale (overflow, a lost range of n), not the last digits."""
    for name in K.scale_tables():
        st = K.pair_reference(name)
        emi, bound = float(st["emi"][0]), PC.emi_bound(st["emi"])
        print(name, emi, bound)
        assert 0.1 * emi < bound < 10 * emi and PC.bound(st["mi"]) < 1e-10 * float(st["mi"][0])  # MI keeps its digits


# ---------------------------------------------------------------------------- the Pearson p-value
def test_pearson_grid_covers_both_fractions():
    grid = K.pearson_grid()
    assert {n for n, _, _ in grid} == set(K.PEARSON_N) | {1, 2} and len(grid) == 12 * len(K.PEARSON_N) + 2
    for n in K.PEARSON_N:
        a = 0.5 * (n - 2.0)
        lo, hi = K.pearson_switch(n)
        assert 1.0 - lo * lo < (a + 1.0) / (a + 2.5) <= 1.0 - hi * hi
    assert any(r < 0 for _, r, _ in grid)


def test_host_ibeta_half_stays_inside_ibeta_rel():
    """pgm_lgs_ibeta_half (the host build of the code the kernel runs) on the grid of the device test.  Measured
    2026-10-21: the worst error / bound is 0.43 (n = 10^4, t = 30); at n = 10^6 it is 0.23 (8.0e-12 of p, t = 5), at
    n = 10^8 0.28 (2.5e-10 of p, t = 10)."""
    from pgmpy_amd import _native as N

    L = N.load_library()
    out = ctypes.c_double()
    worst = {}
    for n, r, tag in K.pearson_grid():
        want, tol = K.pearson_reference(n, r)
        if n <= 2:
            continue
        assert L.pgm_lgs_ibeta_half(0.5 * (n - 2.0), r * r, ctypes.byref(out)) == N.PGM_OK
        err = abs(out.value - want)
        assert err <= tol, (n, tag, out.value, want, tol)
        if tol and err / tol >= worst.get(n, (-1.0,))[0]:
            worst[n] = (err / tol, tag, err / want if want else 0.0)
    for n, w in worst.items():
        print(f"host n {n}: worst error / bound {w[0]:.3g} at {w[1]} (relative error {w[2]:.3g})")


# ---------------------------------------------------------------------------- Gaussian scores
def test_score_G_has_exact_residuals():
    """rss = G_vv - sum_k G_vk^2 / G_kk in exact rational arithmetic is the fp64 the builder states, and every
    quantity the kernel forms on the way (1 / sqrt(G_kk), the scaled entries, the products) is a power of two times a
    small integer."""
    for n in K.SCORE_N:
        g = K.score_G(n)
        s = K.SCORE_SCALE[n]
        assert 0.25 * n <= s <= 4 * n and math.sqrt(s) == int(math.sqrt(s)) and g[3, 3] == n and not g[:3, 3].any()
        for parents, cols in enumerate(([], [1], [1, 2])):
            exact = Fraction(g[0, 0]) - sum(Fraction(g[0, k]) ** 2 / Fraction(g[k, k]) for k in cols)
            _, _, rss = K.score_reference(n, parents, "ll")
            assert Fraction(rss) == exact and g[1, 2] == 0.0
            assert all(math.sqrt(g[k, k]) ** 2 == g[k, k] for k in cols)
        score, tol, rss = K.score_reference(n, 2, "bic")
        closed = -0.5 * n * (math.log(2 * math.pi * rss / n) + 1.0) - 2.0 * math.log(n)
        assert abs(score - closed) <= tol


# ---------------------------------------------------------------------------- structure scores
def test_score_counts_hold_what_they_are_for():
    t = K.score_tables()
    assert [x.shape for x in t] == [(4, 1), (3, 4), (254, 1), (3, 129), (3, 4), (5, 1)] and 129 == S.CHUNK + 1
    allc = K.score_counts()
    assert allc.min() == 0 and allc.max() == K.BIG and (allc == 0).mean() > 0.1
    assert ((allc > 0) & (allc < 1024)).sum() > 10 and (allc > 2 ** 30).sum() > 10  # log-uniform: every decade
    assert (t[4] == K.BIG).all() and (t[3][:, 5] > 0).sum() == 1 and not t[3][:, 7].any() and not t[3][:, 128].any()
    assert (t[5].sum(axis=1) == 0).sum() == 1 and max(int(x.sum(axis=0).max()) for x in t) < 2 ** 53
    lg, lo = K.score_arguments()
    assert len(lg) > 1000 and lg.max() > K.BIG and lo.max() >= 3 * K.BIG and lg.min() > 0 and lo.min() >= 1
    # the restatement is finite in every mode
    for kind in ("k2", "bdeu"):
        alpha, beta = K.score_params(kind)
        for mode in (S.BD, S.BD | S.SKIP_EMPTY):
            assert np.isfinite(S.score_ref(allc, K.SCORE_FAMILIES, mode, alpha, beta)[0].astype(np.float64)).all()
    assert np.isfinite(S.score_ref(allc, K.SCORE_FAMILIES, S.LL)[0].astype(np.float64)).all()


def test_ulp_argument_file(tmp_path):
    path = str(tmp_path / "args.txt")
    n_lg, n_lo = K.write_ulp_arguments(path)
    with open(path) as f:
        lines = f.read().split("\n")[:-1]
    assert len(lines) == n_lg + n_lo and lines[0].startswith("lgamma 0x") and lines[-1].startswith("log 0x")
    assert float.fromhex(lines[-1].split()[1]) == K.score_arguments()[1].max()
