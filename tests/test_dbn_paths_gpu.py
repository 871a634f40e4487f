"""The dynamic-network filter (pgmpy_amd/csrc/pgmdbn.hip, pgmdbn_plan.cpp) on the paths its branch cases stop short
of: the launch with more than 64 KiB of dynamic LDS from both sides (n = 255 with everything clamped, J = S = 3,072),
the benchmarked HMM shape, two sequences per wave, a node of 254 states, a sequence that dies at slice 0 or only at the
last slice, a row window inside a wider buffer, queried subsets, and families given out of node order.  The shapes are
tests/dbn_cases.path_cases(); test_dbn_gpu.test_device_matches_long_double_recursion walks them with the branch cases
and asserts each one's plan geometry.  Every comparison with the long-double restatement is under the rule of
dbn_cases.tolerance, max(16 d, 64 * 2^-53), d being numpy's own fp64 deviation on the case; tests/test_dbn_cpu.py shows
that this bound sees a structural fault on every case (profiles/dbn_fault_table.json).  Each test prints its worst
error and what was allowed.

Worst error / allowed (MI355X, 2026-10-21, one run of this module and of test_dbn_gpu; the data is seeded, so a run
repeats it).  Allowed was the floor, 64 * 2^-53 = 7.11e-15, in every row: 16 d stayed below it on all of these cases.
                                    filter     smooth     loglik
  hmm_J8_S8_n9                      0.020      0.026      0.032
  mixed_J30_S6                      0.016      0.031      0.010
  card254                           0.0003     0.0005     0.0013
  card254, cell set to 253 / 255    0.0003     0.0005     0.019 / 0.010
  n255_all_clamped                  0 (exact indicators)  0.025
  J3072_S3072                       0.031      0.031      0.0045
  deterministic, dead at last       0.009 over the finite filter entries (dead at slice 0 has none)
The window, subset and family-order tests compare bytes.  A record, not a bound.  Against the library as it stood
before this module, test_family_order_does_not_change_the_bits failed on both cases: the plan numbered a family by its
place in the caller's list, so the factors of a product were multiplied in that order and the last bits moved.
"""
import numpy as np
import pytest

from tests import dbn_cases as C
from tests.test_dbn_gpu import _assert_path, _check_case, _device, _host, _inference, _run

pytestmark = pytest.mark.gpu


def _outputs(plan, codes, tables, **window):
    """(filter, smooth, loglik, flags) of a direct plan.run, on the host."""
    f, s, l, flags = plan.run(_device(codes), *tables, want_filter=True, want_smooth=True, **window)
    return _host(f), _host(s), _host(l), _host(flags)


def _differing(a, b):
    """The names of the outputs (filter, smooth, loglik, flags) whose bytes differ."""
    return [what for what, x, y in zip(("filter", "smooth", "loglik", "flags"), a, b)
            if x.shape != y.shape or x.tobytes() != y.tobytes()]


def test_n255_all_clamped_yields_indicators(gpu):
    """n at its limit, J = 1, 64 sequences per wave, 99,456 bytes of LDS: exact indicators, loglik within the rule."""
    case = C.path_cases()["n255_all_clamped"]
    inf = _inference(case["spec"])
    _assert_path(case, inf)
    f, s, lf, ls, flags = _run(case, inf)
    ev = case["ev"]  # [B, T + 1, n]; every node is binary, so node v's states are columns 2 v and 2 v + 1
    hot = (np.arange(2)[None, None, None, :] == ev[:, :, :, None]).astype(np.float64).reshape(case["B"], case["T"] + 1, -1)
    assert np.array_equal(f, hot) and np.array_equal(s, hot)
    assert not flags.any() and lf.tobytes() == ls.tobytes()
    tol = C.tolerance(C.golden_d(case)[1])
    worst = max(float(abs(lf[b] - C.reference(case, b)[2]) / max(abs(C.reference(case, b)[2]), 1.0)) for b in range(case["B"]))
    print(f"n255_all_clamped indicators: loglik {worst:.3g} (allowed {tol:.3g})")
    assert worst <= tol


@pytest.mark.parametrize("where", ["slice0", "last"])
def test_dead_sequence_positions(gpu, where):
    """A sequence whose evidence becomes impossible at slice 0, or only at the last slice, inside a wave it shares
    with live sequences: the pattern of NaN, -inf and the flag is the restatement's; every other sequence has the
    bytes of the clean run."""
    case = C.kernel_cases()["deterministic"]
    spec, n, T, b = case["spec"], 3, case["T"], 31
    inf = _inference(spec)
    assert 1 < inf.plan(case["clamped"]).info.seq_per_wave and b % inf.plan(case["clamped"]).info.seq_per_wave
    clean = _run(case, inf)
    # X is a deterministic function of Z within a slice: observe Z = 0 and the X it excludes; Y stays as sampled
    t = 0 if where == "slice0" else T
    x_of_z = np.argmax(spec["fam1" if t else "fam0"][0][1], axis=0)
    ev = case["ev"].copy()
    ev[b, :, 0] = ev[b, :, 2] = C.MISSING
    ev[b, t, 2], ev[b, t, 0] = 0, 1 - x_of_z[0]
    f, s, lf, ls, flags = _run(dict(case, codes=C.to_codes(ev)), inf)
    wf, ws, wl, dead = C.recursion(spec, case["clamped"], ev[b])
    assert dead, "the sequence was built to be impossible"
    w64 = C.recursion(spec, case["clamped"], ev[b], np.float64)[0]
    alive = ~np.isnan(wf)
    assert alive[:t].all() and not alive[t:].any()
    d = float(np.abs(w64[alive] - wf[alive]).max()) if alive.any() else 0.0
    tol = C.tolerance(d)
    assert np.array_equal(np.isnan(f[b]), np.isnan(wf)) and np.array_equal(np.isnan(s[b]), np.isnan(ws))
    worst = float(np.abs(f[b][alive] - wf[alive]).max()) if alive.any() else 0.0
    print(f"deterministic, dead at {where}: finite filter entries {worst:.3g} (allowed {tol:.3g})")
    assert worst <= tol
    assert lf[b] == float(wl) and ls[b] == float(wl) and flags[b] == int(dead) and flags.sum() == 1
    keep = np.arange(case["B"]) != b
    for x, y in zip((f, s, lf, ls), clean[:4]):
        assert x[keep].tobytes() == y[keep].tobytes()


@pytest.mark.parametrize("name", ["J15_S3", "J65_S65"])
def test_window_inside_a_wider_buffer(gpu, name):
    """Rows [3, 3 + B) of a buffer [(T + 1) n, B + 8] whose other columns hold 200, no state and not "missing":
    nothing outside the window is read (no ValueError), and the outputs have the bytes of the tight buffer's."""
    case = C.kernel_cases()[name]
    inf = _inference(case["spec"])
    plan, tables, B = inf.plan(case["clamped"]), inf._tables(), case["B"]
    assert max(case["spec"]["card"]) <= 200
    tight = _outputs(plan, case["codes"], tables)
    wide = np.full((case["codes"].shape[0], B + 8), 200, dtype=np.uint8)
    wide[:, 3:3 + B] = case["codes"]
    got = _outputs(plan, wide, tables, n_rows=B, row0=3)
    assert got[0].shape == (B, case["T"] + 1, sum(case["spec"]["card"]))
    assert _differing(got, tight) == [] and not got[3].any()


@pytest.mark.parametrize("name", ["two_iface", "mixed_J30_S6"])
def test_queried_subsets_are_columns_of_the_full_query(gpu, name):
    """filter_codes / smooth_codes of a subset (without the first node, without the last) are the subset's columns
    of the full query bit for bit; log_likelihood_codes (Q = 0) has the filter's loglik bits and flags."""
    case = C.all_cases()[name]
    inf = _inference(case["spec"])
    codes, observed, names = _device(case["codes"]), case["clamped"], case["spec"]["names"]
    full_plan = inf.plan(observed)
    full = {"filter": inf.filter_codes(codes, observed), "smooth": inf.smooth_codes(codes, observed)}
    for subset in (names[1:], names[:-1]):
        cols = np.concatenate([np.arange(sum(case["spec"]["card"]))[full_plan.query_slices[names.index(v)]] for v in subset])
        assert inf.plan(observed, subset).n_query == len(cols) < full_plan.n_query
        for kind, call in (("filter", inf.filter_codes), ("smooth", inf.smooth_codes)):
            m, l, flags = call(codes, observed, variables=subset)
            want_m, want_l, want_flags = full[kind]
            assert _host(m).tobytes() == np.ascontiguousarray(_host(want_m)[:, :, cols]).tobytes(), (kind, subset)
            assert _host(l).tobytes() == _host(want_l).tobytes() and _host(flags).tobytes() == _host(want_flags).tobytes()
    l, flags = inf.log_likelihood_codes(codes, observed)
    assert inf.plan(observed, []).n_query == 0
    assert _host(l).tobytes() == _host(full["filter"][1]).tobytes() and _host(flags).tobytes() == _host(full["filter"][2]).tobytes()


@pytest.mark.parametrize("name", ["iface_clamped_2_3", "two_iface"])
def test_family_order_does_not_change_the_bits(gpu, name):
    """A plan built with both family sets permuted (each its own way) and the values laid out in that order gives
    the bytes of the node-ordered plan: the tables are found where the given order put them, and the factors of a
    product are multiplied in node order."""
    from pgmpy_amd import engine as E
    from pgmpy_amd.inference._dbn import DbnPlan, flat_values

    case = C.kernel_cases()[name]
    inf = _inference(case["spec"])
    n = len(inf.names)
    clamped, queried = [v in case["clamped"] for v in inf.names], [1] * n
    perm0, perm1 = list(range(n))[::-1], list(range(1, n)) + [0]
    ordered = DbnPlan(inf.card, clamped, queried, inf.families0, inf.families1)
    permuted = DbnPlan(inf.card, clamped, queried, [inf.families0[i] for i in perm0], [inf.families1[i] for i in perm1])
    assert permuted.offsets0 != ordered.offsets0 and permuted.offsets1 != ordered.offsets1
    tables = (E.to_device(flat_values([inf.cpds0[i] for i in perm0])), E.to_device(flat_values([inf.cpds1[i] for i in perm1])))
    want = _outputs(ordered, case["codes"], inf._tables())
    got = _outputs(permuted, case["codes"], tables)
    assert np.isfinite(want[0]).all() and not want[3].any()
    assert _differing(got, want) == []


def test_card254_code_edge(gpu):
    """Beside PGM_EV_MISSING: in the column of the 254-state node a code 254 is refused, 253 is its last state and
    255 is "not observed"."""
    case = C.path_cases()["card254"]
    assert (case["ev"][:, :, 0] == 253).any(), "state 253 is observed in the case as it stands"
    inf = _inference(case["spec"])
    b, t = 1, 2
    for code in (253, C.MISSING):
        ev = case["ev"].copy()
        ev[b, t, 0] = code
        _check_case(dict(case, name=f"card254_cell{code}", ev=ev, codes=C.to_codes(ev)))
    ev = case["ev"].copy()
    ev[b, t, 0] = 254
    with pytest.raises(ValueError, match="dbn_run"):
        inf.filter_codes(_device(C.to_codes(ev)), observed=case["clamped"])
