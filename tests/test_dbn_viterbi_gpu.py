"""Viterbi decoding on the device (pgmpy_amd/csrc/pgmdbn.hip, k_dbn_viterbi; DBNInference.viterbi_codes /
viterbi_batch / map_query) against the long-double restatement of tests/viterbi_cases.py, per sequence, by the rule
of viterbi_cases.differs: impossible matches; logmap within max(16 d, 64 * 2^-53) relative to max(|logmap|, 1), d
being numpy's own fp64 deviation on the case; the path EQUAL to the restatement's when its optimum is separated by
4 (T + 1)(n + 3) u, else consistent with the evidence and as probable as the optimum.  On the random-table cases no
sequence is in the second class (asserted; tests/test_dbn_viterbi_cpu.py shows it on the CPU); on the power-of-two tie
cases the path has to be equal with no margin at all.  tests/test_dbn_viterbi_cpu.py shows that this rule sees every
structural fault of viterbi_cases.FAULTS on these cases (profiles/dbn_viterbi_fault_table.json).  Each comparison
prints its worst logmap error and what was allowed.

A record, not a bound (MI355X, 2026-10-21, one run; the data is seeded, so a run repeats it): every path of every case
passed the rule (2 sequences each of doc_free_J8_S2 and doc_predict through its below-margin branch); the worst relative logmap error
2.5e-16 (vit_hmm_T12_B13) among the cases of T <= 12, allowed 7.11e-15, the floor, in all of them; 1.5e-15 at
T = 2,000, allowed 2.5e-14; log_probability_codes(path) against logmap in the round trip 8.5e-16.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest

from tests import dbn_cases as C
from tests import viterbi_cases as V
from tests.test_dbn_gpu import _assert_path, _device, _host, _inference

pytestmark = pytest.mark.gpu


def _viterbi(case, inf=None, **kwargs):
    """(paths [B, T + 1, n], logmap [B], impossible [B]) of viterbi_codes, on the host."""
    inf = inf or _inference(case["spec"])
    path, logmap, flags = inf.viterbi_codes(_device(case["codes"]), observed=case["clamped"], **kwargs)
    assert path.element_size() == 1 and tuple(path.shape) == case["codes"].shape
    path = _host(path)
    B = path.shape[1]
    return np.ascontiguousarray(path.T).reshape(B, -1, len(case["spec"]["card"])), _host(logmap), _host(flags)


def _check_case(case, rows=None, inf=None):
    rows = list(range(case["B"])) if rows is None else list(rows)
    exact = case["name"] in V.tie_cases()
    tol = C.tolerance(V.golden_d(case, None if len(rows) == case["B"] else tuple(rows)))
    inf = inf or _inference(case["spec"])
    if "expect" in case:
        _assert_path(case, inf)
    paths, logmap, flags = _viterbi(case, inf)
    assert paths.shape == (case["B"], case["T"] + 1, len(case["spec"]["card"])) and logmap.shape == flags.shape == (case["B"],)
    if not exact and case["name"] not in V.HAND_TABLES:
        assert V.below_margin(case, rows) == [], "a random-table case whose exact path comparison would test nothing"
    worst = 0.0
    for b in rows:
        why = V.differs(case, b, (paths[b], logmap[b], flags[b]), tol, exact)
        assert why is None, (case["name"], b, why)
        if not flags[b]:
            wl = V.reference(case, b)[1]
            worst = max(worst, float(abs(logmap[b] - wl) / max(abs(wl), 1.0)))
    print(f"{case['name']}: logmap {worst:.3g} (allowed {tol:.3g}), {len(rows)} paths, "
          f"{len(V.below_margin(case, rows))} of them below the margin")
    return paths, logmap, flags


CASES = sorted(V.all_cases())


@pytest.mark.parametrize("name", CASES)
def test_device_matches_long_double_viterbi(gpu, name):
    """Every sequence of every case: the branch and path cases of dbn_cases run through Viterbi, the shapes of
    viterbi_cases.shape_cases() (the HMM shape at B = 13, T = 12 with a partly idle last wave; two sequences per wave
    with idle lanes; lanes striding over x' at J = 130 and at J = S = 3,072, the launch that needs the kernel's own
    hipFuncSetAttribute; fully observed sequences) and the tie cases, whose paths are compared exactly."""
    case = V.all_cases()[name]
    inf = _inference(case["spec"])
    info = inf.plan(case["clamped"], []).info
    if name in ("vit_J3072_T3_B2", "J3072_S3072", "n255_all_clamped"):
        assert info.lds_bytes > 65536
    if name == "vit_hmm_T12_B13":
        assert (info.n_configs, info.n_interface, info.seq_per_wave) == (8, 8, 8) and case["B"] % 8 and case["T"] == 12
    if name == "vit_J130_S130":
        assert 64 < info.n_configs <= 256 and info.seq_per_wave == 1
    _check_case(case, inf=inf)


@pytest.mark.parametrize("name", ["n255_all_clamped", "vit_doc_observed", "vit_two_iface_observed"])
def test_observed_sequences_come_back_with_their_loglik(gpu, name):
    """Nothing left to choose (every node clamped: J = 1, 64 sequences per wave; or every cell of the free nodes
    observed): path is the input, logmap is pgm_dbn_run's loglik within the tolerance of both."""
    case = V.all_cases()[name]
    inf = _inference(case["spec"])
    paths, logmap, flags = _viterbi(case, inf)
    assert np.array_equal(paths, case["ev"]) and not flags.any()
    loglik, _ = inf.log_likelihood_codes(_device(case["codes"]), observed=case["clamped"])
    tol = C.tolerance(V.golden_d(case)) + C.tolerance(C.golden_d(case)[1])
    worst = float(np.max(np.abs(logmap - _host(loglik)) / np.maximum(np.abs(logmap), 1.0)))
    print(f"{name}: logmap against loglik {worst:.3g} (allowed {tol:.3g})")
    assert worst <= tol


@pytest.mark.parametrize("name", ["iface_clamped_2_3", "two_iface"])
def test_family_order_does_not_change_the_bits(gpu, name):
    from pgmpy_amd import engine as E
    from pgmpy_amd.inference._dbn import DbnPlan, flat_values

    case = C.kernel_cases()[name]
    inf = _inference(case["spec"])
    n = len(inf.names)
    clamped, queried = [v in case["clamped"] for v in inf.names], [0] * n
    perm0, perm1 = list(range(n))[::-1], list(range(1, n)) + [0]
    ordered = DbnPlan(inf.card, clamped, queried, inf.families0, inf.families1)
    permuted = DbnPlan(inf.card, clamped, queried, [inf.families0[i] for i in perm0], [inf.families1[i] for i in perm1])
    tables = (E.to_device(flat_values([inf.cpds0[i] for i in perm0])), E.to_device(flat_values([inf.cpds1[i] for i in perm1])))
    want = [_host(x) for x in ordered.viterbi(_device(case["codes"]), *inf._tables())]
    got = [_host(x) for x in permuted.viterbi(_device(case["codes"]), *tables)]
    assert np.isfinite(want[1]).all() and not want[2].any()
    assert [x.tobytes() for x in got] == [x.tobytes() for x in want]


def test_card254_code_edge(gpu):
    """In the column of the 254-state node: 253 is its last state, 255 is "not observed", 254 is refused."""
    case = C.path_cases()["card254"]
    inf = _inference(case["spec"])
    b, t = 1, 2
    for code in (253, C.MISSING):
        ev = case["ev"].copy()
        ev[b, t, 0] = code
        paths, _, _ = _check_case(dict(case, name=f"card254_cell{code}", ev=ev, codes=C.to_codes(ev)), inf=inf)
        assert code == C.MISSING or paths[b, t, 0] == 253
    ev = case["ev"].copy()
    ev[b, t, 0] = 254
    with pytest.raises(ValueError, match="dbn_viterbi"):
        inf.viterbi_codes(_device(C.to_codes(ev)), observed=case["clamped"])


def test_bad_codes_are_refused(gpu):
    case = C.kernel_cases()["doc_J2_T1_B63"]
    inf = _inference(case["spec"])
    for row, col, code in ((7, 0, C.MISSING), (9, 3, 2), (11, 2, 5)):  # a clamped cell missing; codes >= card
        codes = case["codes"].copy()
        codes[col, row] = code
        with pytest.raises(ValueError, match="dbn_viterbi"):
            inf.viterbi_codes(_device(codes), observed=case["clamped"])
    _check_case(case, inf=inf)  # and the handle still works


def test_uniform_model_decodes_to_state_zero(gpu):
    """Every completion is as probable as every other: the lowest state wins in every unobserved cell."""
    for name in ("tie_uniform", "tie_uniform_free"):
        case = V.tie_cases()[name]
        paths, logmap, flags = _viterbi(case)
        hidden = case["ev"] == C.MISSING
        assert hidden.any() and (paths[hidden] == 0).all() and np.array_equal(paths[~hidden], case["ev"][~hidden])
        assert not flags.any() and np.isfinite(logmap).all()


def test_bit_identity_across_positions_and_splits(gpu):
    """One sequence alone, at rows 0 and 77 of 130, and in a batch split into row windows by a small scratch: the
    bytes of its path column and the bits of its logmap are the same in all of them."""
    case = C.kernel_cases()["J15_S3"]
    inf = _inference(case["spec"])
    seq = case["codes"][:, 5:6]
    batch = case["codes"].copy()
    batch[:, 0] = batch[:, 77] = seq[:, 0]
    alone = _viterbi(dict(case, codes=np.ascontiguousarray(seq)), inf)
    whole = _viterbi(dict(case, codes=batch), inf)
    per_row = inf.plan(case["clamped"], []).viterbi_scratch_bytes(1, case["T"] + 1)
    assert per_row == case["T"] * 15 * 2
    split = _viterbi(dict(case, codes=batch), inf, scratch_bytes=7 * per_row)  # 19 launches of 7 rows, 77 = 11 x 7
    for x, y, z in zip(alone, whole, split):
        assert x[0].tobytes() == y[0].tobytes() == y[77].tobytes() == z[0].tobytes() == z[77].tobytes()
        assert y.tobytes() == z.tobytes()
    assert not whole[2].any()


def test_windows(gpu):
    """Rows [3, 3 + B) of a codes buffer eight columns wider whose other columns hold 200 (no state, not "missing":
    read, it would raise the flag), and the path written at row0_out = 5 of a buffer prefilled with 0xAB: the window
    has the bytes of the tight run and no byte outside it changes."""
    import torch

    from pgmpy_amd import _native as N

    case = C.kernel_cases()["J65_S65"]
    inf = _inference(case["spec"])
    plan, (v0, v1), B = inf.plan(case["clamped"], []), inf._tables(), case["B"]
    assert max(case["spec"]["card"]) <= 200
    tight = [_host(x) for x in plan.viterbi(_device(case["codes"]), v0, v1)]
    wide = np.full((case["codes"].shape[0], B + 8), 200, dtype=np.uint8)
    wide[:, 3:3 + B] = case["codes"]
    got = [_host(x) for x in plan.viterbi(_device(wide), v0, v1, n_rows=B, row0=3)]
    assert [x.tobytes() for x in got] == [x.tobytes() for x in tight] and not got[2].any()
    n_cols, ld_out = wide.shape[0], B + 11
    out = torch.full((n_cols, ld_out), 0xAB, dtype=torch.uint8, device="cuda")
    logmap = torch.empty(B, dtype=torch.float64, device="cuda")
    scratch = torch.empty(plan.viterbi_scratch_bytes(B, case["T"] + 1) // 2, dtype=torch.int16, device="cuda")
    codes = _device(wide)
    N.check(N.lib().pgm_dbn_viterbi(plan._h, N.ptr(codes), n_cols, B + 8, 3, B, case["T"] + 1, N.ptr(v0), N.ptr(v1), N.ptr(out),
                                    ld_out, 5, N.ptr(logmap), None, N.ptr(scratch), scratch.numel() * 2, N.stream_handle()),
            "dbn_viterbi")
    out = _host(out)
    assert out[:, 5:5 + B].tobytes() == tight[0].tobytes() and _host(logmap).tobytes() == tight[1].tobytes()
    assert (out[:, :5] == 0xAB).all() and (out[:, 5 + B:] == 0xAB).all()


def test_dead_sequences(gpu):
    """One sequence impossible at slice 0 and one only at the last slice, in a wave they share with live ones: 255 in
    every free cell (the observed ones too), the clamped cells copied, -inf and the flag; the live sequences have the
    bytes of the run without the dead ones."""
    case = C.kernel_cases()["deterministic"]
    spec, T = case["spec"], case["T"]
    inf = _inference(spec)
    spw = inf.plan(case["clamped"], []).info.seq_per_wave
    first, late = 29, 31
    assert spw > 1 and first // spw == late // spw and first % spw and late % spw
    clean = _viterbi(case, inf)
    ev = case["ev"].copy()
    for b, t in ((first, 0), (late, T)):
        # X is a deterministic function of Z within a slice: observe Z = 0 and the X it excludes; Y stays as sampled
        x_of_z = np.argmax(spec["fam1" if t else "fam0"][0][1], axis=0)
        ev[b, :, 0] = ev[b, :, 2] = C.MISSING
        ev[b, t, 2], ev[b, t, 0] = 0, 1 - x_of_z[0]
    dirty = dict(case, name="deterministic_two_dead", ev=ev, codes=C.to_codes(ev))
    paths, logmap, flags = _viterbi(dirty, inf)
    for b in (first, late):
        assert V.reference(dirty, b)[2], "the sequence was built to be impossible"
        assert flags[b] == 1 and logmap[b] == -np.inf
        assert (paths[b][:, [0, 2]] == C.MISSING).all() and np.array_equal(paths[b][:, 1], ev[b][:, 1])
        assert V.differs(dirty, b, (paths[b], logmap[b], flags[b]), 0.0) is None
    keep = np.ones(case["B"], dtype=bool)
    keep[[first, late]] = False
    assert flags.sum() == 2
    for x, y in zip((paths, logmap, flags), clean):
        assert x[keep].tobytes() == y[keep].tobytes()


def test_long_sequence(gpu):
    """T = 2,000 on the HMM shape: without the division by c_t delta underflows near slice 400 and a possible
    sequence would be reported impossible.  One sequence against the restatement; all of them finite and
    consistent with what was observed."""
    case = V.long_case()
    paths, logmap, flags = _check_case(case, rows=[0])
    assert not flags.any() and np.isfinite(logmap).all() and (logmap < -1000).all()
    seen = case["ev"] != C.MISSING
    assert np.array_equal(paths[seen], case["ev"][seen]) and (paths[:, :, 0] < 8).all()


# The doc network's patterns are those of viterbi_cases.golden_patterns whose min_margin is not 0 (its P(Z_0) = (0.5,
# 0.5) ties maxima off the best path on the others).  The two-interface network has 16 nodes at T = 3 and a factor of
# VariableElimination holds 12 variables at most, so its patterns observe four cells: 12 unobserved nodes.
ENGINE_PATTERNS = {
    "doc": [{}, {("Z", 3): 0, ("Y", 1): 1}, {("Z", 0): 0, ("X", 2): 1}, {("Z", 0): 1, ("Z", 2): 0, ("Y", 3): 0}],
    "two_iface": [{("Y", t): t % 2 for t in range(4)}, {("W", 0): 1, ("Z", 0): 1, ("Y", 0): 0, ("Y", 2): 1},
                  {("W", 1): 1, ("Y", 2): 0, ("X", 3): 1, ("Z", 3): 0}, {("Z", 1): 0, ("W", 2): 1, ("X", 0): 1, ("Y", 3): 0}],
}


def test_an_independent_engine_agrees(gpu):
    """The project's own VariableElimination.map_query over every unobserved node of the network unrolled to T = 3
    returns the assignment DBNInference.map_query returns.  The patterns are ones whose min_margin is above 1e-6
    (asserted): on a tie two correct engines may differ."""
    from pgmpy_amd.inference import VariableElimination

    T = 3
    for net, spec in C.golden_networks().items():
        model = C.to_model(spec)
        inf = _inference(spec)
        bn, columns = model.unroll(T + 1)
        ve = VariableElimination(bn)
        for pat, ev in enumerate(ENGINE_PATTERNS[net]):
            assert V.viterbi(spec, [], C.evidence_array(spec, ev, T))[3] > 1e-6, (net, pat)
            hidden = [(name, t) for t in range(T + 1) for name in spec["names"] if (name, t) not in ev]
            got = inf.map_query(hidden, ev)  # the variables carry the sequence to slice T whatever the evidence
            want = ve.map_query(variables=[f"{name}_{t}" for name, t in hidden],
                                evidence={f"{name}_{t}": s for (name, t), s in ev.items()}, show_progress=False)
            assert got == {(name, t): want[f"{name}_{t}"] for name, t in hidden}, (net, pat)
            # `variables` only selects entries of the joint optimum
            assert inf.map_query([hidden[0], hidden[-1]], ev) == {k: got[k] for k in (hidden[0], hidden[-1])}


def test_reference_map_queries(gpu):
    """map_query and viterbi_batch against the reference's VariableElimination.map_query on the unrolled networks
    (tests/golden/dbn_viterbi.json): the state names of every unobserved node and the log-probability of the
    completed sequence; and an impossible row of a frame: NaN in its unobserved cells, -inf, the flag, the rows beside
    it untouched."""
    golden = V.load_golden()
    for net in ("doc", "two_iface"):
        spec = C.golden_spec(C.load_golden(), net)
        inf = _inference(spec)
        recs = [r for r in golden["queries"] if r["network"] == net]
        assert len(recs) >= 5
        T = recs[0]["T"]
        frame = {(name, t): [np.nan] * len(recs) for t in range(T + 1) for name in spec["names"]}
        for i, rec in enumerate(recs):
            ev = {(k[0], int(k[1])): int(s) for k, s in rec["evidence"]}
            want = {(k[0], int(k[1])): int(s) for k, s in rec["map"]}
            assert inf.map_query(variables=list(want), evidence=ev) == want, (net, rec["pattern"])
            for k, s in ev.items():
                frame[k][i] = s
        df = pd.DataFrame({j: col for j, col in enumerate(frame.values())})
        df.columns = pd.Index(list(frame), tupleize_cols=False)
        res = inf.viterbi_batch(df)
        seqs = res.sequences()
        assert list(seqs.columns) == [(name, t) for t in range(T + 1) for name in spec["names"]] and len(seqs) == len(recs)
        assert not res.impossible.any()
        for i, rec in enumerate(recs):
            full = {**{(k[0], int(k[1])): int(s) for k, s in rec["evidence"]}, **{(k[0], int(k[1])): int(s) for k, s in rec["map"]}}
            assert {k: int(seqs[k][i]) for k in seqs.columns} == full, (net, rec["pattern"])
            assert abs(res.log_probability[i] - rec["log_probability"]) <= 1e-12 * max(abs(rec["log_probability"]), 1)
    dead = golden["impossible"]
    spec = C.golden_spec(golden, dead["network"])
    inf = _inference(spec)
    ev = {(k[0], int(k[1])): int(s) for k, s in dead["evidence"]}
    with pytest.raises(ValueError, match="probability 0"):
        inf.map_query(evidence=ev)
    T = dead["T"]
    keys = [(name, t) for t in range(T + 1) for name in spec["names"]]
    rows = [[ev.get(k, np.nan) for k in keys], [0 if k == ("Y", 1) else np.nan for k in keys]]
    df = pd.DataFrame(rows)
    df.columns = pd.Index(keys, tupleize_cols=False)
    res = inf.viterbi_batch(df)
    seqs = res.sequences()
    assert list(res.impossible) == [True, False] and res.log_probability[0] == -np.inf and np.isfinite(res.log_probability[1])
    assert seqs.iloc[0].isna().all() and not seqs.iloc[1].isna().any()  # no node is observed in every cell: all are free
    assert {k: int(s) for k, s in seqs.iloc[1].items() if k != ("Y", 1)} == inf.map_query(evidence={("Y", 1): 0}, variables=[k for k in keys if k != ("Y", 1)])


def test_round_trip_on_resident_codes(gpu):
    """simulate_codes -> viterbi_codes -> log_probability_codes of the unrolled network, nothing leaving the device:
    the returned path is a code matrix the rest of the project reads, and its log-probability is logmap."""
    import torch

    from pgmpy_amd.metrics import BayesianModelProbability

    spec = C.hmm_spec()
    model, T1, B = C.to_model(spec), 6, 500
    inf = _inference(spec)
    codes = model.simulate_codes(B, T1, seed=9)
    hidden = codes.clone()
    hidden[0::9] = C.MISSING  # H, node 0 of every slice, is not observed
    path, logmap, flags = inf.viterbi_codes(hidden, observed=spec["names"][1:])
    assert path.is_cuda and tuple(path.shape) == tuple(codes.shape) and not bool(flags.any())
    keep = torch.ones(codes.shape[0], dtype=torch.bool, device=codes.device)
    keep[0::9] = False
    assert bool((path[keep] == codes[keep]).all()) and bool((path[0::9] < 8).all())
    logp, _ = BayesianModelProbability(model.unroll(T1)[0]).log_probability_codes(path)
    got, want = _host(logp)[:B], _host(logmap)
    case = dict(name="round_trip_hmm", spec=spec, clamped=spec["names"][1:], T=T1 - 1, B=B,
                ev=np.ascontiguousarray(_host(hidden).T).reshape(B, T1, 9))
    tol = C.tolerance(V.golden_d(case, tuple(range(8))))
    worst = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)))
    print(f"round trip: log_probability_codes(path) against logmap {worst:.3g} (allowed {tol:.3g})")
    assert worst <= tol
    # and the most probable completion is at least as probable as the sequence that was sampled
    assert (_host(BayesianModelProbability(model.unroll(T1)[0]).log_probability_codes(codes)[0])[:B] <= want + 1e-9).all()
