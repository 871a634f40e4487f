"""Viterbi decoding of a dynamic network without a device: the numpy restatement (tests/viterbi_cases.py) against
brute-force argmax over the unrolled network and against the recorded reference, the structural faults the rule of the
device tests has to see, the host-side argument checks of pgm_dbn_viterbi, and the symbol."""
import ctypes
import json

import numpy as np
import pytest

from tests import dbn_cases as C
from tests import viterbi_cases as V


def _small_specs():
    return {"doc": C.doc_spec(), "two_iface": C.make_spec(seed=72, **C.TWO_IFACE), "cross": C.make_spec(seed=70, **C.CROSS)}


def _evidence(spec, T, seed, hide):
    full = C.sample(spec, T, 6, seed)
    rng = np.random.default_rng(seed + 1)
    ev = full.copy()
    ev[rng.random(ev.shape) < hide] = C.MISSING
    return ev


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("name", ["doc", "two_iface", "cross"])
def test_restatement_equals_enumeration(name):
    """The path is the brute-force argmax of the unrolled joint and logmap its logarithm to 1e-15 relative, with
    nothing clamped and with the always-observed nodes clamped; random patterns at T = 1 .. 3 and fixed ones with
    interface evidence at t >= 1.  Every optimum is separated, so there is one argmax to agree on."""
    spec = _small_specs()[name]
    iface = sorted({p for p, _ in spec["inter"]})
    evs = [e for T in (1, 2, 3) for e in _evidence(spec, T, 400 + T, 0.6)]
    evs += [np.full((1, len(spec["card"])), C.MISSING, dtype=np.uint8)]
    evs += [C.evidence_array(spec, {(iface[0], 1): 1, ("Y", 2): 0}, 3), C.evidence_array(spec, {(iface[-1], 2): 0, (iface[0], 3): 1}, 3),
            C.evidence_array(spec, {(iface[0], 3): 0}, 3)]
    separated = 0
    for ev in evs:
        want_path, want_l, gap = V.enumerate_map(spec, ev)
        # the docstring network's P(Z_0) = (0.5, 0.5) ties two completions on some patterns: there the path need
        # only be AN optimum; everywhere else it is the one argmax
        assert gap > 1e-9 or (name == "doc" and gap == 0)
        separated += gap > 1e-9
        seen = (ev != C.MISSING).all(axis=0)
        for clamped in ([], [v for v, s in zip(spec["names"], seen) if s]):
            path, l, dead, margin = V.viterbi(spec, clamped, ev)
            assert not dead and (gap == 0 or np.array_equal(path, want_path))
            assert abs(l - want_l) <= 1e-15 * max(abs(want_l), 1)
            assert margin >= 0 and abs(V.path_logprob(spec, ev, path) - want_l) <= 1e-15 * max(abs(want_l), 1)
    assert separated >= 15


def test_restatement_on_impossible_and_tied_evidence():
    det = C.kernel_cases()["deterministic"]
    spec = det["spec"]
    x_of_z = np.argmax(spec["fam0"][0][1], axis=0)
    ev = C.evidence_array(spec, {("Z", 0): 0, ("X", 0): 1 - int(x_of_z[0]), ("Y", 1): 1}, 2)
    path, l, dead, _ = V.viterbi(spec, [], ev)
    assert dead and l == -np.inf and (path == C.MISSING).all()  # every FREE cell, the observed ones too
    path, l, dead, _ = V.viterbi(spec, ["Y"], C.evidence_array(spec, {("Z", 0): 0, ("X", 0): 1 - int(x_of_z[0]), ("Y", 0): 0, ("Y", 1): 1}, 1))
    assert dead and l == -np.inf and (path[:, [0, 2]] == C.MISSING).all() and list(path[:, 1]) == [0, 1]  # clamped cells copied
    # the all-uniform model: every completion has the same probability, the lowest states win
    for name in ("tie_uniform", "tie_uniform_free"):
        case = V.tie_cases()[name]
        for b in range(case["B"]):
            path, _, dead, margin = V.reference(case, b)
            assert not dead and margin == 0 and (path[case["ev"][b] == C.MISSING] == 0).all()
    assert any((V.reference(V.tie_cases()[name], b)[0][V.tie_cases()[name]["ev"][b] == C.MISSING] != 0).any()
               for name in ("tie_pow2_S8", "tie_pow2_S4_R4", "tie_pow2_free") for b in range(8))


def test_random_table_cases_have_separated_optima():
    """What lets the device tests compare paths exactly: on every random-table case no sequence's min_margin is
    below 4 (T + 1)(n + 3) u.  The tie cases are the opposite on purpose: their margin is 0."""
    for name, case in V.all_cases().items():
        if name in V.FAULT_SKIP:
            continue  # seconds per run: the device tests assert it on the sequences they run
        if name in V.tie_cases():
            assert min(V.reference(case, b)[3] for b in range(case["B"])) == 0, name
        elif name in V.HAND_TABLES:
            assert 0 < len(V.below_margin(case)) < case["B"], name  # both classes of the rule are reached
        else:
            assert V.below_margin(case) == [], name


def test_rule_sees_structural_faults():
    """Every fault of viterbi_cases.FAULTS, applied to the fp64 run of the restatement, is told from the long-double
    run by the rule the device tests use, on at least three device cases; the all-tie and the long case see the
    faults that need them.  The table is profiles/dbn_viterbi_fault_table.json."""
    table = V.fault_table()
    assert len(V.FAULTS) == 6 and set(table) == (set(V.all_cases()) - set(V.FAULT_SKIP)) | {"vit_hmm_T2000"}
    for fault in V.FAULTS:
        seen = [name for name, row in table.items() if row[fault]]
        assert len(seen) >= 3, (fault, seen)
    assert any(table[name]["ties_last"] for name in V.tie_cases())
    assert table["vit_hmm_T2000"]["no_scale"]
    with open(V.FAULT_TABLE) as f:
        recorded = json.load(f)
    assert recorded["table"] == table and recorded["faults"] == V.FAULTS


def test_goldens_equal_restatement():
    """The reference's VariableElimination.map_query on the unrolled network, recorded by
    tests/golden/make_golden_viterbi.py: the same assignment and log-probability (1e-12) from the restatement."""
    golden = V.load_golden()
    assert len(golden["queries"]) >= 10
    for rec in golden["queries"]:
        spec = C.golden_spec(C.load_golden(), rec["network"])
        ev = C.evidence_array(spec, {(k[0], int(k[1])): int(s) for k, s in rec["evidence"]}, rec["T"])
        path, l, dead, margin = V.viterbi(spec, [], ev)
        assert not dead and margin >= 0 and rec["gap"] > 1e-6
        want ={(k[0], int(k[1])): int(s) for k, s in rec["map"]}
        assert {(spec["names"][v], t): int(path[t, v]) for t in range(rec["T"] + 1) for v in range(len(spec["card"]))
                if ev[t, v] == C.MISSING} == want
        assert abs(float(l) - rec["log_probability"]) <= 1e-12 * max(abs(rec["log_probability"]), 1)
    dead = golden["impossible"]
    spec = C.golden_spec(golden, dead["network"])
    ev = C.evidence_array(spec, {(k[0], int(k[1])): int(s) for k, s in dead["evidence"]}, dead["T"])
    assert V.viterbi(spec, [], ev)[2]


# ------------------------------------------------------------------------------------------------ the host side
def test_symbol_and_abi():
    import pgmpy_amd
    from pgmpy_amd import _native as N

    lib = N.load_library()
    assert "pgm_dbn_viterbi" in N.EXPORTED and len(lib.pgm_dbn_viterbi.argtypes) == 17
    assert lib.pgm_version() == 25 and pgmpy_amd.ABI_VERSION == 25


def test_scratch_bytes():
    from pgmpy_amd.inference._dbn import DbnPlan

    p = DbnPlan([3, 5, 2], [0, 0, 1], [1, 1, 1], [([v], [k]) for v, k in enumerate([3, 5, 2])],
                [([3 + v, v], [k, k]) for v, k in enumerate([3, 5, 2])])
    assert p.info.n_configs == 15 and p.viterbi_scratch_bytes(10, 7) == 10 * 6 * 15 * 2 and p.viterbi_scratch_bytes(10, 1) == 0
    assert p.info.lds_bytes >= p.info.seq_per_wave * (8 * 15 + 8 * 15 + 4 * 15 + 6 * 3)  # delta, m, argx, cl / ev


def test_viterbi_refuses_bad_arguments_without_a_device():
    from pgmpy_amd import _native as N
    from pgmpy_amd.inference._dbn import DbnPlan

    L = N.load_library()
    p = DbnPlan([2, 3], [0, 1], [1, 1], [([0], [2]), ([1], [3])], [([2, 0], [2, 2]), ([3, 1], [3, 3])])
    assert p.info.n_configs == 2
    buf = np.zeros(8192, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 64
    need = 16 * 2 * 2 * 2  # n_rows x (slices - 1) x J x 2

    def run(plan=p._h, codes=base, n_cols=6, ld=16, row0=0, n_rows=16, n_slices=3, v0=base, v1=base, path=base, ld_out=16,
            row0_out=0, logmap=None, scratch=base, scratch_bytes=need):
        return L.pgm_dbn_viterbi(plan, codes, n_cols, ld, row0, n_rows, n_slices, v0, v1, path, ld_out, row0_out, logmap, None,
                                 scratch, scratch_bytes, None)

    for kwargs, message in (
            (dict(plan=None), "null plan"), (dict(codes=None), "null codes"), (dict(v0=None), "null codes / values"),
            (dict(v1=None), "null codes / values"), (dict(path=None), "null path"),
            (dict(v0=base + 4), "not 8-byte aligned"), (dict(v1=base + 2), "not 8-byte aligned"),
            (dict(logmap=base + 4), "not 8-byte aligned"),
            (dict(n_cols=5), "5 code columns"), (dict(n_slices=2), "6 code columns"), (dict(n_slices=0, n_cols=0), "0 slices"),
            (dict(n_slices=65536, n_cols=131072), "65536 slices"),
            (dict(row0=1), "outside ld 16"), (dict(n_rows=17, ld_out=32), "outside ld 16"), (dict(row0=-1), "outside ld 16"),
            (dict(row0_out=1), "outside ld_out 16"), (dict(ld_out=15), "outside ld_out 15"), (dict(row0_out=-1), "outside ld_out"),
            (dict(scratch_bytes=need - 2), "bytes of scratch"), (dict(scratch=None), "bytes of scratch"),
            (dict(scratch_bytes=-1), "bytes of scratch"), (dict(scratch=base + 1), "2-byte aligned")):
        assert run(**kwargs) == N.PGM_EINVAL, kwargs
        assert "dbn_viterbi" in N.last_error() and message in N.last_error(), (kwargs, N.last_error())
    # an empty window is fine and launches nothing: no device is needed for it, and no scratch
    assert run(n_rows=0) == N.PGM_OK and run(n_rows=0, row0=16, row0_out=16, scratch=None, scratch_bytes=0) == N.PGM_OK


def test_compute_needs_a_device(monkeypatch):
    import pandas as pd
    import torch

    from pgmpy_amd import _native as N
    from pgmpy_amd._native import NativeUnavailable
    from pgmpy_amd.inference import DBNInference

    N.load_library()
    monkeypatch.setattr(N, "_device_ok", False)  # as on a machine without a device, wherever this runs
    inf = DBNInference(C.to_model(C.doc_spec()))
    df = pd.DataFrame({("Y", 0): [0, 1], ("Y", 1): [1, np.nan]})
    for call in (lambda: inf.map_query(evidence={("Y", 0): 0}), lambda: inf.viterbi_batch(df),
                 lambda: inf.viterbi_codes(torch.zeros((6, 4), dtype=torch.uint8), observed=["X", "Y"])):
        with pytest.raises(NativeUnavailable):
            call()
    assert inf.map_query(variables=[]) == {}
    with pytest.raises(ValueError, match="not in the model"):
        inf.map_query(evidence={("Q", 0): 0})
