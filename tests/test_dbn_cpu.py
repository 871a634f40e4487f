"""Dynamic networks without a device: the model class against the reference's recorded behaviour, the numpy
restatement against enumeration and the goldens, and the host side of the pgm_dbn plan (geometry, refusals)."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from pgmpy_amd.inference import DBNInference  # noqa: F401  (without the feature the module does not import)
from pgmpy_amd.models import DynamicBayesianNetwork, DynamicNode  # noqa: F401
from tests import dbn_cases as C


def _t(x):
    return (x[0], int(x[1]))


def _edges(es):
    return sorted((_t(u), _t(v)) for u, v in es)


def _doc_model(cpds=True):
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.models import DynamicBayesianNetwork

    m = DynamicBayesianNetwork()
    m.add_edges_from([(("Z", 0), ("X", 0)), (("X", 0), ("Y", 0)), (("Z", 0), ("Z", 1))])
    if cpds:
        m.add_cpds(TabularCPD(("Z", 0), 2, [[0.5], [0.5]]),
                   TabularCPD(("X", 0), 2, [[0.6, 0.9], [0.4, 0.1]], evidence=[("Z", 0)], evidence_card=[2]),
                   TabularCPD(("Y", 0), 2, [[0.2, 0.3], [0.8, 0.7]], evidence=[("X", 0)], evidence_card=[2]),
                   TabularCPD(("Z", 1), 2, [[0.4, 0.7], [0.6, 0.3]], evidence=[("Z", 0)], evidence_card=[2]))
    return m


# ------------------------------------------------------------------------------------------------ the model class
def test_graph_logic_matches_reference():
    g = C.load_golden()["graph"]
    m = _doc_model(cpds=False)
    assert _edges(m.edges()) == _edges(g["edges"])
    assert _edges(m.get_intra_edges()) == _edges(g["intra0"]) and _edges(m.get_intra_edges(3)) == _edges(g["intra3"])
    assert _edges(m.get_inter_edges()) == _edges(g["inter"])
    assert sorted(m.get_interface_nodes(0)) == sorted(map(_t, g["interface0"]))
    assert sorted(m.get_interface_nodes(1)) == sorted(map(_t, g["interface1"]))
    assert sorted(m.get_slice_nodes(2)) == sorted(map(_t, g["slice2"]))
    assert sorted(m.get_constant_bn().edges()) == sorted(tuple(e) for e in g["constant_bn_edges"])
    assert sorted(tuple(sorted(e)) for e in m.moralize().edges()) == sorted(tuple(sorted(map(_t, e))) for e in g["moral_edges"])
    assert sorted(set(m.get_markov_blanket(("Z", 1)))) == sorted(map(_t, g["markov_blanket_Z1"]))
    assert sorted(m._nodes()) == ["X", "Y", "Z"]
    c = m.copy()
    assert _edges(c.edges()) == _edges(m.edges())


def test_edge_and_model_errors_match_reference():
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.models import DynamicBayesianNetwork

    err = C.load_golden()["graph"]["errors"]
    m = _doc_model(cpds=False)
    for name, bad in (("backward", lambda: m.add_edge(("X", 1), ("Z", 0))), ("far", lambda: m.add_edge(("X", 0), ("Z", 2))),
                      ("self", lambda: m.add_edge(("X", 0), ("X", 0))), ("loop", lambda: m.add_edge(("Y", 0), ("Z", 0))),
                      ("shape", lambda: m.add_edge("X", "Z"))):
        with pytest.raises((ValueError, NotImplementedError)) as e:
            bad()
        assert [type(e.value).__name__, str(e.value)] == err[name]
    for name, cpd in (("parents", TabularCPD(("X", 0), 2, [[0.5], [0.5]])),
                      ("sum", TabularCPD(("X", 0), 2, [[0.6, 0.9], [0.3, 0.1]], evidence=[("Z", 0)], evidence_card=[2]))):
        m2 = DynamicBayesianNetwork([(("Z", 0), ("X", 0)), (("Z", 0), ("Z", 1))])
        m2.add_cpds(cpd)
        with pytest.raises(ValueError) as e:
            m2.check_model()
        assert str(e.value) == err["check_" + name][1]
    with pytest.raises(ValueError, match="cpd should be an instance of TabularCPD"):
        m.add_cpds("x")
    with pytest.raises(ValueError, match="CPD defined on variable not in the model"):
        m.add_cpds(TabularCPD(("Q", 0), 2, [[0.5], [0.5]]))
    with pytest.raises(ValueError, match="Only Maximum Likelihood"):
        m.fit(pd.DataFrame({("X", 0): [0]}), estimator="bayes")
    with pytest.raises(ValueError, match="must start from time slice 0"):
        m.fit(pd.DataFrame({("X", 1): [0]}))


def test_initialize_initial_state_and_cpd_bookkeeping():
    from pgmpy_amd.models import DynamicNode

    g = C.load_golden()["graph"]
    m = _doc_model()
    m.initialize_initial_state()
    got = sorted(([_t(v) for v in c.variables], np.asarray(c.get_values()).tolist()) for c in m.get_cpds())
    want = sorted(([_t(v) for v in vs], vals) for vs, vals in g["initialized"])
    assert [a for a, _ in got] == [a for a, _ in want]
    for (_, a), (_, b) in zip(got, want):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-15)
    assert m.check_model() and len(m.get_cpds(time_slice=0)) == 3 and len(m.get_cpds(time_slice=[1])) == 3
    assert m.get_cpds(("Z", 1)).variables[1] == ("Z", 0)
    assert m.states[("X", 1)] == [0, 1]
    cpd = m.get_cpds(("Y", 1))
    m.remove_cpds(cpd)
    assert m.get_cpds(("Y", 1)) is None and len(m.cpds) == 5
    with pytest.raises(ValueError, match="Node not present in the model."):
        m.get_cpds(("Q", 0))
    node = DynamicNode("X", 1)
    assert node == ("X", 1) and hash(node) == hash(("X", 1)) and node.node == "X" and node.time_slice == 1
    assert str(node) == "(X, 1)" and node.to_tuple() == ("X", 1) and DynamicNode("A", 1) < DynamicNode("B", 0)
    with pytest.raises(IndexError):
        node[2]
    m.add_cpds(cpd)
    bn, columns = m.unroll(3)
    assert columns == ["X_0", "Y_0", "Z_0", "X_1", "Y_1", "Z_1", "X_2", "Y_2", "Z_2"]
    assert sorted(bn.edges()) == sorted([("Z_0", "X_0"), ("X_0", "Y_0"), ("Z_0", "Z_1"), ("Z_1", "X_1"), ("X_1", "Y_1"),
                                         ("Z_1", "Z_2"), ("Z_2", "X_2"), ("X_2", "Y_2")])
    assert bn.check_model()


def test_exports():
    import pgmpy_amd.inference as I
    import pgmpy_amd.models as M
    from pgmpy_amd import _native as N

    assert "DynamicBayesianNetwork" in M.__all__ and "DynamicNode" in M.__all__ and "DBNInference" in I.__all__
    lib = N.load_library()
    for name in ("pgm_dbn_plan_create", "pgm_dbn_plan_destroy", "pgm_dbn_info", "pgm_dbn_run"):
        assert name in N.EXPORTED and getattr(lib, name).argtypes is not None
    assert lib.pgm_version() == 25
    import pgmpy_amd

    assert pgmpy_amd.ABI_VERSION == 25


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("case", C.small_cases(), ids=lambda c: c["name"])
def test_long_double_recursion_equals_enumeration(case):
    """1e-15 relative (to the largest entry of a marginal, which is at most 1; to |loglik|)."""
    for ev in case["ev"][:8]:
        f, s, l, dead = C.recursion(case["spec"], case["clamped"], ev)
        ef, es, el = C.enumerate_unrolled(case["spec"], ev)
        assert not dead
        assert float(np.abs(f - ef).max()) <= 1e-15 and float(np.abs(s - es).max()) <= 1e-15
        assert float(abs(l - el)) <= 1e-15 * max(float(abs(el)), 1.0)


def test_goldens_equal_long_double_recursion():
    golden = C.load_golden()
    assert len(golden["queries"]) >= 30
    for rec in golden["queries"]:
        spec = C.golden_spec(golden, rec["network"])
        ev = {_t(k): s for k, s in rec["evidence"]}
        variables = [_t(v) for v in rec["variables"]]
        T = max([t for _, t in variables] + [t for _, t in ev])
        f, s, _, _ = C.recursion(spec, [], C.evidence_array(spec, ev, T))
        off, _ = C.offsets(spec)
        for i, (name, t) in enumerate(variables):
            v = spec["names"].index(name)
            np.testing.assert_allclose(rec["forward"][i], f[t, off[v]:off[v] + spec["card"][v]].astype(float), rtol=0, atol=1e-12)
            if rec["backward"] is not None:
                np.testing.assert_allclose(rec["backward"][i], s[t, off[v]:off[v] + spec["card"][v]].astype(float), rtol=0,
                                           atol=1e-12)
        # the recorded d is this machine's too, up to the order in which numpy's fp64 sums run on it
        for now, then in zip(C.deviation(spec, [], C.evidence_array(spec, ev, T)), rec["d"]):
            assert abs(now - then) <= 4 * C.U and now <= 16 * C.U
    for name, spec in C.golden_networks().items():
        for (c0, t0), (c1, t1) in zip(spec["fam0"] + spec["fam1"],
                                      C.golden_spec(golden, name)["fam0"] + C.golden_spec(golden, name)["fam1"]):
            assert list(c0) == list(c1) and np.array_equal(t0, t1)


def test_recorded_reference_faults_are_faults():
    """Where the reference was recorded although it is wrong, the recorded enumeration is the restatement's."""
    golden = C.load_golden()
    for case in C.interface_evidence_cases():
        rec = golden["interface_evidence"][case["name"]]
        T = max(t for _, t in list(case["evidence"]) + [case["query"]])
        _, s, _, _ = C.recursion(case["spec"], [], C.evidence_array(case["spec"], case["evidence"], T))
        off, _ = C.offsets(case["spec"])
        v = case["spec"]["names"].index(case["query"][0])
        np.testing.assert_allclose(rec["enumerated"], s[case["query"][1], off[v]:off[v] + 2].astype(float), rtol=0, atol=1e-12)
        assert np.abs(np.asarray(rec["reference"]) - np.asarray(rec["enumerated"])).max() > 1e-2
    assert golden["reference_faults"] and all(f["gap"] > 1e-3 for f in golden["reference_faults"])
    assert max(f["gap"] for f in golden["reference_faults"]) > 1e-2


# ------------------------------------------------------------------------------------------------ the plan's host side
def _plan(card, clamped, fam0, fam1, queried=None):
    from pgmpy_amd.inference._dbn import DbnPlan

    return DbnPlan(card, clamped, queried if queried is not None else [1] * len(card), fam0, fam1)


def _chain_families(card):
    """Independent chains: node v has no parent at slice 0 and its own copy as parent afterwards."""
    n = len(card)
    return [([v], [card[v]]) for v in range(n)], [([n + v, v], [card[v], card[v]]) for v in range(n)]


@pytest.mark.parametrize("card,clamped,J,S,spw,prev,cur", [
    ([2, 3], [1, 1], 1, 1, 64, 0, 2),
    ([2, 3], [0, 1], 2, 2, 32, 1, 1),
    ([3, 5, 2], [0, 0, 1], 15, 15, 4, 2, 1),
    ([2] * 6, [0] * 6, 64, 64, 1, 6, 0),
    ([5, 13], [0, 0], 65, 65, 1, 2, 0),
    ([2] * 12, [0] * 12, 4096, 4096, 1, 12, 0),
])
def test_plan_geometry(card, clamped, J, S, spw, prev, cur):
    fam0, fam1 = _chain_families(card)
    p = _plan(card, clamped, fam0, fam1)
    i = p.info
    n = len(card)
    assert (i.n, i.n_configs, i.n_interface, i.seq_per_wave, i.block) == (n, J, S, spw, 64)
    assert (i.n_prev_families, i.n_cur_families, i.n_free) == (prev, cur, n - sum(clamped))
    assert i.lds_bytes == spw * (8 * (J + 2 * S) + 6 * n) and i.lds_bytes <= 160 * 1024
    assert i.scratch_per_slice == S + 1 and i.n_query == sum(card)
    assert i.values0 == sum(card) and i.values1 == sum(k * k for k in card)
    assert p.offsets0 == list(np.cumsum([0] + card[:-1])) and p.offsets1 == list(np.cumsum([0] + [k * k for k in card[:-1]]))
    assert p.scratch_bytes(10, 7) == 10 * 7 * (S + 1) * 8


def _spec_families(spec):
    """The two family sets of a spec as (columns, cardinalities)."""
    n, card = len(spec["card"]), spec["card"]
    return tuple([(list(cols), [card[c % n] for c in cols]) for cols, _ in spec[k]] for k in ("fam0", "fam1"))


@pytest.mark.parametrize("name,J,S,spw,prev,cur,lds", [
    ("hmm_J8_S8_n9", 8, 8, 8, 1, 8, 1968),
    ("mixed_J30_S6", 30, 6, 2, 3, 1, 720),
    ("card254", 254, 254, 1, 1, 1, 6108),
    ("n255_all_clamped", 1, 1, 64, 0, 255, 99456),
    ("J3072_S3072", 3072, 3072, 1, 3, 1, 73752),
])
def test_path_case_geometry(name, J, S, spw, prev, cur, lds):
    """Each case of dbn_cases.path_cases() reaches the path it is there for, and says so in its `expect`."""
    case = C.path_cases()[name]
    spec = case["spec"]
    fam0, fam1 = _spec_families(spec)
    i = _plan(spec["card"], [v in case["clamped"] for v in spec["names"]], fam0, fam1).info
    assert (i.n_configs, i.n_interface, i.seq_per_wave, i.n_prev_families, i.n_cur_families, i.lds_bytes) == (J, S, spw, prev, cur, lds)
    assert case["expect"] == dict(J=J, S=S, spw=spw, n_prev=prev, n_cur=cur, lds=lds)
    assert (lds > 65536) == (name in ("n255_all_clamped", "J3072_S3072"))
    assert i.n == len(spec["card"]) <= 255 and case["codes"].shape == ((case["T"] + 1) * i.n, case["B"])
    if name == "card254":
        assert (case["ev"][:, :, 0] == 253).any()
    if name == "hmm_J8_S8_n9":
        assert case["B"] % spw  # the last wave is partly idle


def test_plan_lds_at_the_64k_edge():
    """An all-clamped chain takes 64 (24 + 6 n) bytes: below 64 KiB at n = 166, above it from n = 167."""
    for n, lds in ((166, 65280), (167, 65664)):
        fam0, fam1 = _chain_families([2] * n)
        i = _plan([2] * n, [1] * n, fam0, fam1).info
        assert (i.n_configs, i.seq_per_wave, i.lds_bytes) == (1, 64, lds) and lds == 64 * (24 + 6 * n)
    assert 65280 <= 65536 < 65664


@pytest.mark.parametrize("name", ["iface_clamped_2_3", "two_iface"])
def test_plan_family_order(name):
    """Families given out of node order: the same geometry, each table where the given order put it."""
    case = C.kernel_cases()[name]
    spec = case["spec"]
    n, clamped = len(spec["card"]), [v in case["clamped"] for v in spec["names"]]
    fam0, fam1 = _spec_families(spec)
    perm0, perm1 = list(range(n))[::-1], list(range(1, n)) + [0]
    a = _plan(spec["card"], clamped, fam0, fam1)
    b = _plan(spec["card"], clamped, [fam0[i] for i in perm0], [fam1[i] for i in perm1])
    for field in ("n_configs", "n_interface", "seq_per_wave", "n_prev_families", "n_cur_families", "lds_bytes", "values0", "values1"):
        assert getattr(a.info, field) == getattr(b.info, field), field
    for perm, fams, off in ((perm0, fam0, b.offsets0), (perm1, fam1, b.offsets1)):
        sizes = [int(np.prod(fams[i][1])) for i in perm]
        assert off == list(np.cumsum([0] + sizes[:-1]))


def test_tolerance_sees_structural_faults():
    """Every fault of dbn_cases.FAULTS, applied to the fp64 run of the restatement, against the long-double run
    under tolerance(golden_d(case)), on every case (up to 16 sequences; J3072_S3072: one sequence, CHEAP_FAULTS).
    The table is profiles/dbn_fault_table.json; the conditions below are what it has to meet."""
    import json

    table = C.fault_table()
    cases = C.all_cases()
    assert set(table) == set(cases) and len(C.FAULTS) == 7
    for name, row in table.items():
        assert any(row.values()), f"{name} sees no fault: make it stronger"
        case = cases[name]
        if case["T"] >= 1 and C.has_free_interface(case):
            assert row["message_group"] and row["beta_index"], name
        assert ("clamped_parent_slice" in row) == C.has_clamped_prev_parent(case)
        if "clamped_parent_slice" in row:
            assert row["clamped_parent_slice"], name
    for fault in C.FAULTS:
        seen = [name for name, row in table.items() if row.get(fault)]
        assert len(seen) >= 3, (fault, seen)
    with open(C.FAULT_TABLE) as f:
        recorded = json.load(f)
    assert recorded["table"] == table and recorded["faults"] == C.FAULTS


def test_plan_interface_smaller_than_joint():
    # A_0 -> A_1 alone carries over; B hangs off A within the slice: S = 3 < J = 15
    p = _plan([3, 5], [0, 0], [([0], [3]), ([1, 0], [5, 3])], [([2, 0], [3, 3]), ([3, 2], [5, 3])])
    assert (p.info.n_configs, p.info.n_interface, p.info.n_prev_families, p.info.n_cur_families) == (15, 3, 1, 1)
    # a clamped interface node is a table offset, not part of the message
    p = _plan([3, 5], [1, 0], [([0], [3]), ([1, 0], [5, 3])], [([2, 0], [3, 3]), ([3, 2], [5, 3])])
    assert (p.info.n_configs, p.info.n_interface, p.info.n_prev_families) == (5, 1, 0)
    p = _plan([3, 5], [0, 0], [([0], [3]), ([1, 0], [5, 3])], [([2, 0], [3, 3]), ([3, 2], [5, 3])], queried=[0, 1])
    assert p.info.n_query == 5 and p.query_slices == {1: slice(0, 5)}


def test_plan_refusals():
    fam0, fam1 = _chain_families([2] * 13)
    with pytest.raises(ValueError, match="more than 4096 joint states"):
        _plan([2] * 13, [0] * 13, fam0, fam1)
    assert _plan([2] * 13, [1] + [0] * 12, fam0, fam1).info.n_configs == 4096
    fam0, fam1 = _chain_families([2] * 256)
    with pytest.raises(ValueError, match=r"256 slice nodes \(1 \.\. 255\)"):
        _plan([2] * 256, [1] * 256, fam0, fam1)
    fam0, fam1 = _chain_families([2, 3])
    with pytest.raises(ValueError, match="column 2 is out of range"):
        _plan([2, 3], [0, 0], [([0, 2], [2, 2]), ([1], [3])], fam1)
    with pytest.raises(ValueError, match="column 4 is out of range"):
        _plan([2, 3], [0, 0], fam0, [([2, 4], [2, 2]), ([3, 1], [3, 3])])
    with pytest.raises(ValueError, match="node column 1 is out of range"):
        _plan([2, 3], [0, 0], fam0, [([1, 0], [3, 2]), ([3, 1], [3, 3])])
    with pytest.raises(ValueError, match="its slice-t parent, column 1, has no slice-0 family"):
        _plan([2, 3], [0, 0], fam0[:1], fam1)
    with pytest.raises(ValueError, match="node 1 has no transition family"):
        _plan([2, 3], [0, 0], fam0, fam1[:1])
    with pytest.raises(ValueError, match="gives column 0 cardinality 3, node 0 has 2"):
        _plan([2, 3], [0, 0], fam0, [([2, 0], [2, 3]), ([3, 1], [3, 3])])
    with pytest.raises(ValueError, match="has two slice-0 families"):
        _plan([2, 3], [0, 0], [([0], [2]), ([0], [2])], fam1)
    with pytest.raises(ValueError, match="lists column 0 twice"):
        _plan([2, 3], [0, 0], fam0, [([2, 0, 0], [2, 2, 2]), ([3, 1], [3, 3])])
    with pytest.raises(ValueError, match="cardinality 0"):
        _plan([0, 3], [0, 0], fam0, fam1)


def test_raw_entry_points_refuse_bad_arguments():
    from pgmpy_amd import _native as N

    L = N.load_library()
    assert L.pgm_dbn_plan_create(None, None, None, 2, None, 0, None, 0, None) == N.PGM_EINVAL
    h = ctypes.c_void_p()
    assert L.pgm_dbn_plan_create(None, None, None, 2, None, 0, None, 0, ctypes.byref(h)) == N.PGM_EINVAL
    assert "null" in N.last_error() and not h.value
    assert L.pgm_dbn_info(None, None, None, None) == N.PGM_EINVAL
    assert L.pgm_dbn_plan_destroy(None) == N.PGM_OK
    fam0, fam1 = _chain_families([2, 3])
    p = _plan([2, 3], [0, 1], fam0, fam1)
    buf = np.zeros(4096, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 64

    def run(plan=p._h, codes=base, n_cols=6, ld=16, row0=0, n_rows=16, n_slices=3, v0=base, v1=base, filt=None, smooth=None,
            loglik=None, scratch=None, scratch_bytes=0):
        return L.pgm_dbn_run(plan, codes, n_cols, ld, row0, n_rows, n_slices, v0, v1, filt, smooth, loglik, None, scratch,
                             scratch_bytes, None)

    for kwargs, message in (
            (dict(plan=None), "null plan"), (dict(codes=None), "null codes"), (dict(v1=None), "null codes / values"),
            (dict(v0=base + 4), "not 8-byte aligned"), (dict(loglik=base + 2), "not 8-byte aligned"),
            (dict(row0=1), "outside ld"), (dict(n_rows=17), "outside ld"), (dict(row0=-1), "outside ld"),
            (dict(n_cols=5), "5 code columns"), (dict(n_slices=0, n_cols=0), "0 slices"),
            (dict(n_slices=65536, n_cols=131072), "65536 slices"),
            (dict(smooth=base), "bytes of scratch"), (dict(smooth=base, scratch=base, scratch_bytes=16 * 3 * 3 * 8 - 8), "bytes of scratch")):
        assert run(**kwargs) == N.PGM_EINVAL, kwargs
        assert message in N.last_error(), (kwargs, N.last_error())
    # an empty window is fine and launches nothing: no device is needed for it
    assert run(n_rows=0) == N.PGM_OK and run(n_rows=0, row0=16) == N.PGM_OK


def test_compute_needs_a_device(monkeypatch):
    import torch

    from pgmpy_amd import _native as N
    from pgmpy_amd._native import NativeUnavailable
    from pgmpy_amd.inference import DBNInference

    N.load_library()
    monkeypatch.setattr(N, "_device_ok", False)  # as on a machine without a device, wherever this runs
    m = C.to_model(C.doc_spec())
    inf = DBNInference(m)
    codes = torch.zeros((6, 4), dtype=torch.uint8)
    df = pd.DataFrame({("Y", 0): [0, 1], ("Y", 1): [1, np.nan]})
    for call in (lambda: inf.query([("Z", 0)], {("Y", 0): 0}), lambda: inf.forward_inference([("Z", 1)], {("Y", 0): 0}),
                 lambda: inf.backward_inference([("Z", 0)]), lambda: inf.filter_batch(df), lambda: inf.smooth_batch(df),
                 lambda: inf.log_likelihood_batch(df), lambda: inf.filter_codes(codes, observed=["X", "Y"]),
                 lambda: inf.smooth_codes(codes), lambda: inf.log_likelihood_codes(codes),
                 lambda: m.simulate(n_samples=4, n_time_slices=3, seed=1), lambda: m.simulate_codes(4, 3, seed=1),
                 lambda: m.fit(pd.DataFrame({(v, t): [0, 1, 1] for t in range(2) for v in "XYZ"}))):
        with pytest.raises(NativeUnavailable):
            call()
    codes, observed = inf.encode(df)
    assert codes.shape == (6, 2) and observed == [] and codes[1, 0] == 0 and codes[4, 1] == C.MISSING and codes[0, 0] == C.MISSING
    with pytest.raises(NotImplementedError):
        inf.forward_inference([("Z", 0)], args="potential")
