"""The particle filter's restatement against the exact filter, its resampling rule, and the host side of the
pgm_dbn_pf_* entry points (no device: every check below runs before any HIP call)."""
import ctypes

import numpy as np
import pytest

from tests import dbn_cases as C
from tests import dbn_pf_cases as PF

FAKE = ctypes.c_void_p(4096)  # a non-null, aligned pointer that no host check dereferences


@pytest.mark.parametrize("name", list(PF.specs()))
def test_restatement_within_margin_of_exact_filter(name):
    spec, worst = PF.specs()[name], 0.0
    for b, ev in enumerate(PF.evidence(name, 5)):
        got = PF.reference(name, 5, 4096, b=b)
        exact = np.asarray(C.recursion(spec, [], ev)[0], dtype=np.float64)
        ratio = np.abs(got["filter"] - exact) / PF.margin(exact, got["ess"][:, None])
        worst = max(worst, float(ratio.max()))
        assert got["flag"] == 0 and np.isfinite(got["loglik"])
    print(f"{name}: largest |error| / margin = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", list(PF.specs()))
def test_resampling_identity_and_monotone(name):
    spec = PF.specs()[name]
    free = PF.run(spec, np.full((3, len(spec["card"])), 255, dtype=np.uint8), 256, seed=3)
    assert np.array_equal(free["anc"], np.tile(np.arange(256, dtype=np.uint16), (3, 1)))
    assert np.all(free["ess"] == 256.0) and free["loglik"] == 0.0
    anc = PF.reference(name, 5, 4096)["anc"].astype(np.int64)
    assert np.all(np.diff(anc, axis=1) >= 0) and anc.max() < 4096


def _plan(spec, queried=None):
    from pgmpy_amd.inference._dbn_pf import DbnPfPlan

    n = len(spec["card"])
    fams = [[(list(cols), [spec["card"][c % n] for c in cols]) for cols, _ in spec[k]] for k in ("fam0", "fam1")]
    return DbnPfPlan(spec["card"], [True] * n if queried is None else queried, fams[0], fams[1])


def test_bindings_and_plan():
    from pgmpy_amd import _native as N

    lib = N.load_library()
    for name in ("pgm_dbn_pf_plan_create", "pgm_dbn_pf_plan_destroy", "pgm_dbn_pf_plan_info", "pgm_dbn_pf_run", "pgm_dbn_pf_trace"):
        assert name in N.EXPORTED and getattr(lib, name).argtypes is not None
    assert lib.pgm_version() == 25
    spec = PF.specs()["two_iface"]
    plan = _plan(spec, [True, False, True, True])
    assert plan.order0 == PF.plan_order(4, spec["fam0"], 0) == [0, 3, 1, 2]
    assert plan.order1 == PF.plan_order(4, spec["fam1"], 4)
    assert (plan.info.n, plan.info.n_interface, plan.n_query_nodes, plan.n_query) == (4, 2, 3, 6)
    for n_particles, block in ((64, 64), (128, 128), (1024, 256), (4096, 256)):
        info = plan.info_at(n_particles)
        # the code tile, w / q / scan, the histogram, the pad, the evidence bytes
        assert info.lds_bytes == (4 + 2) * n_particles + 8 * n_particles + 8 * 6 + 128 + 8
        assert (info.block, info.max_particles) == (block, 4096)


def _create(card, f0, f1, queried=None, patch=None, **over):
    """(status, message) of pgm_dbn_pf_plan_create; `over` replaces an argument (c_card, c_fam0, n, n0, n1) by name."""
    from pgmpy_amd import _native as N
    from pgmpy_amd._plan import family_array

    a0, a1 = family_array(f0)[1], family_array(f1)[1]
    if patch:
        patch(a0)
    n = len(card)
    arg = dict(c_card=(ctypes.c_int32 * max(n, 1))(*card), c_fam0=a0, n=n, n0=len(f0), n1=len(f1))
    arg.update(over)
    h = ctypes.c_void_p()
    lib = N.load_library()
    rc = lib.pgm_dbn_pf_plan_create(arg["c_card"], (ctypes.c_uint8 * max(n, 1))(*(queried or [0] * n)), arg["n"], arg["c_fam0"],
                                    arg["n0"], a1, arg["n1"], ctypes.byref(h))
    lib.pgm_dbn_pf_plan_destroy(h)
    return rc, N.last_error()


def test_host_argument_checks():
    from pgmpy_amd import _native as N

    lib = N.load_library()
    plan = _plan(PF.specs()["doc"])
    fam0 = [([0, 2], [2, 2]), ([1, 0], [2, 2]), ([2], [2])]
    fam1 = [([3, 5], [2, 2]), ([4, 3], [2, 2]), ([5, 2], [2, 2])]
    wide0, wide1 = [([v], [254]) for v in range(255)], [([255 + v], [254]) for v in range(255)]
    ring = [([v, (v + 1) % 255, (v + 2) % 255], [254] * 3) for v in range(255)]
    for card, f0, f1, kw, msg in (
            ([2, 2, 255], fam0, fam1, {}, "cardinality 255"), ([2, 2, 2], fam0[:2], fam1, {}, "has no slice-0 family"),
            ([2, 2, 2], fam0, fam1[:2] + [([5, 6], [2, 2])], {}, "out of range"),
            ([2, 2, 2], fam0, [([3, 4], [2, 2]), ([4, 3], [2, 2]), fam1[2]], {}, "cycle"),
            ([2, 2, 3], fam0, fam1, {}, "cardinality 2, node 2 has 3"),
            ([2, 2, 2], fam0, fam1, dict(n=0), "0 slice nodes"), ([2, 2, 2], fam0, fam1, dict(n=256), "256 slice nodes"),
            ([2, 2, 2], fam0, fam1, dict(c_card=None), "null card"), ([2, 2, 2], fam0, fam1, dict(c_fam0=None), "null families"),
            ([2, 2, 2], fam0, fam1, dict(n1=-1), "3 / -1 families"), ([2, 2, 2], fam0, fam1, dict(patch=lambda a: setattr(a[0], "n_vars", 0)), "has 0 variables"),
            ([2, 2, 2], [([0, 2, 2], [2, 2, 2])] + fam0[1:], fam1, {}, "lists column 2 twice"),
            ([2, 2, 2], fam0 + [([2, 0], [2, 2])], fam1, {}, "node 2 has two slice-0 families"),
            ([254] * 255, [([0, 1, 2, 3], [254] * 4)] + wide0[1:], wide1, {}, "family 0 has 2^31 table entries"),
            ([254] * 255, ring, wide1, {}, "the slice-0 tables have 2^31 entries"),
            ([254] * 255, wide0, wide1, dict(queried=[1] * 255), "bytes of LDS for 64 particles")):
        rc, said = _create(card, f0, f1, **kw)
        assert rc == N.PGM_EINVAL and msg in said, (msg, said)
    assert _create([2, 2, 2], fam0, fam1)[0] == N.PGM_OK
    for n_particles in (0, 32, 100, 8192):
        with pytest.raises(ValueError, match="a power of two, 64 .. 4096"):
            plan.info_at(n_particles)
    assert lib.pgm_dbn_pf_plan_info(None, 64, None, None, None, None, None) == N.PGM_EINVAL and "null plan" in N.last_error()

    def run(h=plan._h, codes=FAKE, n_cols=6, ld=4, row0=0, n_rows=4, T=2, v0=FAKE, v1=FAKE, P=64, first=0, filt=FAKE,
            anc=None, traj=None):
        return lib.pgm_dbn_pf_run(h, codes, n_cols, ld, row0, n_rows, T, v0, v1, P, first, 1, filt, None, None, None, anc, traj, None)

    odd8, odd2 = ctypes.c_void_p(4100), ctypes.c_void_p(4097)
    for kwargs, msg in ((dict(h=None), "null plan"), (dict(codes=None), "null codes"), (dict(v1=None), "null codes / values"),
                        (dict(T=0, n_cols=0), "0 slices"), (dict(T=65536, n_cols=3 * 65536), "65536 slices"),
                        (dict(n_cols=5), "5 code columns"), (dict(row0=1), "outside ld"), (dict(n_rows=-1), "outside ld"),
                        (dict(P=96), "a power of two"), (dict(first=-1), "first_row"), (dict(filt=odd8), "8-byte aligned"),
                        (dict(v0=odd8), "8-byte aligned"), (dict(anc=odd2), "2-byte aligned"), (dict(traj=FAKE), "traj without ancestors"),
                        (dict(ld=2 ** 31, n_rows=2 ** 31), "2147483648 sequences in one call")):
        assert run(**kwargs) == N.PGM_EINVAL and msg in N.last_error(), (kwargs, N.last_error())
    assert run(n_rows=0) == N.PGM_OK

    def trace(h=plan._h, anc=FAKE, traj=FAKE, rows=2, T=2, P=64, out=FAKE, ld_out=128, row0_out=0):
        return lib.pgm_dbn_pf_trace(h, anc, traj, rows, T, P, out, ld_out, row0_out, None)

    for kwargs, msg in ((dict(h=None), "null plan"), (dict(anc=None), "null ancestors"), (dict(out=None), "null ancestors / traj / out"),
                        (dict(anc=odd2), "2-byte aligned"), (dict(T=0), "0 slices"), (dict(P=65), "a power of two"),
                        (dict(rows=2 ** 31 // 16), "134217728 sequences"), (dict(ld_out=127), "outside ld_out"),
                        (dict(row0_out=1), "outside ld_out")):
        assert trace(**kwargs) == N.PGM_EINVAL and msg in N.last_error(), (kwargs, N.last_error())
    assert trace(rows=0) == N.PGM_OK


def test_particles_past_the_lds_budget_name_the_largest_that_fits():
    """60 nodes, all in the interface: 120 N + 8 N bytes of tile and scan pass the budget at N = 2048."""
    from pgmpy_amd import _native as N

    names = [f"N{i:02d}" for i in range(60)]
    plan = _plan(C.make_spec(names=names, card=[2] * 60, intra=[], inter=[(v, v) for v in names], seed=1), [False] * 60)
    assert plan.max_particles == 1024 and plan.info_at(1024).lds_bytes == 128 * 1024 + 128 + 64 <= N.DBN_PF_LDS_MAX
    assert plan.info_at(2048).lds_bytes > N.DBN_PF_LDS_MAX  # the query itself answers; the run refuses
    rc = N.load_library().pgm_dbn_pf_run(plan._h, FAKE, 60, 1, 0, 1, 1, FAKE, FAKE, 2048, 0, 1, None, None, None, None, None,
                                         None, None)
    assert rc == N.PGM_EINVAL and "the largest that fits is 1024" in N.last_error()


def test_approx_inference_takes_a_dynamic_network_without_a_device():
    from pgmpy_amd.factors.discrete import TabularCPD
    from pgmpy_amd.inference import ApproxInference

    infer = ApproxInference(C.to_model(C.doc_spec()))
    assert [infer.dbn_filters(*a) for a in ((10,), (5000,), (10000, 2048))] == [(1, 64), (2, 4096), (5, 2048)]
    with pytest.raises(NotImplementedError, match="virtual_evidence"):
        infer.query([("Z", 1)], virtual_evidence=[TabularCPD(("X", 0), 2, [[0.5], [0.5]])])
    with pytest.raises(ValueError, match="not in the model"):
        infer.query([("Q", 1)])
