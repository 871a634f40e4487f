"""The particle filter on the device (pgmpy_amd/csrc/pgmdbn_pf.hip) against its restatement (tests/dbn_pf_cases.py):
filter, ess, ancestors, trajectories and traced samples bit for bit, the log-likelihood within the device's log."""
import numpy as np
import pytest

from tests import dbn_cases as C
from tests import dbn_pf_cases as PF

pytestmark = pytest.mark.gpu
LOG_TOL = 4e-13  # per log term (tests/lw_cases.tolerance); a slice adds two


def _inference(spec):
    from pgmpy_amd.inference import DBNInference

    return DBNInference(C.to_model(spec))


def _host(t):
    from pgmpy_amd.inference.batch import download

    return download(t.contiguous())


def _run(inf, codes, N, seed, first_row=0, variables=None, **kw):
    """dict of host arrays from plan.run + plan.trace: filter, loglik, ess, flag, anc (uint16), traj, samples."""
    from pgmpy_amd import engine as E

    plan = inf.pf_plan(variables)
    filt, ll, ess, flags, anc, traj = plan.run(E.to_device_raw(np.ascontiguousarray(codes)), *inf._tables(), N, seed,
                                               first_row=first_row, want_traj=True, **kw)
    rows = anc.shape[0]
    samples = _host(plan.trace(anc, traj)).reshape(-1, rows, N)
    return {"filter": _host(filt), "loglik": _host(ll), "ess": _host(ess), "flag": _host(flags),
            "anc": _host(anc.view(flags.dtype)).view(np.uint16), "traj": _host(traj), "samples": samples}


def _assert_equal(got, b, want, T):
    for key in ("filter", "ess", "anc", "traj"):
        assert np.array_equal(got[key][b], want[key], equal_nan=key in ("filter", "ess")), key
    assert np.array_equal(got["samples"][:, b], PF.trace(want["anc"], want["traj"]))
    assert got["flag"][b] == want["flag"]
    if np.isfinite(want["loglik"]):
        assert abs(got["loglik"][b] - want["loglik"]) <= LOG_TOL * 2 * T
    else:
        assert np.array_equal(got["loglik"][b], want["loglik"], equal_nan=True)


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("N", [64, 256, 1024])
@pytest.mark.parametrize("name", list(PF.specs()))
def test_device_equals_restatement(name, N, T):
    spec, ev = PF.specs()[name], PF.evidence(name, T)
    got = _run(_inference(spec), C.to_codes(ev), N, seed=7)
    for b in range(len(ev)):
        _assert_equal(got, b, PF.run(spec, ev[b], N, 7, first_row=b * N), T)


def test_placement_independence():
    """Sequence 1 of a batch of three, alone with first_row shifted, and in a row window between 0xAB pad rows."""
    spec, ev, N, T = PF.specs()["two_iface"], PF.evidence("two_iface", 5), 256, 5
    inf = _inference(spec)
    batch = _run(inf, C.to_codes(ev), N, seed=7)
    alone = _run(inf, C.to_codes(ev[1:2]), N, seed=7, first_row=N)
    padded = np.full((T * 4, 5), 0xAB, dtype=np.uint8)
    padded[:, 2] = C.to_codes(ev[1:2])[:, 0]
    window = _run(inf, padded, N, seed=7, first_row=N, row0=2, n_rows=1)
    for key in batch:
        ours = batch[key][:, 1] if key == "samples" else batch[key][1]
        for other in (alone, window):
            assert np.array_equal(ours, other[key][:, 0] if key == "samples" else other[key][0]), key


def test_special_sequences():
    """No evidence: the forward sampler's rows.  An impossible sequence, a bad code: their own outputs alone."""
    N, T = 256, 3
    spec = C.make_spec(seed=80, deterministic=("X",), **C.DOC)
    model = C.to_model(spec)
    inf = _inference(spec)
    free = np.full((T * 3, 2), 255, dtype=np.uint8)
    from pgmpy_amd import engine as E

    samples = inf.posterior_sample_codes(E.to_device_raw(free), N, seed=5)
    assert np.array_equal(_host(samples), _host(model.simulate_codes(2 * N, T, seed=5)))

    ev = np.full((3, T, 3), 255, dtype=np.uint8)
    ev[0, :, 1] = 1                                             # an ordinary sequence
    ev[1, 1, 2], ev[1, 1, 0] = 0, int(spec["fam1"][0][1][:, 0].argmin())  # X_1 at the state P(X | Z = 0) gives 0
    ev[2, 2, 1] = 7                                             # no state of Y
    with pytest.raises(IndexError, match="cardinality"):
        _run(inf, C.to_codes(ev), N, seed=9)
    got = _run(inf, C.to_codes(ev), N, seed=9, strict=False)
    for b in range(3):
        _assert_equal(got, b, PF.run(spec, ev[b], N, 9, first_row=b * N), T)
    assert list(got["flag"]) == [0, PF.IMPOSSIBLE, PF.BAD] and got["loglik"][1] == -np.inf
    assert np.isfinite(got["filter"][1, 0]).all() and np.isnan(got["filter"][1, 1:]).all() and np.isnan(got["filter"][2]).all()
    values0, values1 = inf._tables()
    with pytest.raises(ValueError, match="total is not finite or not > 0"):  # a CPD column that cannot be drawn from
        inf.pf_plan().run(E.to_device_raw(free), values0 * 0, values1, N, 9)


def test_thirteen_chains_past_the_exact_filter():
    k, N, T = 13, 1024, 4
    spec = PF.chain_spec(k)
    hidden = spec["names"][:k]
    ev = C.sample(spec, T - 1, 1, seed=230)[0]
    ev[:, :k] = 255
    inf = _inference(spec)
    from pgmpy_amd import engine as E

    codes = E.to_device_raw(C.to_codes(ev[None]))
    with pytest.raises(ValueError, match="more than 4096 joint states"):
        inf.filter_codes(codes, observed=spec["names"][k:], variables=hidden)
    filt, ll, ess, flags = (_host(t) for t in inf.particle_filter_codes(codes, N, seed=11, variables=hidden))
    want = PF.run(spec, ev, N, 11, queried=set(hidden))
    assert np.array_equal(filt[0], want["filter"]) and np.array_equal(ess[0], want["ess"]) and flags[0] == 0
    assert abs(ll[0] - want["loglik"]) <= LOG_TOL * 2 * T
    for i in range(k):
        exact = np.asarray(C.recursion(PF.one_chain(spec, i, k), [], ev[:, [i, k + i]])[0], dtype=np.float64)[:, :2]
        assert np.all(np.abs(filt[0][:, 2 * i:2 * i + 2] - exact) <= PF.margin(exact, ess[0][:, None])), i


CHAINS = PF.chain_spec(13)
QUERIES = {  # spec, evidence, variables, (filters, particles) that serve n_samples = 5000
    "docstring": (C.doc_spec(), {("Y", 0): 0, ("Y", 1): 1, ("X", 2): 0}, [("Z", 2), ("X", 1)], (2, 4096)),
    # 26 nodes, 13 of them interface: 4,096 particles do not fit, and 2,048 take more than 64 KiB of dynamic LDS
    "thirteen_chains": (CHAINS, {(f"O{i:02d}", t): (i + t) % 2 for i in range(13) for t in range(2)},
                        [("H12", 1), ("H00", 0)], (3, 2048)),
}


@pytest.mark.parametrize("case", list(QUERIES))
def test_approx_inference_query(case):
    """n_samples = 5000: filters on consecutive stream rows, pooled by their evidence estimates, against the
    restatement pooled the same way."""
    from pgmpy_amd.inference import ApproxInference

    spec, evidence, variables, filters = QUERIES[case]
    infer = ApproxInference(C.to_model(spec))
    queried = sorted({name for name, _ in variables}, key=spec["names"].index)
    plan = infer._dbn.pf_plan(queried)
    R, P = infer.dbn_filters(5000, plan.max_particles)
    assert (R, P) == filters and (plan.info_at(P).lds_bytes > 65536) == (case == "thirteen_chains")
    T = 1 + max(t for _, t in list(variables) + list(evidence))
    runs = [PF.run(spec, C.evidence_array(spec, evidence, T - 1), P, 13, first_row=r * P, queried=set(queried)) for r in range(R)]
    weight = np.exp(np.array([r["loglik"] for r in runs]) - max(r["loglik"] for r in runs))
    want = np.zeros((2, 2))
    for r, w in zip(runs, weight):
        rows = PF.trace(r["anc"], r["traj"])  # queried node k of slice t at row t queried + k
        np.add.at(want, tuple(rows[t * len(queried) + queried.index(name)] for name, t in variables), w / (P * weight.sum()))
    got = infer.query(variables, n_samples=5000, evidence=evidence, seed=13)
    assert got.variables == variables
    np.testing.assert_allclose(got.values, want, rtol=1e-10, atol=0)
    assert infer.map_query(variables, n_samples=5000, evidence=evidence, seed=13) == \
        dict(zip(variables, np.unravel_index(int(want.argmax()), want.shape)))


def test_get_distribution_counts_a_frame_of_sequences():
    from pgmpy_amd.inference import ApproxInference

    model = C.to_model(C.doc_spec())
    frame = model.simulate(n_samples=300, n_time_slices=2, seed=3)
    want = np.zeros((2, 2))
    np.add.at(want, (frame[("Z", 1)].to_numpy(dtype=int), frame[("X", 0)].to_numpy(dtype=int)), 1)
    got = ApproxInference(model).get_distribution(frame, [("Z", 1), ("X", 0)])
    assert got.variables == [("Z", 1), ("X", 0)] and np.array_equal(got.values, want / 300)
    assert np.array_equal(ApproxInference(model).query([("X", 0)], samples=frame, joint=False)[("X", 0)].values, want.sum(axis=0) / 300)
