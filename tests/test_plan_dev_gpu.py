"""The device side of the three plan handles (pgmpy_amd/csrc/pgm_plan_dev.h behind FitPlan, SamplePlan and
GibbsPlan) and their flagged launches on the device: the flag word is this call's and no call's after it,
the lazy stages of a FitPlan come in any order, a destroyed plan leaves nothing behind, and a plan follows
the current device.  tests/test_plan_dev_cpu.py exercises the bookkeeping itself with stubbed operations.

The model is two families, P(c0) and P(c1 | c0), with cardinalities 2 and 3 (as Gibbs factors the same
two); the code matrix is a 5-row window at row0 = 3 of ld = 16 rows.  Expectations are the restatements
of tests/fit_cases.py, sample_cases.py, gibbs_cases.py, score_cases.py, ci_cases.py and em_cases.py, with
their bounds."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ci_cases as CI
from tests import em_cases as EM
from tests import fit_cases as F
from tests import gibbs_cases as G
from tests import sample_cases as S
from tests import score_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMS = [([0], [2]), ([1, 0], [3, 2])]
CARD = [2, 3]
# a CI test needs X and Y: the stage-order test reads the pair both ways instead of P(c0)
PAIRS = [([0, 1], [2, 3]), ([1, 0], [3, 2])]
TABLES = [np.array([0.3, 0.7]), np.array([[0.2, 0.5], [0.3, 0.25], [0.5, 0.25]])]
VALUES = np.concatenate([t.ravel() for t in TABLES])
LD, ROW0, N = 16, 3, 5
WINDOW = np.array([[0, 1, 1, 0, 1], [2, 0, 1, 1, 2]], dtype=np.uint8)
OUTSIDE = 200  # not a state: a launch that read outside the window would raise
SEED, FIRST = 5, 7


def _codes(bad_col=None):
    """The code matrix; bad_col: that column's code of the window's middle row is its cardinality."""
    buf = np.full((2, LD), OUTSIDE, dtype=np.uint8)
    buf[:, ROW0:ROW0 + N] = WINDOW
    if bad_col is not None:
        buf[bad_col, ROW0 + 2] = CARD[bad_col]
    return buf


def _dev(a):
    from pgmpy_amd import engine as E

    return E.to_device_raw(np.ascontiguousarray(a))


def _host(t):
    from pgmpy_amd.inference.batch import download

    return download(t)


def _fit(families=FAMS):
    from pgmpy_amd.estimators._fit import FitPlan

    return FitPlan(families)


def _sample():
    from pgmpy_amd.sampling._sample import SamplePlan

    return SamplePlan(FAMS)


def _gibbs():
    from pgmpy_amd.sampling._gibbs import GibbsPlan

    return GibbsPlan(FAMS, CARD)


# ---------------------------------------------------------------------------- one clean call of each kind
# Each returns what the call produced on the host and asserts that it is the restatement's.
@functools.lru_cache(maxsize=None)
def _estep_ref():
    return EM.estep_ref(FAMS, [0], VALUES, WINDOW)


def _count(plan):
    got = _host(plan.count(_dev(_codes()), n_rows=N, row0=ROW0))
    assert got.dtype == np.int64 and np.array_equal(got, F.count_ref(_codes(), FAMS, ROW0, N))
    return got


def _estep(plan):
    tables, loglik = plan.estep([0], _dev(VALUES), _dev(_codes()), n_rows=N, row0=ROW0, want_loglik=True)
    got, ll = _host(tables), _host(loglik)
    want, want_ll, counted, _ = _estep_ref()
    want = np.asarray(want, dtype=np.float64)
    assert counted.all()
    # both families have the latent c0 in scope, L = 2 (em_cases.bound / bound_loglik, as tests/test_em_gpu.py)
    assert np.all(np.abs(got - want) <= EM.bound(N, 2, 2, want))
    want_ll = np.asarray(want_ll, dtype=np.float64)
    assert np.all(np.abs(ll[ROW0:ROW0 + N] - want_ll) <= EM.bound_loglik(2, 2, want_ll))
    assert np.all(ll[:ROW0] == 0.0) and np.all(ll[ROW0 + N:] == 0.0)
    return got


def _cdf(plan):
    got = _host(plan.cdf(_dev(VALUES)))
    assert np.array_equal(got, np.concatenate([S.running_sums(t.reshape(t.shape[0], -1)).ravel() for t in TABLES]))
    return got


def _forward(plan):
    """c0 is GIVEN (the window's codes), c1 is drawn."""
    modes = [S.GIVEN, S.FREE]
    codes = _dev(_codes())
    plan.forward(plan.cdf(_dev(VALUES)), codes, n_rows=N, row0=ROW0, first_row=FIRST, seed=SEED, modes=modes)
    got = _host(codes)
    want, _, bad = S.sample_ref(FAMS, TABLES, N, seed=SEED, first_row=FIRST, given=WINDOW, modes=modes)
    assert not bad and np.array_equal(got[:, ROW0:ROW0 + N], want)
    assert np.array_equal(got[0], _codes()[0]) and (got[1, :ROW0] == OUTSIDE).all() and (got[1, ROW0 + N:] == OUTSIDE).all()
    return got


def _sweep(plan):
    codes = _dev(_codes())
    plan.sweep(_dev(VALUES), codes, 3, n_chains=N, row0=ROW0, first_chain=FIRST, seed=SEED)
    got = _host(codes)
    want, _, undrawn, bad = G.gibbs_ref(FAMS, TABLES, CARD, WINDOW, 3, seed=SEED, first_chain=FIRST)
    assert not undrawn and not bad and np.array_equal(got[:, ROW0:ROW0 + N], want)
    assert (got[:, :ROW0] == OUTSIDE).all() and (got[:, ROW0 + N:] == OUTSIDE).all()
    return got


def _bad_count(plan):
    plan.count(_dev(_codes(bad_col=0)), n_rows=N, row0=ROW0)


def _bad_estep(plan):  # c0 is latent and never read: the bad code is c1's
    plan.estep([0], _dev(VALUES), _dev(_codes(bad_col=1)), n_rows=N, row0=ROW0)


def _bad_cdf(plan):  # the column of P(c1 | c0 = 0) is all zero
    values = VALUES.copy()
    values[2::2] = 0.0
    plan.cdf(_dev(values))


def _bad_forward(plan):  # the given c0
    plan.forward(plan.cdf(_dev(VALUES)), _dev(_codes(bad_col=0)), n_rows=N, row0=ROW0, first_row=FIRST, seed=SEED,
                 modes=[S.GIVEN, S.FREE])


def _bad_sweep(plan):
    plan.sweep(_dev(VALUES), _dev(_codes(bad_col=1)), 3, n_chains=N, row0=ROW0, first_chain=FIRST, seed=SEED)


FLAGGED = {
    "count": (_fit, _bad_count, _count, IndexError, "fit_count: a state code is >= its variable's cardinality"),
    "estep": (_fit, _bad_estep, _estep, IndexError, "fit_estep: a state code is >= its variable's cardinality"),
    "cdf": (_sample, _bad_cdf, _cdf, ValueError, "sample_cdf: a CPD column's total is not finite or not > 0"),
    "forward": (_sample, _bad_forward, _forward, IndexError,
                "sample_forward: a given state code is >= its variable's cardinality"),
    "sweep": (_gibbs, _bad_sweep, _sweep, IndexError, "gibbs_sweep: a state code is >= its variable's cardinality"),
}


# ---------------------------------------------------------------------------- the flag is per call
@pytest.mark.parametrize("name", list(FLAGGED))
def test_a_raised_flag_is_that_call_s_alone(gpu, name):
    """A call with one bad input raises what it raises today; the next call on the same plan with clean
    input succeeds and equals the restatement (exactly, or within the restatement's bound for the E-step);
    so does a clean call before the bad one."""
    make, bad, clean, error, message = FLAGGED[name]
    plan = make()
    first = clean(plan)
    with pytest.raises(error, match=message):
        bad(plan)
    after = clean(plan)
    if name != "estep":  # fp64 atomics in no fixed order: within the bound, checked by _estep
        assert first.tobytes() == after.tobytes()
    fresh = make()
    with pytest.raises(error, match=message):
        bad(fresh)
    clean(fresh)


# ---------------------------------------------------------------------------- the stages in any order
def _score(plan, counts):
    alpha, beta = SC.kernel_params(plan.families)
    got = _host(plan.score(counts, SC.BD, _dev(alpha), _dev(beta)))
    want, mag, n, _ = SC.score_ref(_host(counts), plan.families, SC.BD, alpha, beta)
    assert (np.abs(got.astype(SC.LD) - want).astype(np.float64) <= SC.bound(n, mag, SC.U_DEVICE)).all()
    return got


def _citest(plan, counts):
    stat, dof, p = (_host(t) for t in plan.citest(counts, 1.0, yates=True))
    for f, table in enumerate(CI.tables_of(WINDOW, plan.families)):
        s, d, pv, mag, cells = CI.ci_ref(table, 1.0, True, False)
        b = CI.bound(cells, mag)
        assert int(dof[f]) == d and CI.same(stat[f], s, b) and CI.same(p[f], pv, CI.p_bound(s, d, pv, b)), f
    return stat, dof, p


def _pair_count(plan):
    got = _host(plan.count(_dev(_codes()), n_rows=N, row0=ROW0))
    assert np.array_equal(got, F.count_ref(_codes(), PAIRS, ROW0, N))
    return got


def test_the_stages_of_a_fit_plan_come_in_any_order(gpu):
    """citest before score before count on one plan, the reverse on a second: identical outputs, each the
    restatement's.  (Over PAIRS: pgm_fit_citest refuses a plan with a one-variable family on the host.)"""
    counts = _dev(F.count_ref(_codes(), PAIRS, ROW0, N))
    a, b = _fit(PAIRS), _fit(PAIRS)
    ci_a = _citest(a, counts)
    score_a = _score(a, counts)
    count_a = _pair_count(a)
    count_b = _pair_count(b)
    score_b = _score(b, counts)
    ci_b = _citest(b, counts)
    assert count_a.tobytes() == count_b.tobytes() and score_a.tobytes() == score_b.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ci_a, ci_b))
    # and again on the first plan, every stage now built
    assert _score(a, counts).tobytes() == score_a.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(_citest(a, counts), ci_a))


def test_a_refused_citest_leaves_the_plan_usable(gpu):
    """The two-family model itself: its first family has no Y, the CI stage is never built, and score and
    count before and after the refusal are the restatement's."""
    plan = _fit()
    counts = _dev(F.count_ref(_codes(), FAMS, ROW0, N))
    with pytest.raises(ValueError, match="fit_citest: family 0 has fewer than two variables"):
        plan.citest(counts, 1.0)
    first = _score(plan, counts)
    with pytest.raises(ValueError, match="fit_citest: family 0 has fewer than two variables"):
        plan.citest(counts, 1.0)
    assert _score(plan, counts).tobytes() == first.tobytes()
    _count(plan)


def test_destroyed_plans_leave_nothing_behind(gpu):
    """A plan destroyed before any launch and one destroyed after only a score leave torch.cuda's memory
    as it was, and the process exits cleanly (tests/workers/plan_dev_destroy.py)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "workers", "plan_dev_destroy.py")], cwd=ROOT,
                       timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["after"] == out["before"], out
    assert len(out["scores"]) == 2 and all(np.isfinite(out["scores"])), out


# ---------------------------------------------------------------------------- a plan follows the device
def test_a_plan_follows_the_current_device(gpu):
    """The same FitPlan, SamplePlan and GibbsPlan on device 0, then 1, then 0 again: every result is the
    restatement's (asserted by the helpers) and the three equal each other."""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices: a plan's move between devices cannot be shown on one")
    fit, pairs, sample, gibbs = _fit(), _fit(PAIRS), _sample(), _gibbs()
    runs = []
    for d in (0, 1, 0):
        with torch.cuda.device(d):
            counts = _dev(F.count_ref(_codes(), PAIRS, ROW0, N))
            runs.append([_count(fit), _score(pairs, counts), *_citest(pairs, counts), _pair_count(pairs), _cdf(sample),
                         _forward(sample), _sweep(gibbs)])
            _estep(fit)
            torch.cuda.synchronize()
    for other in runs[1:]:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(runs[0], other))
