"""Every branch of the batched calibration schedule (bp_batch.BPSchedule) on the small trees of
tests/bp_cases.py: which branch ran is read from BPSchedule.trace and asserted, how each recorded step runs
from the program's records, and every entry of every clique belief, sepset belief and marginal of every row
is compared with the long-double closed form under the bound derived in bp_cases (exact zeros, NaN marginals
of the impossible rows).  Row counts: 3 (level-batch jobs only), 65 (past one wave, still odd: the fused
kernel declines every pass), 66 (the smallest shapes the fused kernel takes: clique-sized steps reach
program.PM_PREFER_MIN, separator-sized ones do not) and 1030 (separator-sized steps reach it too).

Measured on an MI355X, worst |got - ref| / bound over all row counts, sum / max: single 0.046 / 0.046, chain3
0.067 / 0.046, chain3_noev 0.059 / 0.083, chain3_sepev 0.061 / 0.090, chain_swapped 0.051 / 0.046, twins 0.051 /
0.051, nested 0.047 / 0.057, nested_single 0.047 / 0.056, star7_ratio 0.022 / 0.054, star7_sigma 0.016 / 0.053,
star6 0.029 / 0.083, fan20 0.020 / 0.024, deep 0.035 / 0.051, pairs 0.045 / 0.054: the bound counts the worst
case of every rounding in every clique's passes, the errors met are a few roundings."""
import numpy as np
import pytest

from tests import bp_cases as BC

pytestmark = pytest.mark.gpu

NAMES = list(BC.TREES)
OPS = {"marginalize": "sum", "maximize": "max"}
SWEEP_ROWS = (3, 65, 1030)


def _junction_tree(tree):
    from pgmpy_amd.factors.discrete import DiscreteFactor
    from pgmpy_amd.models import JunctionTree

    jt = JunctionTree()
    jt.add_nodes_from(tree["cliques"])
    jt.add_edges_from(tree["edges"])
    jt.add_factors(*[DiscreteFactor(list(c), [tree["card"][v] for v in c], tree["pots"][c]) for c in tree["cliques"]])
    assert jt.check_model()
    return jt


def _bjt(tree):
    from pgmpy_amd.inference.bp_batch import BatchedJunctionTree

    bjt = BatchedJunctionTree(_junction_tree(tree))
    assert bjt.root == tree["cliques"][0] and bjt.order == BC.rooted(tree)[0]
    assert all(bjt.var_clique[v] == BC.first_clique(tree, v) for v in tree["variables"])
    return bjt


def _upload(codes):
    import torch

    return torch.as_tensor(np.ascontiguousarray(codes)).cuda()


def classify(prog):
    """One of specialised / generic_fused / level_job / own_launch per recorded step of a levelled program:
    a bound plan-specialised kernel (merged with its level's others), the generic fused product + marginal
    kernel, a job of its level's batch launch, or a launch of its own (a job alone in its level included)."""
    prog._lower()
    jobs = {}
    for r in prog._recs:
        if r.job is not None:
            jobs[r.level] = jobs.get(r.level, 0) + 1
    out = []
    for r in prog._recs:
        if r.pm is not None:
            assert r.job is None
            out.append("specialised")
        elif r.job is not None:
            out.append("level_job" if jobs[r.level] >= 2 else "own_launch")
        elif r.note.startswith("product_n_marginal"):
            out.append("generic_fused")
        else:
            out.append("own_launch")
    return out


def _names(sch):
    names = {n for _, n in sch.trace}
    assert names <= set(BC.TRACE_NAMES) | set(BC.EXTRA_NAMES), names
    assert all(c in sch.bjt.cliques for c, _ in sch.trace)
    return names


def _download(sch, cal):
    """(beliefs {clique: [rows, size]}, seps {(p, c): [rows, size]}, marginals {var: [rows, card]}) on the host."""
    from pgmpy_amd import engine as E

    R = sch.n_rows
    beliefs = cal.clique_beliefs_rows(list(range(R)))
    seps = {}
    for pc in sch.bjt.order:
        t, sl = cal.seps[pc]
        assert list(sl) == [v for v in pc[1] if v in pc[0]]
        seps[pc] = np.ascontiguousarray(np.moveaxis(E.to_host(t).reshape([sch.bjt.card[v] for v in sl] + [R]), -1, 0)
                                        ).reshape(R, -1)
    marg = {v: np.array(cal.marginal(v)) for v in sch.bjt.variables}
    return beliefs, seps, marg


def _check(tree, op, got, n_rows, shift=0, skip_rows=()):
    """Every entry of a download against the reference; returns the worst error / bound."""
    ref = BC.reference(tree, OPS[op])
    rp = BC.row_patterns(tree, n_rows, shift)
    rows = np.array([r for r in range(n_rows) if r not in skip_rows])
    beliefs, seps, marg = got
    b = BC.bound(tree, OPS[op])
    worst = 0.0
    assert set(beliefs) == set(tree["cliques"]) and set(seps) == set(ref["seps"])
    assert set(marg) == set(tree["variables"])
    for c in tree["cliques"]:
        assert beliefs[c].shape == (n_rows, ref["beliefs"][c].shape[1])
        worst = max(worst, BC.check(beliefs[c][rows], ref["beliefs"][c][rp][rows], b,
                                    f"{tree['name']} {op} clique {c}"))
    for pc, (want, _) in ref["seps"].items():
        worst = max(worst, BC.check(seps[pc][rows], want[rp][rows], b, f"{tree['name']} {op} sepset {pc}"))
    for v in tree["variables"]:
        mb = BC.marginal_bound(tree, OPS[op], v)
        w = BC.check(marg[v][rows], ref["marginals"][v][rp][rows], mb, f"{tree['name']} {op} marginal {v}")
        worst = max(worst, w)
    if tree["ev_vars"]:  # the impossible rows: all-zero beliefs, NaN marginals
        imp = [r for r in rows if rp[r] == 1]
        assert imp
        assert all(not beliefs[c][imp].any() for c in tree["cliques"])
        assert all(np.isnan(marg[v][imp]).all() for v in tree["variables"])
    return worst


def _calibrate(tree, op, n_rows, bjt=None, graph=True, shift=0):
    bjt = bjt or _bjt(tree)
    sch = bjt.schedule(n_rows, tree["ev_vars"], op, marginals=True, graph=graph)
    cal = sch.run(_upload(BC.codes(tree, n_rows, shift)))
    return sch, cal


def _sweep(tree, op, n_rows):
    sch, cal = _calibrate(tree, op, n_rows)
    names = _names(sch)
    fused = BC.FUSED_ROWS(n_rows)
    want = tree["want"]["any"] | tree["want"]["fused" if fused else "unfused"]
    assert want <= names, f"{tree['name']} at {n_rows} rows misses {sorted(want - names)}; reached {sorted(names)}"
    if not fused:
        assert not names & BC.FUSED_ONLY, names & BC.FUSED_ONLY
    kinds = classify(sch.prog)
    count = {k: kinds.count(k) for k in ("specialised", "generic_fused", "level_job", "own_launch")}
    from pgmpy_amd import program as P

    if fused:  # the kernel takes even row counts from 64 up, and only those; specialised from the threshold up
        big = max(BC.prod(tree["card"][v] for v in c) for c in tree["cliques"]) * n_rows >= P.PM_PREFER_MIN
        assert (count["specialised"] >= 1) == big and count["specialised"] + count["generic_fused"] >= 1, count
    else:
        assert count["specialised"] == 0 and count["generic_fused"] == 0, count
    if n_rows * 256 < P.PM_PREFER_MIN:  # every step below the threshold: jobs of the level batches
        assert count["level_job"] >= 1 and any(n.startswith("level batch of") for n in sch.prog.notes), count
    if "sigma_via_ratio" in names:
        from pgmpy_amd.inference.bp_batch import _SepFromRatio

        assert any(isinstance(s, _SepFromRatio) for s in cal.seps.values())
    got = _download(sch, cal)
    assert int(sch.err.cpu()[0]) == 0
    assert all(r.foot for r in sch.prog._recs) and sch.prog.check_hazards() == []
    worst = _check(tree, op, got, n_rows)
    print(f"{tree['name']} {op} {n_rows} rows: worst error / bound {worst:.3f} (bound {BC.bound(tree, OPS[op]):.3g}); "
          f"steps {count}; branches {sorted(names)}")


@pytest.mark.parametrize("n_rows", SWEEP_ROWS)
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("name", NAMES)
def test_schedule_branches_and_values(gpu, name, op, n_rows):
    _sweep(BC.TREES[name], op, n_rows)


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("name", ["chain3", "nested", "star7_ratio", "star6", "chain_swapped", "deep"])
def test_smallest_fused_row_count(gpu, name, op):
    """66 rows: the fewest (past one wave, with a tail) at which the fused kernel takes the passes; the hubs
    of star6 and star7_ratio (72 and 256 states) reach PM_PREFER_MIN there, no separator does."""
    _sweep(BC.TREES[name], op, 66)


@pytest.mark.parametrize("op", list(OPS))
def test_two_marginals_in_one_pass(gpu, op):
    """`pairs` at the fewest rows whose two-marginal passes have the 256 blocks the kernel asks for: two
    sigma' from the root's operands in one pass, two from the container separator in another."""
    tree = BC.TREES["pairs"]
    sch, cal = _calibrate(tree, op, BC.PAIR_ROWS)
    names = _names(sch)
    assert BC.PAIR_NAMES <= names, sorted(names)
    assert sum(r.note.startswith("product_n_marginals") and r.pm is not None for r in sch.prog._recs) == 2
    got = _download(sch, cal)
    assert int(sch.err.cpu()[0]) == 0
    worst = _check(tree, op, got, BC.PAIR_ROWS)
    print(f"pairs {op} {BC.PAIR_ROWS} rows: worst error / bound {worst:.3f}; branches {sorted(names)}")


def test_every_branch_is_reached_at_every_row_count(gpu):
    """The schedules of all trees, built but not run: every name of the decision table that can occur at a
    row count is reached by some tree there (the fused-only names where the kernel takes the passes, the
    two-marginal passes from PAIR_ROWS rows; the knob's name by the knob test)."""
    for n_rows in SWEEP_ROWS + (66, BC.PAIR_ROWS):
        reached = set()
        for tree in BC.TREES.values():
            if n_rows == BC.PAIR_ROWS and tree["name"] != "pairs":
                continue
            reached |= _names(_bjt(tree).schedule(n_rows, tree["ev_vars"], "marginalize", marginals=True, graph=False))
        if n_rows == BC.PAIR_ROWS:
            want = BC.PAIR_NAMES
        else:
            want = set(BC.TRACE_NAMES) - BC.KNOB_ONLY - BC.PAIR_NAMES - \
                (set() if BC.FUSED_ROWS(n_rows) else BC.FUSED_ONLY)
            assert set(BC.EXTRA_NAMES) <= reached
        assert want <= reached, f"{n_rows} rows: not reached {sorted(want - reached)}"


def _same(a, b):
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k], equal_nan=True), k


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("name,n_rows", [("nested", 66), ("star6", 66), ("deep", 65)])
def test_replay_leaves_no_stale_state(gpu, name, op, n_rows):
    """Batch A, a different batch B, then A again on one cached schedule: the third result is the first bit
    for bit and B is within the bound of its own reference; graph replay and plain replay agree bit for bit."""
    tree = BC.TREES[name]
    bjt = _bjt(tree)
    sch, cal = _calibrate(tree, op, n_rows, bjt)
    a1 = _download(sch, cal)
    _check(tree, op, a1, n_rows)
    sch_b, cal = _calibrate(tree, op, n_rows, bjt, shift=5)
    assert sch_b is sch
    _check(tree, op, _download(sch, cal), n_rows, shift=5)
    sch_a, cal = _calibrate(tree, op, n_rows, bjt)
    assert sch_a is sch
    _same(a1, _download(sch, cal))
    plain, cal = _calibrate(tree, op, n_rows, bjt, graph=False)
    assert plain is not sch and plain.prog._graph is None and sch.prog._graph is not None
    _same(a1, _download(plain, cal))


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("name", ["chain3", "star6", "chain_swapped"])
def test_ratio_knob_off(gpu, monkeypatch, name, op):
    """RATIO_PREMARG off (the A/B knob PGM_BP_RATIO=0): no ratio is stored, every result stays within the
    bound, and the sepset beliefs agree with the ratio-on run (rebuilt by _SepFromRatio) within 2 x bound."""
    from pgmpy_amd.inference import bp_batch as B

    tree = BC.TREES[name]
    sch_on, cal = _calibrate(tree, op, 66)
    assert {"ratio_stored", "sigma_via_ratio"} <= _names(sch_on)
    on = _download(sch_on, cal)
    assert any(isinstance(s, B._SepFromRatio) for s in cal.seps.values())
    monkeypatch.setattr(B, "RATIO_PREMARG", False)
    sch_off, cal = _calibrate(tree, op, 66)
    names = _names(sch_off)
    assert "ratio_knob_off" in names and not names & {"ratio_stored", "sigma_via_ratio", "ratio_declined_by_kernel"}
    assert not any(isinstance(s, B._SepFromRatio) for s in cal.seps.values())
    off = _download(sch_off, cal)
    _check(tree, op, off, 66)
    ref = BC.reference(tree, OPS[op])["seps"]
    rp = BC.row_patterns(tree, 66)
    for pc in on[1]:
        tol = 2 * BC.bound(tree, OPS[op]) * np.abs(ref[pc][0][rp].astype(float))
        assert np.all(np.abs(on[1][pc] - off[1][pc]) <= tol)


def test_error_flag_of_a_code_out_of_range(gpu, monkeypatch):
    """A code equal to the cardinality in one row raises the schedule's flag (IndexError from
    calibrate_frame); that row's indicator is all zero, so its beliefs are exactly 0 and its marginals NaN;
    every other row is within the bound, and the next clean run on the same schedule has a clear flag."""
    import pandas as pd

    tree = BC.TREES["chain3"]
    n_rows, bad = 66, 7
    bjt = _bjt(tree)
    codes = BC.codes(tree, n_rows)
    codes[tree["ev_vars"].index("a"), bad] = tree["card"]["a"]
    sch = bjt.schedule(n_rows, tree["ev_vars"], "marginalize", marginals=True, graph=True)
    cal = sch.run(_upload(codes))
    got = _download(sch, cal)
    assert int(sch.err.cpu()[0]) != 0
    _check(tree, "marginalize", got, n_rows, skip_rows=(bad,))
    assert all(not got[0][c][bad].any() for c in tree["cliques"])
    assert all(not got[1][pc][bad].any() for pc in got[1])
    assert all(np.isnan(got[2][v][bad]).all() for v in tree["variables"])
    # the same codes through calibrate_frame (its encoder cannot produce them: handed in)
    monkeypatch.setattr(bjt, "encode", lambda df: (codes, list(tree["ev_vars"])))
    with pytest.raises(IndexError):
        bjt.calibrate_frame(pd.DataFrame({v: [0] * n_rows for v in tree["ev_vars"]}))
    monkeypatch.setattr(bjt, "encode", lambda df: (BC.codes(tree, n_rows), list(tree["ev_vars"])))
    cal = bjt.calibrate_frame(pd.DataFrame({v: [0] * n_rows for v in tree["ev_vars"]}))
    assert bjt.schedule(n_rows, tree["ev_vars"], "marginalize") is sch and int(sch.err.cpu()[0]) == 0
    _check(tree, "marginalize", _download(sch, cal), n_rows)


@pytest.mark.parametrize("name", ["nested", "star7_ratio"])
def test_belief_propagation_compiled_on_a_synthetic_tree(gpu, monkeypatch, name):
    """BeliefPropagation.calibrate / max_calibrate through the compiled one-row schedule: clique and sepset
    beliefs as DiscreteFactors against the reference's pattern without findings."""
    from pgmpy_amd.inference import BeliefPropagation

    monkeypatch.setenv("PGM_BP_COMPILED", "1")
    tree = BC.TREES[name]
    bp = BeliefPropagation(_junction_tree(tree))
    for call, op in (("calibrate", "sum"), ("max_calibrate", "max"), ("calibrate", "sum")):
        getattr(bp, call)()
        assert bp._bjt is not None and bp._bjt._schedules
        # (one row: the fused kernel declines every pass, so no ratio is stored and no sepset belief is rebuilt
        # from one here; those are checked by the sweep at 66 and 1030 rows)
        assert all(not _names(sch) & BC.FUSED_ONLY for sch in bp._bjt._schedules.values())
        ref = BC.reference(tree, op)
        b = BC.bound(tree, op)
        cb, sb = bp.get_clique_beliefs(), bp.get_sepset_beliefs()
        assert set(cb) == set(tree["cliques"]) and set(sb) == {frozenset(e) for e in tree["edges"]}
        worst = 0.0
        for c in tree["cliques"]:
            f = cb[c]
            vals = np.transpose(np.asarray(f.values), [list(f.variables).index(v) for v in c]).ravel()
            worst = max(worst, BC.check(vals, ref["beliefs"][c][0], b, f"{name} {call} clique {c}"))
        for pc, (want, sl) in ref["seps"].items():
            f = sb[frozenset(pc)]
            assert set(f.variables) == set(sl)
            vals = np.transpose(np.asarray(f.values), [list(f.variables).index(v) for v in sl]).ravel()
            worst = max(worst, BC.check(vals, want[0], b, f"{name} {call} sepset {pc}"))
        print(f"BeliefPropagation {name} {call}: worst error / bound {worst:.3f}")
