"""The launch of every entry of tests/rows_cases.py, checked on the host (pgm_rows_launch_info: no device):
every entry compiles and takes the path it is in the table for, the table covers every ahead-of-time row
kernel instance, and its long-double reference stands on its own (live rows, the 1 % condition of the
random family, agreement with the project's oracle)."""
import numpy as np
import pytest

from pgmpy_amd import _native as N
from tests import rows_cases as RC

FIELDS = ("kernel", "values_lds", "acc_lds", "maxfc", "maxt", "nf", "nt", "map", "rg", "blocks", "wg", "lds_bytes")
_BUILT = {}


def built(spec):
    """(factors, plan struct, values) of a case's plan, once per plan name."""
    key = spec["plan"]
    if key not in _BUILT:
        f = RC.make_factors(spec)
        _BUILT[key] = (spec, f) + RC.build_plan(spec, f)
    first, f, pl, values = _BUILT[key]
    assert all(first[k] == spec[k] for k in ("comps", "family", "seed", "n_values")), (first["name"], spec["name"])
    return f, pl, values


def info_dict(info):
    return {k: getattr(info, k) for k in FIELDS}


@pytest.mark.parametrize("spec", RC.CASES + [RC.RING], ids=lambda s: s["name"])
def test_case_compiles_and_takes_its_path(spec):
    _, pl, values = built(spec)
    assert values.size == pl.n_values
    got = info_dict(RC.launch_info(spec, pl))
    want = spec["expect"]
    assert {k: got[k] for k in want} == want, got
    specialisable = all(len(c["q"]) <= 1 and not c["h"] for c in spec["comps"])
    src = RC.plan_source(pl)
    assert (src is not None) == specialisable
    if got["kernel"] in (RC.JIT, RC.JIT2):
        assert specialisable
        grid = src[:src.index("pgm_rows_floor")]  # pgm_rows_jit and pgm_rows_jit2 (the ring always stages)
        assert ("#define VAL(i) S[i]" in grid) == bool(got["values_lds"])
        assert ("#define VAL(i) V[i]" in grid) != bool(got["values_lds"])


def test_table_covers_every_aot_instance_and_family():
    seen_table, seen_affine, fams, jit_lds, rgs = set(), set(), set(), set(), set()
    for spec in RC.CASES:
        _, pl, _ = built(spec)
        i = info_dict(RC.launch_info(spec, pl))
        fams.add(i["kernel"])
        rgs.add(i["rg"])
        if i["kernel"] == RC.TABLE:
            seen_table.add((i["values_lds"], i["acc_lds"], i["maxfc"], i["maxt"]))
        elif i["kernel"] == RC.AFFINE:
            seen_affine.add((i["values_lds"], i["nf"], i["nt"], i["map"]))
        else:
            jit_lds.add(i["values_lds"])
    assert seen_table == {(vl, al, fc, t) for vl in (0, 1) for al in (0, 1) for fc in (2, 4, 8, 16) for t in (4, 8, 48)}
    assert seen_affine == {(vl, nf, nt, mp) for vl in (0, 1) for nf in (1, 2, 4) for nt in (4, 8) for mp in (0, 1)}
    assert fams == {RC.JIT, RC.JIT2, RC.AFFINE, RC.TABLE}
    assert jit_lds == {0, 1}
    assert {1, 2, 3} <= rgs
    # at most about a dozen distinct specialised plans (hipRTC time)
    assert len({s["plan"] for s in RC.CASES if s["expect"].get("kernel") in (RC.JIT, RC.JIT2)}) <= 14


def _ref(spec):
    f, _, _ = built(spec)
    codes = RC.make_codes(spec)
    return RC.reference(spec, f, codes[:, spec["row0"]:spec["row0"] + spec["n_rows"]])


@pytest.mark.parametrize("spec", RC.CASES + [RC.RING], ids=lambda s: s["name"])
def test_reference_alone(spec):
    """Enough live rows to test anything, the dead rows a case is there for, the expected flag, and for the
    random family at most 1 % of the live rows too close to a tie to assert MAP on."""
    ref = _ref(spec)
    n = spec["n_rows"]
    live = int((~ref["dead"]).sum())
    assert live >= n // 4, (live, n)
    assert int(ref["dead"].sum()) >= spec["min_dead"]
    assert ref["err"] == (1 if spec["oob"] else 0)
    assert int(ref["near"].sum()) <= 0.01 * live, (int(ref["near"].sum()), live)
    assert np.isnan(ref["marg"][:, ref["dead"]]).all() and not np.isnan(ref["marg"][:, ~ref["dead"]]).any()
    if spec["family"] == "exact":  # the family's claim: every unnormalised entry is an fp64 number
        for t in ref["tables"]:
            assert (t.astype(np.float64).astype(t.dtype) == t).all()


def test_exact_family_has_ties():
    tied = sum(int(((r["gap"] == 0) & ~r["dead"]).sum()) for r in (_ref(s) for s in RC.CASES[:72:4]))
    assert tied > 100


@pytest.mark.parametrize("name", ["nq3_h2_random", "mixed_simple_table"])
def test_reference_matches_oracle(name):
    """The same spec expressed for the project's oracle: per row, every factor becomes an oracle factor
    over named variables, evidence is reduced away (OFactor.reduce), each component is contracted to its
    query variables by oracle.ve.greedy_contract (float64), and the long-double reference agrees with it to
    a few times the family's bound."""
    from oracle import ve as OVE
    from oracle.factor import OFactor

    spec = next(s for s in RC.CASES if s["name"] == name)
    f, _, _ = built(spec)
    codes = RC.make_codes(spec)[:, :24]
    ref = RC.reference(dict(spec, n_rows=24, row0=0, oob=()), f, codes)
    for r in range(24):
        z, margs = 1.0, []
        for ci, (c, fs) in enumerate(zip(spec["comps"], f)):
            ops = []
            for ax, arr in zip(c["facs"], fs):
                names = [f"e{a[1]}" if a[0] == "e" else f"{a[0]}{ci}_{a[1]}" for a in ax]
                ev = {f"e{a[1]}": int(codes[a[1], r]) for a in ax if a[0] == "e"}
                ops.append(OFactor(names, arr.shape, arr).reduce(ev))
            qv = [f"q{ci}_{i}" for i in range(len(c["q"]))]
            t = np.asarray(OVE.greedy_contract(ops, qv), dtype=np.float64)
            mass = float(t.sum())
            z *= mass
            for i in range(len(qv)):
                with np.errstate(invalid="ignore", divide="ignore"):
                    margs.append(t.sum(axis=tuple(k for k in range(len(qv)) if k != i)) / mass)
        assert bool(ref["dead"][r]) == (not z > 0)
        if z > 0:
            np.testing.assert_allclose(np.concatenate(margs), ref["marg"][:, r].astype(np.float64),
                                       rtol=4 * ref["mcoef"].max() * RC.U, atol=0)


def test_launch_info_checks_arguments_like_run():
    spec = RC.CASES[0]
    _, pl, _ = built(spec)
    with pytest.raises(ValueError, match="rows_plan_run: null codes"):
        N.rows_launch_info(pl, RC.ALL, 10, codes=None)
    with pytest.raises(ValueError, match="marginals requested, marg is null"):
        N.rows_launch_info(pl, RC.ALL, 10, marg=None)
    with pytest.raises(ValueError, match="joint output needs a single-component plan"):
        N.rows_launch_info(pl, RC.JOINT, 10)
    with pytest.raises(ValueError, match="ld_out 5 < n_rows 10"):
        N.rows_launch_info(pl, RC.ALL, 10, ld_out=5)
    assert N.rows_launch_info(pl, RC.ALL, 0).kernel == N.RK_NONE
    assert N.rows_launch_info(pl, RC.ALL, 0).blocks == 0
