"""The case table of the specialised batch generator (tests/nary_cases.py), checked on the host: no device.

Every named case takes the plan its entry names (pgm_contract_n_info for the n-ary jobs, pgm_contract_info for
the pair jobs) and the plain-Python restatement of the planner agrees with the library, so the path classes the
GPU test relies on are proven here.  The table and the seeded random families together reach every path class;
the reference stands on its own against numpy's einsum; no case asks for a byte outside its tensors.
"""
from collections import Counter

import numpy as np
import pytest

from tests import nary_cases as K

NARY = [c["name"] for c in K.CASES if c["kind"] == "nary"]
PAIR = [c["name"] for c in K.CASES if c["kind"] == "pair"]


def _e():
    from pgmpy_amd import engine

    return engine


def _host_tensors(c):
    ops, _, view = K.make_tensors(c, K.make_values(c, "signed"), "cpu")
    return ops, view


def _nary_info(c):
    ops, view = _host_tensors(c)
    return _e().contract_n_info(list(zip(ops, c["ops"])), c["out"], c["reduce"], out=view)


def _assert_nary_plan(c):
    """The library's plan of the case is the restatement's."""
    info, p = _nary_info(c), K.plan_nary(c)
    got = dict(nk=info.nk, nr=info.nr, g_log2=info.g_log2, n_out=info.n_out, n_red=info.n_red, blocks=info.blocks,
               kcard=list(info.kcard[:info.nk]), rcard=list(info.rcard[:info.nr]))
    assert got == {f: p[f] for f in got}, c["name"]
    return got


def _pair_info(c):
    ops, view = _host_tensors(c)
    B = ops[1] if len(ops) > 1 else None
    return _e().contract_info_tensors(ops[0], c["ops"][0], B, c["ops"][1] if B is not None else None, c["out"],
                                      reduce=c["reduce"], combine=c["combine"], out=view)


def _assert_pair_plan(c):
    info = _pair_info(c)
    a_ptr, b_ptr, c_ptr = K.pair_ptrs(c)
    p = K.plan_pair(c, a_ptr=a_ptr, b_ptr=b_ptr, c_ptr=c_ptr)
    got = dict(n_out=info.n_out, n_red=info.n_red, n_ro=info.n_ro, ri_card=info.ri_card,
               nx=info.nx)
    want = dict(n_out=p["n_out"], n_red=p["n_red"], n_ro=p["n_ro"], ri_card=p["ri_card"],
                nx=p["kcard"][-1] if p["kcard"] else 1)
    assert got == want, c["name"]
    return p


# ----------------------------------------------------------------------------- plans
@pytest.mark.parametrize("name", NARY)
def test_named_nary_case_takes_its_plan(name):
    c = K.BY_NAME[name]
    got = _assert_nary_plan(c)
    assert {f: got[f] for f in c["expect"]} == c["expect"]
    assert c["want"] <= K.classes_nary(c), (c["want"] - K.classes_nary(c))


@pytest.mark.parametrize("name", PAIR)
def test_named_pair_case_takes_its_plan(name):
    c = K.BY_NAME[name]
    _assert_pair_plan(c)
    assert c["want"] <= K.classes_of(c), (c["want"] - K.classes_of(c))


def test_random_families_agree_with_the_library_plan():
    for c in K.all_random():
        _assert_nary_plan(c)
    for c in K.random_pair_cases(K.RANDOM_PAIR_SEED, K.RANDOM_PAIRS):
        _assert_pair_plan(c)


def test_contract_n_info_argument_checks():
    import ctypes

    from pgmpy_amd import _native as N

    lib = N.load_library()
    d = N.ContractNDesc()
    d.n_ops, d.reduce, d.n_keep, d.n_red = 1, N.RED_SUM, 1, 0
    d.keep_card[0], d.keep_sc[0], d.keep_s[0][0] = 0, 1, 1
    info = N.ContractNInfo()
    assert lib.pgm_contract_n_info(ctypes.byref(d), None, ctypes.byref(info)) == N.PGM_OK
    assert info.n_out == 0 and info.blocks == 0  # an empty output: no job
    assert lib.pgm_contract_n_info(ctypes.byref(d), None, None) == N.PGM_EINVAL
    assert lib.pgm_contract_n_info(None, None, ctypes.byref(info)) == N.PGM_EINVAL
    d.n_ops = N.PRODN_MAX_OPS + 1
    assert lib.pgm_contract_n_info(ctypes.byref(d), None, ctypes.byref(info)) == N.PGM_EINVAL


# ----------------------------------------------------------------------------- coverage
def test_table_and_random_family_cover_every_path_class():
    named = set().union(*[K.classes_of(c) for c in K.CASES])
    rnd = K.all_random()
    rpairs = K.random_pair_cases(K.RANDOM_PAIR_SEED, K.RANDOM_PAIRS)
    assert len(rnd) >= 200 and len(rpairs) >= 100
    # each class has a named case of its own: the random family is breadth, not the only witness
    assert K.NARY_CLASSES <= named, K.NARY_CLASSES - named
    assert K.PAIR_CLASSES <= named, K.PAIR_CLASSES - named
    every = named.union(*[K.classes_of(c) for c in rnd + rpairs])
    assert (K.NARY_CLASSES | K.PAIR_CLASSES) <= every
    count = Counter(x for c in rnd for x in K.classes_nary(c))
    low = {k: count[k] for k in K.RANDOM_FLOOR_CLASSES if count[k] < K.RANDOM_FLOOR}
    assert not low, low
    for c in rnd:
        assert 1 <= len(c["ops"]) <= 8 and all(1 <= len(o) <= 5 for o in c["ops"])
        assert all(1 <= v <= 9 for v in c["ext"].values())
        assert K.prod(K.out_shape(c)) >= 1 and K.n_red_of(c) <= K.MAX_RED
    print("named cases per class:", dict(sorted(Counter(x for c in K.CASES for x in K.classes_of(c)).items())))
    print("random n-ary cases per class:", dict(sorted(count.items())))
    print("random pair cases per class:", dict(sorted(Counter(x for c in rpairs for x in K.classes_of(c)).items())))


def test_cases_stay_small():
    """The largest tensor of any case is a few MB and the reference holds at most 2^21 terms per case (only the
    grid-stride and one-lane-per-output cases need more than a few thousand outputs)."""
    for c in K.CASES + K.all_random() + K.random_pair_cases(K.RANDOM_PAIR_SEED, K.RANDOM_PAIRS):
        sizes = [K.operand_layout(K.op_shape(c, t), c["views"][t])[0] for t in range(len(c["ops"]))]
        lay = K.out_layout(K.out_shape(c), c["out_kind"])
        sizes.append(lay[0] if lay else K.prod(K.out_shape(c)))
        assert 8 * max(sizes) <= 4 << 20, c["name"]
        assert K.prod(K.out_shape(c)) * K.n_red_of(c) <= K.MAX_WORK, c["name"]


# ----------------------------------------------------------------------------- the reference on its own
def _einsum(c, arrays, out_labels):
    ix = lambda ls: [ord(l) - ord("a") for l in ls]  # noqa: E731
    args = []
    for a, ls in zip(arrays, c["ops"]):
        args += [a, ix(ls)]
    with np.errstate(all="ignore"):
        return np.einsum(*args, ix(out_labels))


def _einsum_cases():
    cases = K.CASES + K.all_random() + K.random_pair_cases(K.RANDOM_PAIR_SEED, K.RANDOM_PAIRS)
    return [c for c in cases if c["kind"] == "nary" or c["combine"] in ("mul", "copy")]


def test_reference_agrees_with_einsum_on_finite_values():
    """Sum cases: ref within the bound of a plain fp64 einsum (which also rounds every product, and adds in an
    order of its own), mag > 0 on at least 99 % of the outputs.  Max / product cases: exactly numpy's."""
    for values in ("signed", "zeros"):
        for c in _einsum_cases():
            arrays = K.make_values(c, values)
            r, mag = K.ref(c, arrays)
            if c["reduce"] == "sum":
                e = _einsum(c, arrays, c["out"])
                assert np.isfinite(e).all() and np.isfinite(r).all()
                assert (np.abs(e.astype(K.LD) - r) <= K.bound(c, mag)).all(), c["name"]
                if values == "signed":
                    assert np.count_nonzero(mag > 0) >= 0.99 * mag.size, c["name"]
                continue
            full = _einsum(c, arrays, c["out"] + K.red_labels(c))
            full = full.reshape(K.prod(K.out_shape(c)), -1)
            np.testing.assert_array_equal(r.reshape(-1), full.max(axis=1), err_msg=c["name"])


def test_reference_gives_numpys_special_value_pattern():
    seen = Counter()
    for c in _einsum_cases():
        arrays = K.make_values(c, "specials")
        r, mag = K.ref(c, arrays)
        if c["reduce"] == "sum":
            e = _einsum(c, arrays, c["out"])
        else:
            full = _einsum(c, arrays, c["out"] + K.red_labels(c))
            with np.errstate(all="ignore"):
                e = full.reshape(K.prod(K.out_shape(c)), -1).max(axis=1).reshape(r.shape)
        np.testing.assert_array_equal(np.isnan(r), np.isnan(e), err_msg=c["name"])
        np.testing.assert_array_equal(np.isposinf(r), np.isposinf(e), err_msg=c["name"])
        np.testing.assert_array_equal(np.isneginf(r), np.isneginf(e), err_msg=c["name"])
        seen.update(nan=int(np.isnan(e).sum()), pinf=int(np.isposinf(e).sum()), ninf=int(np.isneginf(e).sum()),
                    finite=int(np.isfinite(e).sum()))
    assert all(seen[k] > 100 for k in ("nan", "pinf", "ninf", "finite")), seen


def test_compare_rejects_a_wrong_sum_and_a_missing_special():
    """The comparison the GPU test uses fails on an output off by a few ulp of the magnitude and on a NaN where
    the reference has a number."""
    c = K.BY_NAME["g8_lanemap"]
    arrays = K.make_values(c, "signed")
    r, mag = K.ref(c, arrays)
    good = r.astype(np.float64)
    assert K.compare(c, good, arrays) <= 1.0
    off = good.copy()
    off[3] += float(2 * K.bound(c, mag)[3])
    with pytest.raises(AssertionError):
        K.compare(c, off, arrays)
    off = good.copy()
    off[-1] = np.nan
    with pytest.raises(AssertionError):
        K.compare(c, off, arrays)


# ----------------------------------------------------------------------------- footprints
def test_every_case_descriptor_stays_inside_its_tensors():
    """hazard.contract_n_foot / contract_foot of each case's descriptor on its real views: every byte range
    lies inside the storage of the tensor it belongs to."""
    import ctypes

    from pgmpy_amd import hazard as H

    E = _e()
    for c in K.CASES + K.all_random() + K.random_pair_cases(K.RANDOM_PAIR_SEED, K.RANDOM_PAIRS):
        ops, view = _host_tensors(c)
        if view is None:
            import torch

            view = torch.empty(K.out_shape(c), dtype=torch.float64)
        if c["kind"] == "nary":
            d, _ = E.contract_n_desc([(t.shape, t.stride(), ls) for t, ls in zip(ops, c["ops"])], c["out"],
                                     c["reduce"], view.stride())
            foot = H.contract_n_foot(d, [t.data_ptr() for t in ops], view.data_ptr())
        else:
            B = ops[1] if len(ops) > 1 else None
            d, _ = E.contract_desc(c["ops"][0], ops[0].shape, ops[0].stride(), c["ops"][1] if B is not None else None,
                                   B.shape if B is not None else (), B.stride() if B is not None else (), c["out"],
                                   c["reduce"], c["combine"], view.stride())
            foot = H.contract_foot(d, ctypes.c_void_p(ops[0].data_ptr()),
                                   None if B is None else ctypes.c_void_p(B.data_ptr()), ctypes.c_void_p(view.data_ptr()))
        tensors = ops + [view]
        assert len(foot) == len(tensors), c["name"]
        for (lo, hi, mode), t in zip(foot, tensors):
            s = t.untyped_storage()
            assert s.data_ptr() <= lo < hi <= s.data_ptr() + s.nbytes(), (c["name"], mode)
        assert foot[-1][2] == H.WRITE
