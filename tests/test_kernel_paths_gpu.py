"""Every primitive kernel path against a high-precision reference, with signed and special values.

pgm_contract runs every entry of tests/kernel_cases.py (the plan of each is first checked on the real
tensors with pgm_contract_info, so the test knows which kernel ran).  Sums are compared with a long-double
einsum under the worst-case bound of floating-point summation,

    |got - ref| <= (n_red + 2) * 2^-53 * sum_i |a_i| |b_i|,

which holds for any summation order, with or without FMA (n_red - 1 additions and one rounding per
product, to first order in 2^-53; the + 2 covers the second-order terms and the rounding of the
reference).  Max, copy and the elementwise combines are single IEEE operations: exact against numpy.
pgm_argmax, pgm_indicator, pgm_gather, pgm_codes_select, pgm_codes_remap and pgm_product_n are called
through ctypes with their production strides and compared with numpy.
"""
import math

import numpy as np
import pytest

from tests import kernel_cases as K

pytestmark = pytest.mark.gpu

LD = np.longdouble
HAVE_LD = np.finfo(LD).eps < 2.0 ** -60  # 80-bit extended or better; else math.fsum of the fp64 products
SENTINEL = -12345.678
DENORMAL = 5e-324 * 1023
GPU_CASES = [c["name"] for c in K.CASES if c["gpu"]]
REDUCING = [n for n in GPU_CASES if K.BY_NAME[n]["reduce"] is not None]
ELEMENTWISE = [n for n in GPU_CASES if K.BY_NAME[n]["reduce"] is None]


def _e():
    from pgmpy_amd import engine

    return engine


def _n():
    from pgmpy_amd import _native

    return _native


# ----------------------------------------------------------------------------- plumbing
def _dev(arr, off=0):
    """Host array -> device tensor of the same dtype and shape whose address is 16-B aligned plus
    off * itemsize (a view into a buffer off elements longer)."""
    E = _e()
    a = np.ascontiguousarray(arr)
    if off == 0:
        t = E.to_device_raw(a)
    else:
        flat = np.concatenate([np.zeros(off, dtype=a.dtype), a.reshape(-1)])
        t = E.to_device_raw(flat)[off:].view(a.shape)
    assert t.data_ptr() % 16 == (off * a.dtype.itemsize) % 16
    return t


def _host(t):
    return t.cpu().numpy()


def _out_buffer(c):
    """(buffer, view) of the case's output: the view has the strides and offset of K.out_layout, the buffer
    is filled with the sentinel (None, None for the engine-allocated C-order output)."""
    import torch

    if c["out"] is None:
        return None, None
    buf_shape, shape, strides, off = K.out_layout(c)
    buf = torch.full(buf_shape, SENTINEL, dtype=torch.float64, device="cuda")
    if c["out"] == "T":
        view = buf.permute(*reversed(range(len(shape))))
    elif len(shape) == 1:
        view = buf[K.PAD_LO:K.PAD_LO + 2 * shape[0]:2]
    else:
        view = buf[tuple(slice(K.PAD_LO, K.PAD_LO + s) for s in shape)]
    assert list(view.shape) == shape and list(view.stride()) == strides
    assert view.data_ptr() - buf.data_ptr() == 8 * off
    return buf, view


def _check_sentinels(c, buf, view):
    """Nothing outside the view was written."""
    if buf is None or c["out"] == "T":
        return
    import torch

    mask = torch.ones_like(buf, dtype=torch.bool)
    shape = list(view.shape)
    if len(shape) == 1:
        mask[K.PAD_LO:K.PAD_LO + 2 * shape[0]:2] = False
    else:
        mask[tuple(slice(K.PAD_LO, K.PAD_LO + s) for s in shape)] = False
    assert bool((buf[mask] == SENTINEL).all()), "a padding element was overwritten"


def _ix(labels):
    return [ord(l) - ord("a") for l in labels]


def _check_plan(c, A, B, out, reduce, combine):
    """The plan on the real tensors is the table's (real alignment decides ROWS_TAB2)."""
    E = _e()
    info = E.contract_info_tensors(A, c["la"], B, c["lb"], c["keep"], reduce=reduce, combine=combine, out=out)
    got = {f: (tuple(info.grid) if f == "grid" else getattr(info, f)) for f in c["expect"]}
    assert got == c["expect"], (c["name"], reduce, combine)
    return info


def _run(c, A, B, reduce, combine):
    """One pgm_contract of the case -> host result (sentinels of a strided out= checked)."""
    E = _e()
    buf, view = _out_buffer(c)
    _check_plan(c, A, B, view, reduce, combine)
    got = E.contract(A, c["la"], B, c["lb"], c["keep"], reduce=reduce, combine=combine, out=view)
    res = _host(got)
    _check_sentinels(c, buf, view)
    return res


# ----------------------------------------------------------------------------- references
def _red_labels(c):
    lb = c["lb"] or []
    return [l for l in dict.fromkeys(c["la"] + lb) if l not in c["keep"]]


def _n_red(c):
    return int(np.prod([c["ext"][l] for l in _red_labels(c)], dtype=np.int64))


def _einsum(c, a, b, out_labels, dtype):
    ops = [a.astype(dtype, copy=False), _ix(c["la"])]
    if b is not None:
        ops += [b.astype(dtype, copy=False), _ix(c["lb"])]
    return np.einsum(*ops, _ix(out_labels))


def _full(c, a, b):
    """COMBINE(A, B) over (kept labels, reduced labels), fp64: one IEEE operation per element."""
    labels = c["keep"] + _red_labels(c)
    with np.errstate(all="ignore"):
        return _einsum(c, a, b, labels, np.float64)


def _ref_sum(c, a, b):
    """(reference sum, sum of |a||b|) per output element in long double (NaN / inf where the inputs give
    them; the magnitudes count finite terms only)."""
    with np.errstate(all="ignore"):
        fa = np.where(np.isfinite(a), np.abs(a), 0.0)
        fb = None if b is None else np.where(np.isfinite(b), np.abs(b), 0.0)
        if HAVE_LD:
            return _einsum(c, a, b, c["keep"], LD), _einsum(c, fa, fb, c["keep"], LD)
        full = _full(c, a, b)
        n_out = int(np.prod(full.shape[:len(c["keep"])], dtype=np.int64))
        rows = full.reshape(n_out, -1)
        ref = np.array([math.fsum(r) if np.isfinite(r).all() else r.sum() for r in rows]).reshape(full.shape[:len(c["keep"])])
        return ref.astype(LD), _einsum(c, fa, fb, c["keep"], np.float64).astype(LD)


def _assert_sum(c, got, a, b):
    ref, mag = _ref_sum(c, a, b)
    assert got.shape == ref.shape
    # the NaN / +inf / -inf pattern is numpy's exactly
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(ref))
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
    fin = np.isfinite(ref)
    err = np.abs(got[fin].astype(LD) - ref[fin])
    bound = (_n_red(c) + 2) * LD(2.0) ** -53 * mag[fin]
    ratio = float(np.max(err / np.where(bound > 0, bound, 1), initial=0.0))
    print(f"{c['name']}: worst |got - ref| / bound = {ratio:.3f} over {int(fin.sum())} finite outputs")
    bad = err > bound
    assert not bad.any(), f"{int(bad.sum())} outputs beyond the summation bound (worst ratio {ratio:.3f})"


def _assert_max(c, got, a, b):
    full = _full(c, a, b)
    nk = len(c["keep"])
    ref = np.max(full.reshape(full.shape[:nk] + (-1,)), axis=-1)
    np.testing.assert_array_equal(got, ref)


def _signed(c, rng):
    sa, sb = K.operand_shapes(c)
    a = rng.uniform(-1.0, 1.0, sa)
    b = None if sb is None else rng.uniform(-1.0, 1.0, sb)
    return a, b


def _plant_reduction_specials(c, a):
    """NaN, +inf, -inf, -0.0 and a denormal at fixed reduction entries of fixed outputs of A: the first and
    the last reduction entry (the last lies in the last ragged chunk / lane and in the last used split), and
    one in the middle; one output's whole reduction is -inf."""
    keep_ax = [c["la"].index(l) for l in c["keep"] if l in c["la"]]
    red_ax = [i for i in range(a.ndim) if i not in keep_ax]
    assert red_ax
    n_keep = int(np.prod([a.shape[i] for i in keep_ax], dtype=np.int64)) if keep_ax else 1

    def at(out_i, where):
        idx = [0] * a.ndim
        if keep_ax:
            ki = np.unravel_index(out_i % n_keep, [a.shape[i] for i in keep_ax])
            for ax, v in zip(keep_ax, ki):
                idx[ax] = int(v)
        for ax in red_ax:
            idx[ax] = {"first": 0, "last": a.shape[ax] - 1, "mid": a.shape[ax] // 2}[where]
        return tuple(idx)

    def whole(out_i):
        idx = [slice(None)] * a.ndim
        if keep_ax:
            ki = np.unravel_index(out_i % n_keep, [a.shape[i] for i in keep_ax])
            for ax, v in zip(keep_ax, ki):
                idx[ax] = int(v)
        return tuple(idx)

    plants = [(0, "first", np.nan), (1, "last", np.nan), (3, "last", np.inf), (4, "first", np.inf),
              (4, "last", -np.inf), (5, "first", -np.inf), (6, "mid", -0.0), (6, "last", DENORMAL),
              (n_keep - 1, "mid", np.nan)][:9 if n_keep > 8 else 8]
    if n_keep > 2:
        a[whole(2)] = -np.inf
    for out_i, where, v in plants:
        if out_i < n_keep and not (out_i == 2 and n_keep > 2):
            a[at(out_i, where)] = v
    return a


# ----------------------------------------------------------------------------- pgm_contract: reductions
@pytest.mark.parametrize("name", REDUCING)
def test_contract_reduction_signed(gpu, name):
    """Signed finite values (sums cancel): the sum within the worst-case bound, the max exact."""
    c = K.BY_NAME[name]
    a, b = _signed(c, np.random.default_rng(7))
    A, B = _dev(a, c["a_off"]), None if b is None else _dev(b)
    _assert_sum(c, _run(c, A, B, "sum", c["combine"]), a, b)
    _assert_max(c, _run(c, A, B, "max", c["combine"]), a, b)


@pytest.mark.parametrize("name", REDUCING)
def test_contract_reduction_special_values(gpu, name):
    """NaN, +-inf, -0.0 and a denormal at the first, a middle and the last reduction entry, and an all -inf
    reduction: max equals np.max (NaN propagates), the sum has numpy's NaN / inf pattern and its finite
    outputs meet the bound."""
    c = K.BY_NAME[name]
    a, b = _signed(c, np.random.default_rng(8))
    a = _plant_reduction_specials(c, a)
    A, B = _dev(a, c["a_off"]), None if b is None else _dev(b)
    gm = _run(c, A, B, "max", c["combine"])
    _assert_max(c, gm, a, b)
    if c["combine"] == "copy" and gm.size > 2:
        assert gm.reshape(-1)[2] == -np.inf  # the all -inf reduction
        assert np.isnan(gm.reshape(-1)[0]) and np.isnan(gm.reshape(-1)[1])
    _assert_sum(c, _run(c, A, B, "sum", c["combine"]), a, b)


# ----------------------------------------------------------------------------- pgm_contract: elementwise
def _bcast(c, x, labels):
    """Operand x[labels] broadcast to the kept labels' order."""
    have = [l for l in c["keep"] if l in labels]
    x = np.transpose(x, [labels.index(l) for l in have])
    shape = [c["ext"][l] if l in labels else 1 for l in c["keep"]]
    return x.reshape(shape)


def _ref_elementwise(c, a, b, combine):
    av = np.broadcast_to(_bcast(c, a, c["la"]), [c["ext"][l] for l in c["keep"]])
    if combine == "copy":
        return np.array(av)
    bv = _bcast(c, b, c["lb"])
    with np.errstate(all="ignore"):
        if combine == "mul":
            return av * bv
        if combine == "add":
            return av + bv
        r = av / bv
        if combine == "div":
            r[np.isnan(r)] = 0.0
        return r


def _plant_elementwise_specials(c, a, b):
    """Specials at the first and last elements and in the middle of A; 0.0 at the same innermost index of
    both operands (0/0) and in B alone (x/0)."""
    fa = a.reshape(-1)
    n = fa.size
    for j, v in enumerate([np.nan, np.inf, -np.inf, -0.0, DENORMAL]):
        for base in (0, n // 2, n - 5):
            fa[base + j] = v
    if b is not None:
        fb = b.reshape(-1)
        m = fb.size  # B spans the innermost kept label, A is C-order with it last
        for j in (7, m // 3, m - 7):
            fb[j] = 0.0  # x / 0 -> +-inf at every outer index
        fa[7], fa[m // 3] = 0.0, -0.0  # outer index 0: 0 / 0
    return a, b


@pytest.mark.parametrize("name", ELEMENTWISE)
@pytest.mark.parametrize("values", ["signed", "special"])
def test_contract_elementwise_exact(gpu, name, values):
    """mul / add / div / div_raw / copy without a reduction: one IEEE operation per element, exact (the
    4-wide unrolled loop, its tail, the grid.y wrap, strided out=).  div: 0/0 -> 0, NaN/x -> 0, x/0 -> +-inf."""
    c = K.BY_NAME[name]
    rng = np.random.default_rng(9)
    sa, sb = K.operand_shapes(c)
    a = rng.uniform(-1.0, 1.0, sa)
    b = None if sb is None else rng.uniform(0.5, 1.5, sb) * rng.choice([-1.0, 1.0], sb)
    if values == "special":
        a, b = _plant_elementwise_specials(c, a, b)
    A, B = _dev(a, c["a_off"]), None if b is None else _dev(b)
    for combine in (["copy"] if b is None else ["mul", "add", "div", "div_raw"]):
        got = _run(c, A, B, None, combine)
        ref = _ref_elementwise(c, a, b, combine)
        np.testing.assert_array_equal(got, ref, err_msg=combine)
        if values == "special" and combine == "div":
            assert not np.isnan(got).any() and np.isinf(got).any() and (got == 0.0).any()
        if values == "special" and combine == "div_raw":
            assert np.isnan(got).any()


def test_normalize_in_place_unrolled(gpu):
    """normalize_ on 1,600,001 elements: the total within the summation bound, then A / total written over A
    (out=A, the 4-wide loop) within 2 ulp of the long-double quotient by that total (one correctly rounded
    division per element; the total's own error is the sum bound's business)."""
    E = _e()
    c = K.BY_NAME["rows_none_unrolled_1d"]
    n = c["ext"]["x"]
    a = np.random.default_rng(10).random(n)
    A = _dev(a)
    s = _host(E.total(A))
    ref_s = a.astype(LD).sum() if HAVE_LD else LD(math.fsum(a))
    assert abs(LD(float(s)) - ref_s) <= (n + 2) * LD(2.0) ** -53 * ref_s
    info = E.contract_info_tensors(A, [0], E.scalar(1.0), [], [0], combine="div_raw", out=A)
    assert info.kernel == K.ROWS and info.unrolled == 1
    E.normalize_(A)
    got = _host(A)
    if HAVE_LD:
        ref = a.astype(LD) / LD(float(s))
        err = np.abs(got.astype(LD) - ref)
        assert (err <= 2 * np.spacing(np.abs(got))).all()
    else:
        np.testing.assert_array_equal(got, a / float(s))
    print("normalize_: worst error in ulp of the true quotient a / sum(a):",
          float(np.max(np.abs(got.astype(LD) - a.astype(LD) / ref_s) / np.spacing(got))))


# ----------------------------------------------------------------------------- pgm_argmax
def _argmax(X, n_rows, row_len, s_row, s_elem, want64, want32):
    import torch

    N = _n()
    o64 = torch.full((n_rows,), -7, dtype=torch.int64, device="cuda") if want64 else None
    o32 = torch.full((n_rows,), -7, dtype=torch.int32, device="cuda") if want32 else None
    N.check(N.lib().pgm_argmax(N.ptr(X), n_rows, row_len, s_row, s_elem, N.ptr(o64), N.ptr(o32), N.stream_handle()),
            "argmax")
    return (None if o64 is None else _host(o64)), (None if o32 is None else _host(o32))


def _argmax_rows(row_len, rng):
    """5 rows: random; the maximum twice (at 10 and 67 when the row is long enough: lane 3 of 64 holds the
    later index); NaN twice the same way; a NaN after a +inf; all -inf."""
    x = rng.uniform(-1.0, 1.0, (5, row_len))
    i0, i1 = (10, 67) if row_len > 67 else (0, row_len - 1)
    x[1, i0] = x[1, i1] = 2.0
    x[2, i0] = x[2, i1] = np.nan
    if row_len >= 3:
        x[3, 0], x[3, row_len - 1] = np.inf, np.nan
    x[4, :] = -np.inf
    return x


@pytest.mark.parametrize("row_len", [1, 2, 3, 63, 64, 65, 1000])
def test_argmax_lane_merge_and_layouts(gpu, row_len):
    x = _argmax_rows(row_len, np.random.default_rng(row_len))
    ref = np.argmax(x, axis=1)
    if row_len > 67:
        assert ref[1] == 10 and ref[2] == 10 and ref[3] == row_len - 1 and ref[4] == 0
    X = _dev(x)
    g64, _ = _argmax(X, 5, row_len, row_len, 1, True, False)
    np.testing.assert_array_equal(g64, ref)
    XT = _dev(np.ascontiguousarray(x.T))  # column-major rows: element stride n_rows, row stride 1
    _, g32 = _argmax(XT, 5, row_len, 1, 5, False, True)
    np.testing.assert_array_equal(g32, ref)
    b64, b32 = _argmax(XT, 5, row_len, 1, 5, True, True)
    np.testing.assert_array_equal(b64, ref)
    np.testing.assert_array_equal(b32, ref)


def test_argmax_one_lane_per_row(gpu):
    """524,288 rows of 3: one lane per row (no shuffle merge), both layouts."""
    n = 524288
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.0, 1.0, (n, 3))
    x[5] = [1.0, 1.0, 0.0]
    x[6] = [0.0, np.nan, np.nan]
    x[7] = [np.inf, 0.0, np.nan]
    x[n - 1] = -np.inf
    x[n - 2] = [0.0, 3.0, 3.0]
    ref = np.argmax(x, axis=1)
    g64, g32 = _argmax(_dev(x), n, 3, 3, 1, True, True)
    np.testing.assert_array_equal(g64, ref)
    np.testing.assert_array_equal(g32, ref)
    _, c32 = _argmax(_dev(np.ascontiguousarray(x.T)), n, 3, 1, n, False, True)
    np.testing.assert_array_equal(c32, ref)


# ----------------------------------------------------------------------------- pgm_indicator
@pytest.mark.parametrize("card", [1, 2, 7])
@pytest.mark.parametrize("n_rows", [1, 255, 257])
def test_indicator(gpu, card, n_rows):
    import torch

    N = _n()
    rng = np.random.default_rng(card * 1000 + n_rows)
    for bad in (False, True):
        codes = rng.integers(0, card, n_rows).astype(np.uint8)
        codes[n_rows // 2] = 255  # not observed: the state column is all 1.0
        if bad:
            codes[n_rows - 1] = card  # out of range: error flag, column all 0.0
        ref = ((codes[None, :] == np.arange(card)[:, None]) | (codes[None, :] == 255)).astype(np.float64)
        C = _dev(codes)
        for transposed in (False, True):
            shape = (n_rows + 3, card + 2) if transposed else (card + 2, n_rows + 3)
            buf = torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")
            view = buf[2:2 + n_rows, 1:1 + card].t() if transposed else buf[1:1 + card, 2:2 + n_rows]
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            N.check(N.lib().pgm_indicator(N.ptr(C), n_rows, card, N.ptr(view), int(view.stride(0)), int(view.stride(1)),
                                          N.ptr(err), N.stream_handle()), "indicator")
            np.testing.assert_array_equal(_host(view), ref)
            assert int(err.item()) == (1 if bad and codes[n_rows - 1] != 255 else 0)
            mask = torch.ones_like(buf, dtype=torch.bool)
            if transposed:
                mask[2:2 + n_rows, 1:1 + card] = False
            else:
                mask[1:1 + card, 2:2 + n_rows] = False
            assert bool((buf[mask] == SENTINEL).all())


# ----------------------------------------------------------------------------- pgm_gather
@pytest.mark.parametrize("row_pos", [0, 1, 2])
def test_gather_row_position_offset_and_error(gpu, row_pos):
    """ROW first, in the middle and last in the output; rows [37, 37 + n_rows) of codes with a leading
    dimension 13 beyond the rows; one static and two per-row evidence labels (200 and 5 states)."""
    import torch

    E, N = _e(), _n()
    rng = np.random.default_rng(20 + row_pos)
    a = rng.uniform(-1.0, 1.0, (3, 200, 4, 5, 2))  # s (static), y (per row), k, z (per row), m
    la = ["s", "y", "k", "z", "m"]
    n_rows, row0 = 301, 37
    ld = row0 + n_rows + 13
    codes = np.full((2, ld), 251, dtype=np.uint8)  # outside the gathered rows: never read (out of range for both)
    codes[0, row0:row0 + n_rows] = rng.integers(0, 200, n_rows)
    codes[1, row0:row0 + n_rows] = rng.integers(0, 5, n_rows)
    codes[0, row0], codes[0, row0 + n_rows - 1] = 199, 0
    out_labels = ["k", "m"]
    out_labels.insert(row_pos, E.ROW)
    A = _dev(a)

    def ref_for(cd):
        y, z = cd[0, row0:row0 + n_rows].astype(int), cd[1, row0:row0 + n_rows].astype(int)
        r = a[2][y, :, z, :]  # [row, k, m]
        return np.moveaxis(r, 0, row_pos)

    ev = {"s": 2, "y": (None, 0), "z": (None, 1)}
    got = E.gather(A, la, ev, out_labels, codes=_dev(codes), ld=ld, row0=row0, n_rows=n_rows)
    np.testing.assert_array_equal(_host(got), ref_for(codes))
    # one out-of-range code: the error is raised, and the value read is index 0 of that axis
    bad = codes.copy()
    bad[1, row0 + 100] = 5
    with pytest.raises(IndexError):
        E.gather(A, la, ev, out_labels, codes=_dev(bad), ld=ld, row0=row0, n_rows=n_rows)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = E.gather(A, la, ev, out_labels, codes=_dev(bad), ld=ld, row0=row0, n_rows=n_rows, err=err)
    assert int(err.item()) == 1
    clamped = bad.copy()
    clamped[1, row0 + 100] = 0
    np.testing.assert_array_equal(_host(got), ref_for(clamped))


# ----------------------------------------------------------------------------- pgm_codes_select / remap
@pytest.mark.parametrize("n_cols", [1, 31, 33, 70])
@pytest.mark.parametrize("n_rows", [1, 257, 1000])
def test_codes_select(gpu, n_cols, n_rows):
    import torch

    N = _n()
    rng = np.random.default_rng(n_cols * 7 + n_rows)
    total_cols, row0 = 75, 11
    ld = row0 + n_rows + 5
    codes = rng.integers(0, 256, (total_cols, ld)).astype(np.uint8)
    cols = rng.permutation(total_cols)[:n_cols].astype(np.int32)
    out = torch.full((n_cols * n_rows + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    C, J = _dev(codes), _dev(cols)
    N.check(N.lib().pgm_codes_select(N.ptr(C), ld, row0, N.ptr(J), n_cols, n_rows, N.ptr(out), N.stream_handle()),
            "codes_select")
    got = _host(out)
    np.testing.assert_array_equal(got[:n_cols * n_rows].reshape(n_cols, n_rows), codes[cols, row0:row0 + n_rows])
    assert (got[n_cols * n_rows:] == 0xEE).all()


def _mix64(z):
    """The splitmix64 finaliser on a uint64 array (wrapping multiplication)."""
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


@pytest.mark.parametrize("n_cols", [1, 31, 33, 70])  # 1, 1, 2 and 4 column chunks per row block
@pytest.mark.parametrize("n_rows", [1, 257, 1000])
def test_codes_remap(gpu, n_cols, n_rows):
    """State codes, error flag, missing-pattern key / count and the 128-bit row hash against numpy, with
    padded leading dimensions; then without the hash and without the key."""
    import torch

    N = _n()
    rng = np.random.default_rng(n_cols * 13 + n_rows)
    lut_stride, ld_raw, ld_out = 16, n_rows + 9, n_rows + 6
    raw = rng.integers(0, 12, (n_cols, ld_raw)).astype(np.int8)
    raw[rng.random((n_cols, ld_raw)) < 0.15] = -1  # NaN
    lut = rng.integers(0, 9, (n_cols, lut_stride)).astype(np.uint8)
    col_key = rng.integers(1, 1 << 62, n_cols).astype(np.uint64)
    for with_bad in (False, True):
        r = raw.copy()
        if with_bad:
            r[n_cols - 1, n_rows - 1] = 16  # >= lut_stride: 254 and the error flag
            r[0, 0] = 100
        rr = r[:, :n_rows].astype(int)
        st = np.where(rr < 0, 255, np.where(rr >= lut_stride, 254,
                                            np.take_along_axis(lut, np.clip(rr, 0, lut_stride - 1), axis=1))).astype(np.uint8)
        miss = rr < 0
        key = np.bitwise_xor.reduce(np.where(miss, col_key[:, None], np.uint64(0)), axis=0)
        nmiss = miss.sum(axis=0).astype(np.uint32)
        x = (np.arange(n_cols, dtype=np.uint64)[:, None] << np.uint64(8)) | st.astype(np.uint64)
        h0 = np.bitwise_xor.reduce(_mix64(x ^ np.uint64(0x9E3779B97F4A7C15)), axis=0)
        h1 = np.bitwise_xor.reduce(_mix64(x ^ np.uint64(0xC2B2AE3D27D4EB4F)), axis=0)
        R, LUT, KEY = _dev(r), _dev(lut), _dev(col_key.view(np.int64))
        for use_key, use_hash in ((True, True), (True, False), (False, True)):
            out = torch.full((n_cols, ld_out), 0xEE, dtype=torch.uint8, device="cuda")
            rk = torch.zeros(n_rows, dtype=torch.int64, device="cuda")
            rn = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
            rh = torch.zeros(2 * n_rows, dtype=torch.int64, device="cuda")
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            N.check(N.lib().pgm_codes_remap(N.ptr(R), ld_raw, n_cols, n_rows, N.ptr(LUT), lut_stride, N.ptr(KEY),
                                            N.ptr(out), ld_out, N.ptr(rk) if use_key else None,
                                            N.ptr(rn) if use_key else None, N.ptr(rh) if use_hash else None,
                                            N.ptr(err), N.stream_handle()), "codes_remap")
            o = _host(out)
            np.testing.assert_array_equal(o[:, :n_rows], st)
            assert (o[:, n_rows:] == 0xEE).all()
            assert int(err.item()) == (1 if with_bad else 0)
            if use_key:
                np.testing.assert_array_equal(_host(rk).view(np.uint64), key)
                np.testing.assert_array_equal(_host(rn).view(np.uint32), nmiss)
            else:
                assert not _host(rk).any() and not _host(rn).any()
            if use_hash:
                h = _host(rh).view(np.uint64).reshape(n_rows, 2)
                np.testing.assert_array_equal(h[:, 0], h0)
                np.testing.assert_array_equal(h[:, 1], h1)
            else:
                assert not _host(rh).any()


# ----------------------------------------------------------------------------- pgm_product_n
def _prodn_operands(n_ops, n_outer, n_x, rng, ratio):
    """n_ops operands over the labels [o, x], cycling through full, row-only ([x]) and outer-only ([o])
    layouts; the RATIO / DEN pair (the last two) keeps away from 0."""
    ops = []
    for i in range(n_ops):
        labels = (["o", "x"], ["x"], ["o"])[i % 3] if n_outer > 1 else ["x"]
        shape = [n_outer if l == "o" else n_x for l in labels]
        v = rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)
        ops.append((v, labels))
    if ratio:  # the pair spans the row axis, where the special values go
        for i in (n_ops - 2, n_ops - 1):
            labels = ["o", "x"] if n_outer > 1 and i == n_ops - 2 else ["x"]
            shape = [n_outer if l == "o" else n_x for l in labels]
            ops[i] = (rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape), labels)
    return ops


def _prodn_ref(ops, kinds, n_outer, n_x, dtype):
    N = _n()
    full = [np.broadcast_to(v.astype(dtype).reshape([n_outer if "o" in ls else 1, n_x if "x" in ls else 1]),
                            (n_outer, n_x)) for v, ls in ops]
    prod = np.ones((n_outer, n_x), dtype=dtype)
    with np.errstate(all="ignore"):
        for i, k in enumerate(kinds):
            if k == N.PRODN_MUL:
                prod = prod * full[i]
            elif k == N.PRODN_RATIO:
                r = full[i] / full[i + 1]
                prod = prod * np.where(np.isnan(r), dtype(0.0), r)
    return prod


@pytest.mark.parametrize("n_ops", [1, 2, 5, 8])
@pytest.mark.parametrize("rows", [(1, 63), (3, 65), (3, 66), (5, 130), (1025, 1027)])
@pytest.mark.parametrize("values", ["finite", "special"])
def test_product_n_operand_counts_and_row_paths(gpu, n_ops, rows, values):
    """1, 2, 5 and 8 operands (kernel templates of 2, 4 and 8 slots), a RATIO / DEN pair in the last two slots
    of 2 and 8; flat (63 rows), row mode (65, odd), two rows per lane with a block below 256 lanes (66, 130)
    and more than one trip of the rows-in-flight loop (1027 rows, 1025 outer states: one block per state).
    Against the long-double product within (n_ops + 1) ulp."""
    E, N = _e(), _n()
    n_outer, n_x = rows
    ratio = n_ops in (2, 8)
    rng = np.random.default_rng(n_ops * 100 + n_x)
    ops = _prodn_operands(n_ops, n_outer, n_x, rng, ratio)
    kinds = [N.PRODN_MUL] * n_ops
    if ratio:
        kinds[-2:] = [N.PRODN_RATIO, N.PRODN_DEN]
        if values == "special":
            num, den = ops[-2][0].reshape(-1), ops[-1][0].reshape(-1)
            for j, (vn, vd) in enumerate([(np.nan, 1.0), (np.inf, 1.0), (-np.inf, -1.0), (-0.0, 1.0), (0.0, 0.0),
                                          (1.0, 0.0), (-1.0, 0.0), (1.0, np.nan), (np.inf, np.inf)]):
                for base in (0, n_x - 9):
                    num[base + j], den[base + j] = vn, vd
            # the ratio is the last factor of the left fold: one rounding into the subnormal range
            num[n_x // 2], den[n_x // 2] = DENORMAL, 1.0
    elif values == "special":  # no ratio operands: plain IEEE products
        v0 = ops[0][0].reshape(-1)
        v0[0], v0[-1], v0[v0.size // 2] = np.nan, np.inf, -0.0
    dev = [(_dev(v), ls) for v, ls in ops]
    got = _host(E.product_n(dev, ["o", "x"] if n_outer > 1 else ["x"], kinds=kinds)).reshape(n_outer, n_x)
    ref64 = _prodn_ref(ops, kinds, n_outer, n_x, np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref64))
    np.testing.assert_array_equal(np.isinf(got), np.isinf(ref64))
    fin = np.isfinite(ref64)
    np.testing.assert_array_equal(np.signbit(got[np.isinf(ref64)]), np.signbit(ref64[np.isinf(ref64)]))
    if HAVE_LD:
        ref = _prodn_ref(ops, kinds, n_outer, n_x, LD)
        err = np.abs(got[fin].astype(LD) - ref[fin])
        assert (err <= (n_ops + 1) * np.spacing(np.abs(ref64[fin]))).all()
    else:
        np.testing.assert_allclose(got[fin], ref64[fin], rtol=(n_ops + 1) * 2.0 ** -52, atol=0)
    if values == "special" and ratio:
        assert got[0, 0] == 0.0 and got[0, 4] == 0.0 and np.isinf(got[0, 5])  # NaN / x -> 0, 0 / 0 -> 0, x / 0 -> inf


@pytest.mark.parametrize("rows", [(1, 63), (3, 65), (3, 66), (1025, 1027)])
def test_product_n_two_mul_operands_exact(gpu, rows):
    E = _e()
    n_outer, n_x = rows
    rng = np.random.default_rng(n_x)
    a, b = rng.uniform(-1.0, 1.0, (n_outer, n_x)), rng.uniform(-1.0, 1.0, n_x)
    got = _host(E.product_n([(_dev(a), ["o", "x"]), (_dev(b), ["x"])], ["o", "x"]))
    np.testing.assert_array_equal(got, a * b)
