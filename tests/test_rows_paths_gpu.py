"""Every entry of tests/rows_cases.py on the GPU, against the long-double reference of the same spec.

Each entry exists for one kernel path of the fused row plan; pgm_rows_launch_info (with the buffers' real
addresses) proves the launch takes it, and for the specialised kernels pgm_rows_bound_kernel must name the
kernel that was predicted.  Checked per entry: marginals, joint, MAP index, MAP gap and the error flag
against the reference (bounds: the module docstring of rows_cases.py), dead rows (NaN marginals / joint,
MAP 0, gap 0), out-of-range codes computed as state 0, and that nothing outside rows [0, n_rows) of any
output was written (the buffers are longer than needed and pre-filled with a sentinel).

Worst error / bound ratios seen on an MI355X are printed per entry (-s) and recorded in the commit that
added this file; they are measurements against the reference, not tolerances.
"""
import ctypes

import numpy as np
import pytest

from pgmpy_amd import _native as N
from tests import rows_cases as RC

pytestmark = pytest.mark.gpu

SENT = -12345.678
SENT_I = -77777
GUARD = 16  # elements kept free in front of and behind every output
_PLANS, _REFS = {}, {}
KERNEL_NAME = {RC.JIT: "pgm_rows_jit", RC.JIT2: "pgm_rows_jit2", RC.AFFINE: "", RC.TABLE: ""}


class _Plan:
    def __init__(self, spec):
        self.factors = RC.make_factors(spec)
        self.pl, self.values = RC.build_plan(spec, self.factors)
        self.h = ctypes.c_void_p()
        N.check(N.lib().pgm_rows_plan_create(ctypes.byref(self.pl), self.values.ctypes.data_as(ctypes.c_void_p),
                                             ctypes.byref(self.h)), "rows_plan_create")

    def __del__(self):
        if getattr(self, "h", None):
            N.load_library().pgm_rows_plan_destroy(self.h)


def plan_of(spec):
    if spec["plan"] not in _PLANS:
        _PLANS[spec["plan"]] = _Plan(spec)
    return _PLANS[spec["plan"]]


def ref_of(spec, plan):
    """codes and reference of a case, shared by the cases that differ in mode bits only."""
    key = (spec["plan"], spec["n_rows"], spec["row0"], spec["ld_codes"], spec["oob"])
    if key not in _REFS:
        for k in [k for k in _REFS if k[1] > 100_000]:  # the large cases come in adjacent pairs: keep one
            del _REFS[k]
        codes = RC.make_codes(spec)
        r0 = spec["row0"]
        _REFS[key] = (codes, RC.reference(spec, plan.factors, codes[:, r0:r0 + spec["n_rows"]]))
    return _REFS[key]


def _buf(n, off, dtype, dev, fill):
    """A sentinel-filled buffer with GUARD elements around n payload elements starting `off` bytes past a
    16-B aligned address; returns (whole tensor, payload view)."""
    import torch

    k = off // np.dtype(dtype).itemsize
    whole = torch.full((GUARD + k + n + GUARD,), fill, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
    assert whole.data_ptr() % 16 == 0 and GUARD * np.dtype(dtype).itemsize % 16 == 0
    return whole, whole[GUARD + k:GUARD + k + n]


def _rel_check(got, ref, c, what, worst):
    """|got - ref| <= c u ref elementwise (ref >= 0 finite); returns nothing, records the worst ratio."""
    got = got.astype(RC.LD)
    err = np.abs(got - ref)
    bound = c * RC.LD(RC.U) * ref
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), float((err / np.where(bound > 0, bound, 1))[bad].max()))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)
    worst[what] = max(worst.get(what, 0.0), float(ratio.max()) if ratio.size else 0.0)


def check_outputs(spec, ref, marg, joint, mp, gap, n_marg, n_joint, worst):
    """Outputs (host arrays shaped [n_marg, ld_out], [n_joint, ld_out], [n], [n]; None if not asked) against
    the reference."""
    n = spec["n_rows"]
    dead, live = ref["dead"], ~ref["dead"]
    exact = spec["family"] == "exact"
    if marg is not None:
        assert np.isnan(marg[:, :n][:, dead]).all()
        c = np.full(n_marg, 2 + RC.U) if exact else ref["mcoef"]
        _rel_check(marg[:, :n][:, live], ref["marg"][:, live], c[:, None], "marg", worst)
    if joint is not None:
        assert np.isnan(joint[:, :n][:, dead]).all()
        c = (2 + RC.U) if exact else RC.coef(spec["comps"][0])
        _rel_check(joint[:, :n][:, live], ref["joint"][:, live], c, "joint", worst)
    if mp is not None:
        assert (mp[dead] == 0).all()
        sel = live & ~ref["near"]
        np.testing.assert_array_equal(mp[sel], ref["map"][sel])
    if gap is not None:
        assert (gap[dead] == 0).all()
        if exact:
            np.testing.assert_array_equal(gap[live], ref["gap"][live].astype(np.float64))
        else:
            err = np.abs(gap[live].astype(RC.LD) - ref["gap"][live])
            bound = ref["gcoef"] * RC.U
            assert (err <= bound).all(), float(err.max() / bound)
            worst["gap"] = max(worst.get("gap", 0.0), float(err.max() / bound) if err.size else 0.0)


@pytest.mark.parametrize("spec", RC.CASES, ids=lambda s: s["name"])
def test_rows_case(gpu, spec):
    import torch

    if not spec["jit"]:  # the choice without hipRTC is a host-side fact; on the device hipRTC is there
        plan = plan_of(spec)
        assert RC.launch_info(spec, plan.pl).kernel == spec["expect"]["kernel"]
        return
    L = N.lib()
    plan = plan_of(spec)
    pl = plan.pl
    codes, ref = ref_of(spec, plan)
    n, ld_out, mode, mis = spec["n_rows"], spec["ld_out"], spec["mode"], spec["mis"]
    n_marg, n_joint = pl.n_marg, pl.n_joint
    cw, cv = _buf(codes.size, mis.get("codes", 0), np.uint8, gpu, RC.OOB)
    cv.copy_(torch.from_numpy(codes.reshape(-1)))
    bufs = {}
    if mode & RC.MARG:
        bufs["marg"] = _buf(n_marg * ld_out, mis.get("marg", 0), np.float64, gpu, SENT)
    if mode & RC.JOINT:
        bufs["joint"] = _buf(n_joint * ld_out, mis.get("joint", 0), np.float64, gpu, SENT)
    if mode & (RC.MAP | RC.GAP):
        bufs["map"] = _buf(n, mis.get("map", 0), np.int32, gpu, SENT_I)
    if mode & RC.GAP:
        bufs["gap"] = _buf(n, mis.get("gap", 0), np.float64, gpu, SENT)
    err = torch.zeros(1 + 2 * GUARD, dtype=torch.int32, device=gpu)
    addr = {k: v[1].data_ptr() for k, v in bufs.items()}
    addr["codes"] = cv.data_ptr()
    info = RC.launch_info(spec, pl, addr)
    want = spec["expect"]
    got = {k: getattr(info, k) for k in want}
    assert got == want, got
    P = ctypes.c_void_p
    a = lambda k: P(addr[k]) if k in addr else None
    bound = P()
    N.check(L.pgm_rows_plan_bind(plan.h, mode, a("codes"), spec["ld_codes"], spec["row0"], n, a("marg"), a("joint"),
                                 ld_out, a("map"), a("gap"), P(err[GUARD:].data_ptr()), N.stream_handle(),
                                 ctypes.byref(bound)), "rows_plan_bind")
    try:
        name = ctypes.create_string_buffer(64)
        nb, wg = ctypes.c_uint32(), ctypes.c_uint32()
        N.check(L.pgm_rows_bound_kernel(bound, name, 64, ctypes.byref(nb), ctypes.byref(wg)), "rows_bound_kernel")
        assert name.value.decode() == KERNEL_NAME[info.kernel]
        if info.kernel in (RC.JIT, RC.JIT2):
            assert (nb.value, wg.value) == (info.blocks, info.wg)
        N.check(L.pgm_rows_bound_run(bound), "rows_bound_run")
        torch.cuda.synchronize()
    finally:
        L.pgm_rows_bound_destroy(bound)
    host = {k: v[0].cpu().numpy() for k, v in bufs.items()}
    e = err.cpu().numpy()
    assert e[GUARD] == ref["err"] and (np.delete(e, GUARD) == 0).all()
    assert (cw.cpu().numpy()[GUARD + mis.get("codes", 0):][:codes.size] == codes.reshape(-1)).all()
    out = {}
    for k, rows, ld, sent in (("marg", n_marg, ld_out, SENT), ("joint", n_joint, ld_out, SENT), ("map", 1, n, SENT_I),
                              ("gap", 1, n, SENT)):
        if k not in host:
            out[k] = None
            continue
        w = host[k]
        k0 = GUARD + mis.get(k, 0) // w.dtype.itemsize
        # nothing outside rows [0, n) of each output row was written
        assert (w[:k0] == sent).all() and (w[k0 + rows * ld:] == sent).all(), k
        m = w[k0:k0 + rows * ld].reshape(rows, ld)
        assert (m[:, n:] == sent).all(), k
        assert not (m[:, :n] == sent).any(), k  # and every row inside was
        out[k] = m if rows > 1 or k in ("marg", "joint") else m[0]
    worst = {}
    check_outputs(spec, ref, out["marg"], out["joint"], out["map"], out["gap"] if mode & RC.GAP else None, n_marg,
                  n_joint, worst)
    near = int(ref["near"].sum())
    print(f"\n[rows_case] {spec['name']} family={spec['family']} rows={n} distinct={ref['distinct']} "
          f"dead={int(ref['dead'].sum())} map_skipped={near} worst/bound=" +
          " ".join(f"{k}:{v:.3f}" for k, v in sorted(worst.items())))


def test_ring_batches_against_reference(gpu):
    """pgm_rows_ring_* on an exact-family two-component plan: 130 rows per batch (two 128-row chunks, the
    second with 2 live rows), 3 slots, 5 batches, each with its own evidence; every batch is checked
    against the reference as soon as its launch finished (start / post / finish, a slot refilled only
    after the launch that ran it)."""
    import torch

    L = N.lib()
    spec = RC.RING
    plan = plan_of(spec)
    pl = plan.pl
    n, S, B = spec["n_rows"], RC.RING_SLOTS, RC.RING_BATCHES
    mode = spec["mode"]
    batches = []
    for b in range(B):
        sb = dict(spec, seed=spec["seed"] + 7 * b, oob=(1, 129) if b == 3 else ())
        codes = RC.make_codes(sb)
        batches.append((sb, codes, RC.reference(sb, plan.factors, codes)))
    n_cols = batches[0][1].shape[0]
    slots = []
    for s in range(S):
        slots.append(dict(codes=_buf(n_cols * n, 0, np.uint8, gpu, RC.OOB), marg=_buf(pl.n_marg * n, 0, np.float64, gpu, SENT),
                          map=_buf(n, 0, np.int32, gpu, SENT_I), gap=_buf(n, 0, np.float64, gpu, SENT)))
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    P = ctypes.c_void_p
    arr = lambda k: (P * S)(*[sl[k][1].data_ptr() for sl in slots])
    lds = (ctypes.c_int64 * S)(*[n] * S)
    row0 = (ctypes.c_int64 * S)(*[0] * S)
    ring = P()
    N.check(L.pgm_rows_ring_create(plan.h, mode, S, arr("codes"), lds, row0, n, arr("marg"), n, arr("map"), arr("gap"),
                                   P(err.data_ptr()), N.stream_handle(), ctypes.byref(ring)), "rows_ring_create")
    try:
        done = 0
        for first in range(0, B, S):  # one launch per round of slots: a slot is refilled after finish()
            cnt = min(S, B - first)
            for i in range(cnt):
                sl = slots[i]
                for k, fill in (("marg", SENT), ("map", SENT_I), ("gap", SENT)):
                    sl[k][0].fill_(fill)
                sl["codes"][1].copy_(torch.from_numpy(batches[first + i][1].reshape(-1)))
            err.zero_()
            torch.cuda.synchronize()
            N.check(L.pgm_rows_ring_start(ring, cnt, 5.0), "rows_ring_start")
            for i in range(1, cnt + 1):
                N.check(L.pgm_rows_ring_post(ring, i), "rows_ring_post")
            N.check(L.pgm_rows_ring_finish(ring), "rows_ring_finish")
            torch.cuda.synchronize()
            want_err = 0
            for i in range(cnt):
                sb, _, ref = batches[first + i]
                want_err |= ref["err"]
                sl = slots[i]
                host = {k: sl[k][0].cpu().numpy() for k in ("marg", "map", "gap")}
                for k, sent in (("marg", SENT), ("map", SENT_I), ("gap", SENT)):
                    assert (host[k][:GUARD] == sent).all() and (host[k][-GUARD:] == sent).all(), (first + i, k)
                    assert not (host[k][GUARD:-GUARD] == sent).any(), (first + i, k)
                check_outputs(sb, ref, host["marg"][GUARD:-GUARD].reshape(pl.n_marg, n), None, host["map"][GUARD:-GUARD],
                              host["gap"][GUARD:-GUARD], pl.n_marg, pl.n_joint, {})
                done += 1
            assert int(err.item()) == want_err
        assert done == B
    finally:
        L.pgm_rows_ring_destroy(ring)
