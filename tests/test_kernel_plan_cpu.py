"""The plan of every entry of tests/kernel_cases.py, checked on the host (pgm_contract_info: no device).

The GPU tests run these shapes for their values; this test proves which kernel and sub-mode each shape
takes, so a planner change that retires a path from the table fails here.
"""
import ctypes

import pytest

from tests import kernel_cases as K


def _info(c, **kw):
    from pgmpy_amd import engine as E

    a, k = K.info_args(c, **kw)
    return E.contract_info(*a, **k)


@pytest.mark.parametrize("name", [c["name"] for c in K.CASES])
def test_case_takes_its_path(name):
    c = K.BY_NAME[name]
    info = _info(c)
    got = {f: (tuple(info.grid) if f == "grid" else getattr(info, f)) for f in c["expect"]}
    assert got == c["expect"]


def test_table_covers_every_path():
    have = set()
    for c in K.CASES:
        have |= K.features(_info(c))
    missing = [r for r in K.REQUIRED if r not in have]
    assert not missing, missing
    # every path that has a GPU-runnable entry: the two plan-only entries add nothing of their own
    have_gpu = set()
    for c in K.CASES:
        if c["gpu"]:
            have_gpu |= K.features(_info(c))
    assert not [r for r in K.REQUIRED if r not in have_gpu]
    # a strided out= for the flat, rows, rows_tab and final kernels, transposed and padded
    strided = {(int(_info(c).kernel), _info(c).n_split > 1, c["out"]) for c in K.CASES if c["out"]}
    for kernel in (K.FLAT, K.ROWS, K.ROWS_TAB):
        assert (kernel, False, "pad") in strided and (kernel, False, "T") in strided, kernel
    assert (K.ROWS, True, "T") in strided and (K.ROWS, True, "pad") in strided and (K.FLAT, True, "pad") in strided


def test_alignment_decides_the_two_row_kernel():
    """ROWS_TAB2 needs 16-B aligned A and C; an address of 8 mod 16 on either side falls back to ROWS_TAB."""
    c = K.BY_NAME["rows_tab2_odd_grid"]
    assert _info(c).kernel == K.ROWS_TAB2
    assert tuple(_info(c).grid) == (2, 3, 1)  # 257 row pairs: ceil(3 / 2) blocks of 256 lanes
    assert _info(c, a_ptr=K.BASE_ADDR + 8).kernel == K.ROWS_TAB
    assert _info(c, c_ptr=K.BASE_ADDR + 8).kernel == K.ROWS_TAB
    assert tuple(_info(c, c_ptr=K.BASE_ADDR + 8).grid) == (3, 3, 1)


def test_info_matches_workspace_and_rejects_bad_descriptors():
    from pgmpy_amd import _native as N
    from pgmpy_amd import engine as E

    lib = N.load_library()
    for c in K.CASES:
        a, k = K.info_args(c)
        d, _ = E.contract_desc(*a, reduce=k["reduce"], combine=k["combine"], out_stride=k["out_stride"])
        info = N.ContractInfo()
        assert lib.pgm_contract_info(ctypes.byref(d), None, None, ctypes.byref(info)) == N.PGM_OK
        ws = ctypes.c_size_t(0)
        assert lib.pgm_contract_workspace(ctypes.byref(d), ctypes.byref(ws)) == N.PGM_OK
        assert ws.value == (8 * info.n_split * info.n_out if info.n_split > 1 else 0), c["name"]
        assert info.empty_splits < info.n_split
    d = N.ContractDesc()
    d.n_keep = 1
    d.keep_card[0] = 0
    assert lib.pgm_contract_info(ctypes.byref(d), None, None, ctypes.byref(N.ContractInfo())) == N.PGM_EINVAL
    d.keep_card[0] = 4
    assert lib.pgm_contract_info(ctypes.byref(d), None, None, None) == N.PGM_EINVAL
