"""ctypes binding of the C-ABI in include/pgmhip.h (libpgmhip.so, gfx950).

This is the seam where pgmpy's numpy/torch dispatch (pgmpy/utils/compat_fns.py:
einsum L63-67, max L53-60, argmax L70-74) is replaced by hand-written HIP
kernels.  There is no CPU fallback: every compute entry point raises
``NativeUnavailable`` when the library or a GPU is missing, so a silent numpy
path can never stand in for the device path.

Device buffers are torch tensors (PyTorch is plumbing here: allocator, streams,
torch.distributed); only raw pointers and the HIP stream handle cross the ABI.
"""
import ctypes
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PGM_LIB_PATH") or os.path.join(HERE, "lib", "libpgmhip.so")  # override: tools only

PGM_OK = 0
PGM_EINVAL = -1
PGM_EINDEX = -2
PGM_ENOMEM = -3
PGM_EDEVICE = -4
PGM_MAX_DIMS = 32
PGM_EV_MISSING = 255

COMBINE_MUL, COMBINE_ADD, COMBINE_DIV, COMBINE_COPY, COMBINE_DIV_RAW = 0, 1, 2, 3, 4
RED_NONE, RED_SUM, RED_MAX = 0, 1, 2

ROWS_MAX_LOOP = 12
ROWS_MAX_FAC = 16
ROWS_MAX_EV = 48
ROWS_MAX_COMP = 12
ROWS_MAX_MARG = 192
ROWS_MARGINALS, ROWS_JOINT, ROWS_MAP, ROWS_MAPGAP, ROWS_VALUES_GLOBAL = 1, 2, 4, 8, 16
BATCH_GRID, BATCH_ONE_WORKGROUP = 0, 1  # pgm_batch_set_mode
ROWS_ONE_GROUP, ROWS_GENERIC, ROWS_NO_JIT, ROWS_FLOOR = 32, 64, 128, 256


class NativeUnavailable(RuntimeError):
    """The gfx950 HIP library (or a GPU) is not available: there is no CPU fallback."""


_I64 = ctypes.c_int64 * PGM_MAX_DIMS


class ContractDesc(ctypes.Structure):
    _fields_ = [
        ("combine", ctypes.c_int32),
        ("reduce", ctypes.c_int32),
        ("n_keep", ctypes.c_int32),
        ("n_red", ctypes.c_int32),
        ("keep_card", _I64),
        ("keep_sa", _I64),
        ("keep_sb", _I64),
        ("keep_sc", _I64),
        ("red_card", _I64),
        ("red_sa", _I64),
        ("red_sb", _I64),
    ]


CK_FLAT, CK_ROWS, CK_ROWS_TAB, CK_ROWS_TAB2 = 0, 1, 2, 3  # enum pgm_contract_kernel
CK_NAMES = ("FLAT", "ROWS", "ROWS_TAB", "ROWS_TAB2")


class ContractInfo(ctypes.Structure):
    """pgm_contract_info_t: the kernel and plan pgm_contract would run (host-only query)."""
    _fields_ = [
        ("kernel", ctypes.c_int32),
        ("g_log2", ctypes.c_int32),
        ("n_split", ctypes.c_uint32),
        ("red_chunk", ctypes.c_uint32),
        ("ri_nb", ctypes.c_uint32),
        ("ri_chunk", ctypes.c_uint32),
        ("grid", ctypes.c_uint32 * 3),
        ("n_ro", ctypes.c_uint32),
        ("n_v", ctypes.c_uint32),
        ("n_out", ctypes.c_uint32),
        ("n_red", ctypes.c_uint32),
        ("ri_card", ctypes.c_uint32),
        ("nx", ctypes.c_uint32),
        ("unrolled", ctypes.c_uint32),
        ("empty_splits", ctypes.c_uint32),
    ]


PRODN_MAX_OPS = 8
PM_MAX_OPS = 8  # operands of a fused product + marginal step (pgm_internal.h MOPS)


PRODN_MUL, PRODN_RATIO, PRODN_DEN, PRODN_MDIV = 0, 1, 2, 3


class ProductNDesc(ctypes.Structure):
    _fields_ = [
        ("n_ops", ctypes.c_int32),
        ("n_keep", ctypes.c_int32),
        ("op_kind", ctypes.c_int32 * PRODN_MAX_OPS),
        ("keep_card", _I64),
        ("keep_sc", _I64),
        ("keep_s", _I64 * PRODN_MAX_OPS),
    ]


class ContractNDesc(ctypes.Structure):
    """pgm_contractn_desc (r06): C[keep] = reduce over red of prod_t X_t."""
    _fields_ = [
        ("n_ops", ctypes.c_int32),
        ("reduce", ctypes.c_int32),
        ("n_keep", ctypes.c_int32),
        ("n_red", ctypes.c_int32),
        ("keep_card", _I64),
        ("keep_sc", _I64),
        ("keep_s", _I64 * PRODN_MAX_OPS),
        ("red_card", _I64),
        ("red_s", _I64 * PRODN_MAX_OPS),
    ]


class ContractNInfo(ctypes.Structure):
    """pgm_contractn_info_t: the plan pgm_batch_add_contract_n makes for a descriptor (host-only query)."""
    _fields_ = [
        ("nk", ctypes.c_int32),
        ("nr", ctypes.c_int32),
        ("g_log2", ctypes.c_int32),
        ("blocks", ctypes.c_uint32),
        ("n_out", ctypes.c_uint32),
        ("n_red", ctypes.c_uint32),
        ("kcard", ctypes.c_uint32 * PGM_MAX_DIMS),
        ("rcard", ctypes.c_uint32 * PGM_MAX_DIMS),
    ]


class GemmDesc(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int64), ("m", ctypes.c_int64), ("n", ctypes.c_int64), ("k", ctypes.c_int64),
                ("offsets", ctypes.c_void_p), ("stride", ctypes.c_int64 * 9), ("lane_order", ctypes.c_int32),
                ("_pad", ctypes.c_int32)]


class GatherDesc(ctypes.Structure):
    _fields_ = [
        ("n_keep", ctypes.c_int32),
        ("n_ev", ctypes.c_int32),
        ("batch_dim", ctypes.c_int32),
        ("_pad", ctypes.c_int32),
        ("ld", ctypes.c_int64),
        ("row0", ctypes.c_int64),
        ("keep_card", _I64),
        ("keep_sa", _I64),
        ("keep_sc", _I64),
        ("ev_col", _I64),
        ("ev_stride", _I64),
        ("ev_card", _I64),
    ]


class RowsPlan(ctypes.Structure):
    _fields_ = [
        ("n_loop", ctypes.c_int32),
        ("n_query", ctypes.c_int32),
        ("n_fac", ctypes.c_int32),
        ("n_ev", ctypes.c_int32),
        ("n_values", ctypes.c_int32),
        ("n_comp", ctypes.c_int32),
        ("n_marg", ctypes.c_int32),
        ("n_joint", ctypes.c_int32),
        ("loop_card", ctypes.c_int32 * ROWS_MAX_LOOP),
        ("loop_marg_off", ctypes.c_int32 * ROWS_MAX_LOOP),
        ("loop_map_stride", ctypes.c_int32 * ROWS_MAX_LOOP),
        ("comp_loop_begin", ctypes.c_int32 * ROWS_MAX_COMP),
        ("comp_n_query", ctypes.c_int32 * ROWS_MAX_COMP),
        ("comp_loop_end", ctypes.c_int32 * ROWS_MAX_COMP),
        ("comp_fac_begin", ctypes.c_int32 * ROWS_MAX_COMP),
        ("comp_fac_end", ctypes.c_int32 * ROWS_MAX_COMP),
        ("fac_base", ctypes.c_int32 * ROWS_MAX_FAC),
        ("fac_stride", (ctypes.c_int32 * ROWS_MAX_LOOP) * ROWS_MAX_FAC),
        ("fac_ev_begin", ctypes.c_int32 * ROWS_MAX_FAC),
        ("fac_ev_end", ctypes.c_int32 * ROWS_MAX_FAC),
        ("ev_col", ctypes.c_int32 * ROWS_MAX_EV),
        ("ev_stride", ctypes.c_int32 * ROWS_MAX_EV),
        ("ev_card", ctypes.c_int32 * ROWS_MAX_EV),
    ]


class FitFamily(ctypes.Structure):
    """pgm_fit_family: the code column and cardinality of a node, then of each of its parents."""
    _fields_ = [("n_vars", ctypes.c_int32), ("col", ctypes.c_int32 * PGM_MAX_DIMS),
                ("card", ctypes.c_int32 * PGM_MAX_DIMS)]


class FitInfo(ctypes.Structure):
    """pgm_fit_info_t: layout and launch geometry of a pgm_fit plan (host-only query)."""
    _fields_ = [("n_families", ctypes.c_int32), ("n_groups", ctypes.c_int32), ("tile_bins", ctypes.c_int32),
                ("rows_per_block", ctypes.c_int32), ("n_cols", ctypes.c_int32), ("block", ctypes.c_int32),
                ("total_bins", ctypes.c_int64), ("total_columns", ctypes.c_int64)]


FIT_MLE, FIT_BAYES, FIT_WEIGHTED = 0, 1, 2
SCORE_BD, SCORE_LL, SCORE_SKIP_EMPTY = 0, 1, 2
SCORE_CHUNK = 128  # PGM_SCORE_CHUNK
CI_YATES = 1  # PGM_CI_YATES
CI_CHUNK = 128  # PGM_CI_CHUNK
EM_MAX_LATENT, EM_MAX_CONFIGS, EM_MAX_FAMILIES, EM_FLOOR = 8, 4096, 32, 1e-10  # PGM_EM_*


class EmInfo(ctypes.Structure):
    """pgm_em_info_t: the latent side and launch geometry of a pgm_fit_estep call (host-only query)."""
    _fields_ = [("n_latent", ctypes.c_int32), ("n_configs", ctypes.c_int32), ("n_latent_families", ctypes.c_int32),
                ("n_plain_families", ctypes.c_int32), ("block", ctypes.c_int32), ("rows_per_block", ctypes.c_int32),
                ("lds_bytes", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class LogpInfo(ctypes.Structure):
    """pgm_logp_info_t: launch geometry and kernel path of a pgm_fit_logprob call (host-only query)."""
    _fields_ = [("block", ctypes.c_int32), ("rows_per_block", ctypes.c_int32), ("vec4", ctypes.c_int32),
                ("n_families", ctypes.c_int32), ("n_partials", ctypes.c_int64)]


LOGP_BLOCK, LOGP_ROWS_PER_BLOCK, LOGP_MAX_BLOCKS = 256, 1024, 65536  # PGM_LOGP_*


class SampleInfo(ctypes.Structure):
    """pgm_sample_info_t: layout, launch geometry and kernel path of a pgm_sample plan (host-only query)."""
    _fields_ = [("n_families", ctypes.c_int32), ("n_cols", ctypes.c_int32), ("block", ctypes.c_int32),
                ("rows_per_block", ctypes.c_int32), ("total_bins", ctypes.c_int64), ("total_columns", ctypes.c_int64),
                ("vec4", ctypes.c_int32), ("weighted", ctypes.c_int32), ("explicit_uniforms", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


SAMPLE_FREE, SAMPLE_GIVEN, SAMPLE_OBSERVED = 0, 1, 2


class LwInfo(ctypes.Structure):
    """pgm_lw_info_t: launch geometry, fixed-point exponent and LDS of a pgm_sample_posterior call (host-only
    query)."""
    _fields_ = [("block", ctypes.c_int32), ("chunk", ctypes.c_int32), ("k", ctypes.c_int32),
                ("lds_bytes", ctypes.c_int32), ("lds_budget", ctypes.c_int32), ("n_cols", ctypes.c_int32),
                ("total_bins", ctypes.c_int64), ("chunks_per_row", ctypes.c_int64), ("workgroups", ctypes.c_int64),
                ("rows_per_launch", ctypes.c_int64)]


LW_CHUNK, LW_MAX_SAMPLES, LW_LDS_BUDGET, LW_MAX_GROUPS = 1024, 1 << 20, 163840, 65536  # PGM_LW_*


class GibbsInfo(ctypes.Structure):
    """pgm_gibbs_info_t: layout, launch geometry and kernel path of a pgm_gibbs plan (host-only query)."""
    _fields_ = [("n_factors", ctypes.c_int32), ("n_cols", ctypes.c_int32), ("total_entries", ctypes.c_int64),
                ("total_incidences", ctypes.c_int64), ("blocks", ctypes.c_int64), ("max_degree", ctypes.c_int32),
                ("max_card", ctypes.c_int32), ("path", ctypes.c_int32), ("block", ctypes.c_int32),
                ("lds_bytes", ctypes.c_int32), ("lds_budget", ctypes.c_int32), ("reg_card", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


GIBBS_LDS, GIBBS_GLOBAL = 0, 1  # PGM_GIBBS_*


class PairInfo(ctypes.Structure):
    """pgm_pair_info_t: the state layout and launch lists of a pgm_pair plan (host-only query)."""
    _fields_ = [("n_vars", ctypes.c_int32), ("n_cols", ctypes.c_int32), ("S", ctypes.c_int64), ("Sp", ctypes.c_int64),
                ("table_size", ctypes.c_int64), ("n_pairs", ctypes.c_int64), ("n_tile_pairs", ctypes.c_int64),
                ("n_groups", ctypes.c_int64), ("n_state_entries", ctypes.c_int64), ("slice_rows", ctypes.c_int64)]


PAIR_STAT_BLOCK, PAIR_MAX_CARD = 64, 254  # PGM_PAIR_STAT_BLOCK; the largest cardinality of a pair plan


class LgGramInfo(ctypes.Structure):
    """pgm_lg_gram_info_t: the tile layout and launch lists of a pgm_lg_gram plan (host-only query)."""
    _fields_ = [("d", ctypes.c_int32), ("n_cols", ctypes.c_int32), ("n_tiles", ctypes.c_int32), ("n_super", ctypes.c_int32),
                ("single_wave", ctypes.c_int32), ("reserved", ctypes.c_int32), ("n_groups", ctypes.c_int64),
                ("n_tile_pairs", ctypes.c_int64), ("out_size", ctypes.c_int64), ("max_slices", ctypes.c_int64),
                ("slice_rows", ctypes.c_int64)]


class LgNetInfo(ctypes.Structure):
    """pgm_lg_net_info_t: the families of a pgm_lg_net plan (host-only query)."""
    _fields_ = [("n_families", ctypes.c_int32), ("n_cols", ctypes.c_int32), ("max_parents", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("n_coef", ctypes.c_int64)]


# PGM_LG_*: the geometry of the linear-Gaussian kernels
LG_TILE, LG_SUPER, LG_ROWS_PER_LANE, LG_STEP = 16, 4, 4, 16
LG_TARGET_BLOCKS, LG_SLICE_MIN = 1024, 1024
LG_COLSUM_CHUNK, LG_COLSUM_MAX_CHUNKS = 4096, 1024
LG_MAX_PARENTS, LG_BLOCK, LG_MAX_BLOCKS, LG_AFFINE_CHUNK = 4096, 256, 65536, 256


class LgsInfo(ctypes.Structure):
    """pgm_lgs_info_t: the buckets of a pgm_lgs job batch (host-only query)."""
    _fields_ = [("n_jobs", ctypes.c_int32), ("d", ctypes.c_int32), ("n_buckets", ctypes.c_int32), ("max_cond", ctypes.c_int32),
                ("n_lane_jobs", ctypes.c_int64), ("n_wave_jobs", ctypes.c_int64), ("wave_lds_bytes", ctypes.c_int64)]


# PGM_LGS_*: the limits and score kinds of the Gaussian structure learning calls
LGS_MAX_COND, LGS_LANE_MAX, LGS_MAX_TARGETS = 64, 7, 3
LGS_LL, LGS_BIC, LGS_AIC = 0, 1, 2


class DbnInfo(ctypes.Structure):
    """pgm_dbn_info_t: the state spaces and launch geometry of a pgm_dbn plan (host-only query)."""
    _fields_ = [("n", ctypes.c_int32), ("n_free", ctypes.c_int32), ("n_configs", ctypes.c_int32),
                ("n_interface", ctypes.c_int32), ("n_prev_families", ctypes.c_int32), ("n_cur_families", ctypes.c_int32),
                ("seq_per_wave", ctypes.c_int32), ("block", ctypes.c_int32), ("n_query", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("lds_bytes", ctypes.c_int64), ("values0", ctypes.c_int64),
                ("values1", ctypes.c_int64), ("scratch_per_slice", ctypes.c_int64)]


DBN_MAX_CONFIGS, DBN_MAX_NODES, DBN_MAX_SLICES = 4096, 255, 65535  # PGM_DBN_MAX_CONFIGS and the plan's other limits


class DbnEstepInfo(ctypes.Structure):
    """pgm_dbn_estep_info_t: the accumulation path and launch geometry of pgm_dbn_estep (host-only query)."""
    _fields_ = [("path", ctypes.c_int32), ("tile_fits", ctypes.c_int32), ("blocks_per_cu", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("lds_bytes", ctypes.c_int64), ("tile_bytes", ctypes.c_int64),
                ("max_blocks", ctypes.c_int64)]


DBN_ESTEP_TILE, DBN_ESTEP_DIRECT = 0, 1  # PGM_DBN_ESTEP_*: the path of an info; DIRECT is also the flag that forces it
DBN_LDS_MAX = 163840  # the LDS a workgroup of the dynamic-network kernels may take

_P = ctypes.c_void_p
RK_NONE, RK_JIT, RK_JIT2, RK_AFFINE, RK_TABLE = -1, 0, 1, 2, 3  # enum pgm_rows_kernel
RK_NAMES = {RK_NONE: "NONE", RK_JIT: "JIT", RK_JIT2: "JIT2", RK_AFFINE: "AFFINE", RK_TABLE: "TABLE"}


class RowsLaunchInfo(ctypes.Structure):
    """pgm_rows_launch_info_t: the kernel and launch pgm_rows_plan_run would make (host-only query)."""
    _fields_ = [
        ("kernel", ctypes.c_int32),
        ("values_lds", ctypes.c_int32),
        ("acc_lds", ctypes.c_int32),
        ("maxfc", ctypes.c_int32),
        ("maxt", ctypes.c_int32),
        ("nf", ctypes.c_int32),
        ("nt", ctypes.c_int32),
        ("map", ctypes.c_int32),
        ("rg", ctypes.c_int32),
        ("blocks", ctypes.c_uint32),
        ("wg", ctypes.c_uint32),
        ("lds_bytes", ctypes.c_uint32),
    ]


def rows_launch_info(plan, mode, n_rows, row0=0, ld_codes=None, ld_out=None, codes=64, marg=64, joint=64, map_=64,
                     gap=64, jit=True):
    """RowsLaunchInfo of a pgm_rows_plan for a launch (pgm_rows_launch_info; no device).  The pointers
    are addresses (ints or None): only NULL and alignment matter."""
    info = RowsLaunchInfo()
    ld_codes = row0 + n_rows if ld_codes is None else ld_codes
    ld_out = n_rows if ld_out is None else ld_out
    P = ctypes.c_void_p
    check(load_library().pgm_rows_launch_info(ctypes.byref(plan), int(mode), P(codes), int(ld_codes), int(row0),
                                              int(n_rows), P(marg), P(joint), int(ld_out), P(map_), P(gap),
                                              1 if jit else 0, ctypes.byref(info)), "rows_launch_info")
    return info


_SIGS = {
    "pgm_version": ([], ctypes.c_int),
    "pgm_last_error": ([ctypes.c_char_p, ctypes.c_size_t], ctypes.c_int),
    "pgm_device_count": ([ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
    "pgm_set_device": ([ctypes.c_int], ctypes.c_int),
    "pgm_alloc": ([ctypes.POINTER(_P), ctypes.c_size_t], ctypes.c_int),
    "pgm_free": ([_P], ctypes.c_int),
    "pgm_memcpy_h2d": ([_P, _P, ctypes.c_size_t, _P], ctypes.c_int),
    "pgm_memcpy_d2h": ([_P, _P, ctypes.c_size_t, _P], ctypes.c_int),
    "pgm_memcpy_d2h_async": ([_P, _P, ctypes.c_size_t, _P], ctypes.c_int),
    "pgm_memcpy_d2d": ([_P, _P, ctypes.c_size_t, _P], ctypes.c_int),
    "pgm_memset": ([_P, ctypes.c_int, ctypes.c_size_t, _P], ctypes.c_int),
    "pgm_host_alloc": ([ctypes.POINTER(_P), ctypes.c_size_t], ctypes.c_int),
    "pgm_host_free": ([_P], ctypes.c_int),
    "pgm_stream_sync_spin": ([_P], ctypes.c_int),
    "pgm_stream_sync": ([_P], ctypes.c_int),
    "pgm_event_create": ([ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_event_destroy": ([_P], ctypes.c_int),
    "pgm_event_record": ([_P, _P], ctypes.c_int),
    "pgm_event_elapsed_ms": ([_P, _P, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
    "pgm_contract_workspace": ([ctypes.POINTER(ContractDesc), ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "pgm_contract": ([ctypes.POINTER(ContractDesc), _P, _P, _P, _P, ctypes.c_size_t, _P], ctypes.c_int),
    "pgm_contract_info": ([ctypes.POINTER(ContractDesc), _P, _P, ctypes.POINTER(ContractInfo)], ctypes.c_int),
    "pgm_product_n": ([ctypes.POINTER(ProductNDesc), ctypes.POINTER(_P), _P, _P], ctypes.c_int),
    "pgm_product_n_marginal_ok": ([ctypes.POINTER(ProductNDesc), ctypes.POINTER(_P), _P,
                                   ctypes.POINTER(ctypes.c_int64), _P], ctypes.c_int),
    "pgm_product_n_marginal": ([ctypes.POINTER(ProductNDesc), ctypes.POINTER(_P), _P,
                                ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, _P, _P], ctypes.c_int),
    "pgm_product_n_marginal_bind": ([ctypes.POINTER(ProductNDesc), ctypes.POINTER(_P), _P,
                                     ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, _P, ctypes.POINTER(_P)],
                                    ctypes.c_int),
    "pgm_product_n_marginal_source": ([ctypes.POINTER(ProductNDesc), ctypes.POINTER(_P), _P,
                                       ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, _P, ctypes.c_char_p,
                                       ctypes.c_size_t], ctypes.c_int),
    "pgm_product_n_marginals_bind": ([ctypes.POINTER(ProductNDesc), ctypes.POINTER(_P),
                                      ctypes.POINTER(ctypes.c_int64), _P, ctypes.POINTER(ctypes.c_int64), _P,
                                      ctypes.c_int32, ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_product_n_bind": ([ctypes.POINTER(ProductNDesc), ctypes.POINTER(_P), _P, ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_pm_bound_run": ([_P, _P], ctypes.c_int),
    "pgm_pm_merge": ([ctypes.POINTER(_P), ctypes.c_int32, ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_pm_prepare": ([ctypes.POINTER(_P), ctypes.c_int32], ctypes.c_int),
    "pgm_pm_bound_source": ([_P, ctypes.c_char_p, ctypes.c_size_t], ctypes.c_int),
    "pgm_pm_bound_destroy": ([_P], ctypes.c_int),
    "pgm_gemm": ([ctypes.POINTER(GemmDesc), _P, _P, _P, _P], ctypes.c_int),
    "pgm_batch_create": ([ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_batch_add_contract": ([_P, ctypes.POINTER(ContractDesc), _P, _P, _P], ctypes.c_int),
    "pgm_batch_add_gather": ([_P, ctypes.POINTER(GatherDesc), _P, _P, _P, _P], ctypes.c_int),
    "pgm_batch_add_product_n": ([_P, ctypes.POINTER(ProductNDesc), ctypes.POINTER(_P), _P], ctypes.c_int),
    "pgm_contract_n_info": ([ctypes.POINTER(ContractNDesc), ctypes.POINTER(_P), ctypes.POINTER(ContractNInfo)], ctypes.c_int),
    "pgm_batch_add_contract_n": ([_P, ctypes.POINTER(ContractNDesc), ctypes.POINTER(_P), _P], ctypes.c_int),
    "pgm_batch_add_indicator": ([_P, _P, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int64, _P],
                                ctypes.c_int),
    "pgm_batch_set_mode": ([_P, ctypes.c_int32], ctypes.c_int),
    "pgm_batch_blocks": ([_P, ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "pgm_batch_add_level": ([_P], ctypes.c_int),
    "pgm_batch_finalize": ([_P], ctypes.c_int),
    "pgm_batch_run": ([_P, _P], ctypes.c_int),
    "pgm_batch_destroy": ([_P], ctypes.c_int),
    "pgm_batch_specialise": ([_P, ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_codes_select": ([_P, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int32, ctypes.c_int64, _P, _P],
                         ctypes.c_int),
    "pgm_graph_capture_begin": ([_P], ctypes.c_int),
    "pgm_graph_capture_end": ([_P, ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_graph_launch": ([_P, _P], ctypes.c_int),
    "pgm_graph_destroy": ([_P], ctypes.c_int),
    "pgm_gather": ([ctypes.POINTER(GatherDesc), _P, _P, _P, _P, _P], ctypes.c_int),
    "pgm_indicator": ([_P, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int64, _P, _P],
                      ctypes.c_int),
    "pgm_argmax": ([_P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _P, _P, _P], ctypes.c_int),
    "pgm_rows_plan_create": ([ctypes.POINTER(RowsPlan), _P, ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_rows_plan_destroy": ([_P], ctypes.c_int),
    "pgm_rows_launch_info": ([ctypes.POINTER(RowsPlan), ctypes.c_int32, _P, ctypes.c_int64, ctypes.c_int64,
                              ctypes.c_int64, _P, _P, ctypes.c_int64, _P, _P, ctypes.c_int32,
                              ctypes.POINTER(RowsLaunchInfo)], ctypes.c_int),
    "pgm_rows_plan_run": ([_P, ctypes.c_int32, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _P, _P,
                           ctypes.c_int64, _P, _P, _P, _P], ctypes.c_int),
    "pgm_rows_plan_bind": ([_P, ctypes.c_int32, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _P, _P,
                            ctypes.c_int64, _P, _P, _P, _P, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "pgm_rows_bound_run": ([_P], ctypes.c_int),
    "pgm_rows_plan_source": ([ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)],
                             ctypes.c_int),
    "pgm_rows_plan_stream_source": ([ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                     ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "pgm_rows_bound_destroy": ([_P], ctypes.c_int),
    "pgm_rows_bound_kernel": ([_P, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32),
                               ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
    "pgm_rows_shard_run": ([ctypes.POINTER(_P), ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_int64, ctypes.c_int64,
                            ctypes.c_int64, _P, ctypes.c_int64, _P, _P], ctypes.c_int),
    "pgm_host_any_negative_i8": ([ctypes.POINTER(_P), ctypes.c_int32, ctypes.c_int64, _P, ctypes.c_int32], ctypes.c_int),
    "pgm_host_scan_begin": ([ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_host_scan_push": ([_P, ctypes.POINTER(_P), ctypes.c_int32], ctypes.c_int),
    "pgm_host_scan_end": ([_P, _P, ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "pgm_host_lut_map_u8": ([ctypes.POINTER(_P), ctypes.POINTER(_P), ctypes.c_int32, ctypes.c_int64, _P, ctypes.c_int64,
                             ctypes.c_int32], ctypes.c_int),
    "pgm_rows_ring_create": ([_P, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64),
                              ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.POINTER(_P), ctypes.c_int64,
                              ctypes.POINTER(_P), ctypes.POINTER(_P), _P, _P, ctypes.POINTER(ctypes.c_void_p)],
                             ctypes.c_int),
    "pgm_rows_ring_start": ([_P, ctypes.c_uint32, ctypes.c_double], ctypes.c_int),
    "pgm_rows_ring_start_ready": ([_P, ctypes.c_uint32, ctypes.c_double, ctypes.c_double], ctypes.c_int),
    "pgm_rows_ring_post": ([_P, ctypes.c_uint32], ctypes.c_int),
    "pgm_rows_ring_finish": ([_P], ctypes.c_int),
    "pgm_rows_ring_cancel": ([_P], ctypes.c_int),
    "pgm_rows_ring_counter": ([_P, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
    "pgm_rows_ring_kernel": ([_P, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32),
                              ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
    "pgm_rows_ring_destroy": ([_P], ctypes.c_int),
    "pgm_codes_remap": ([_P, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, _P, ctypes.c_int32, _P, _P,
                         ctypes.c_int64, _P, _P, _P, _P, _P], ctypes.c_int),
    "pgm_sample_joint": ([_P, ctypes.c_int64, ctypes.c_int64, _P, _P, ctypes.c_int64, _P, _P], ctypes.c_int),
    "pgm_dq_create": ([ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "pgm_dq_destroy": ([_P], ctypes.c_int),
    "pgm_dq_bind_rows": ([_P, _P, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "pgm_dq_launch": ([_P], ctypes.c_int),
    "pgm_dq_launch_group": ([ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32], ctypes.c_int),
    "pgm_dq_sync": ([_P], ctypes.c_int),
    "pgm_dq_wait": ([_P], ctypes.c_int),
    "pgm_dq_release": ([_P], ctypes.c_int),
    "pgm_dq_launch_release": ([_P], ctypes.c_int),
    "pgm_dq_timer_start": ([_P], ctypes.c_int),
    "pgm_dq_timer_stop_ms": ([_P, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
    "pgm_dq_timer_stop_ticks": ([_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                 ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "pgm_dq_timer_dispatch_stats": ([_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)],
                                    ctypes.c_int),
    "pgm_dq_bound_destroy": ([_P], ctypes.c_int),
    "pgm_dq_bound_info": ([_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                           ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "pgm_dq_bind_pm": ([_P, _P, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "pgm_dq_run_chain": ([ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32],
                         ctypes.c_int),
    "pgm_dq_profiling": ([_P, ctypes.c_int32], ctypes.c_int),
    "pgm_dq_timer_dispatch_times": ([_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                     ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "pgm_fit_plan_create": ([ctypes.POINTER(FitFamily), ctypes.c_int32, ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_fit_plan_destroy": ([_P], ctypes.c_int),
    "pgm_fit_plan_info": ([_P, ctypes.POINTER(FitInfo), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                           ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "pgm_fit_count": ([_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _P, _P, _P],
                      ctypes.c_int),
    "pgm_fit_finish": ([_P, _P, _P, ctypes.c_int32, _P, _P], ctypes.c_int),
    "pgm_fit_score": ([_P, _P, ctypes.c_int32, _P, _P, _P, _P, _P], ctypes.c_int),
    "pgm_fit_states_observed": ([_P, _P, _P, _P], ctypes.c_int),
    "pgm_fit_citest": ([_P, _P, ctypes.c_double, ctypes.c_int32, _P, _P, _P, _P], ctypes.c_int),
    "pgm_fit_estep_info": ([_P, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.POINTER(EmInfo)], ctypes.c_int),
    "pgm_fit_estep": ([_P, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, _P, _P, ctypes.c_int32, ctypes.c_int64,
                       ctypes.c_int64, ctypes.c_int64, _P, _P, _P], ctypes.c_int),
    "pgm_fit_logprob_info": ([_P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(LogpInfo)],
                             ctypes.c_int),
    "pgm_fit_log_values": ([_P, _P, _P, _P], ctypes.c_int),
    "pgm_fit_logprob": ([_P, _P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, _P],
                        ctypes.c_int),
    "pgm_sample_plan_create": ([ctypes.POINTER(FitFamily), ctypes.c_int32, ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_sample_plan_destroy": ([_P], ctypes.c_int),
    "pgm_sample_plan_info": ([_P, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, ctypes.POINTER(SampleInfo),
                              ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "pgm_sample_cdf": ([_P, _P, _P, _P], ctypes.c_int),
    "pgm_sample_forward": ([_P, _P, _P, _P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                            ctypes.c_int64, ctypes.c_uint64, _P, _P, _P], ctypes.c_int),
    "pgm_sample_posterior_info": ([_P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(LwInfo)],
                                  ctypes.c_int),
    "pgm_sample_posterior": ([_P, _P, _P, _P, _P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                              ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32, _P, _P, _P, _P, _P, _P],
                             ctypes.c_int),
    "pgm_gibbs_plan_create": ([ctypes.POINTER(FitFamily), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
                               ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_gibbs_plan_destroy": ([_P], ctypes.c_int),
    "pgm_gibbs_plan_info": ([_P, ctypes.c_int64, ctypes.POINTER(GibbsInfo), ctypes.POINTER(ctypes.c_int64),
                             ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
                             ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "pgm_gibbs_start": ([_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                         ctypes.c_uint64, _P], ctypes.c_int),
    "pgm_gibbs_sweep": ([_P, _P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                         ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64, _P, _P, ctypes.c_int64, ctypes.c_int64, _P, _P],
                        ctypes.c_int),
    "pgm_pair_plan_create": ([ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
                              ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_pair_plan_destroy": ([_P], ctypes.c_int),
    "pgm_pair_plan_info": ([_P, ctypes.POINTER(PairInfo), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
                            ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "pgm_pair_plan_set_slice": ([_P, ctypes.c_int64], ctypes.c_int),
    "pgm_pair_count_info": ([_P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                             ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                             ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "pgm_pair_count": ([_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                        ctypes.c_int32, _P, _P], ctypes.c_int),
    "pgm_pair_mi": ([_P, _P, ctypes.c_int32, _P, _P, _P, _P, _P], ctypes.c_int),
    "pgm_pair_emi": ([_P, _P, ctypes.c_int32, _P, _P], ctypes.c_int),
    "pgm_lg_gram_plan_create": ([ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_lg_gram_plan_destroy": ([_P], ctypes.c_int),
    "pgm_lg_gram_plan_info": ([_P, ctypes.POINTER(LgGramInfo), ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "pgm_lg_gram_plan_set_slice": ([_P, ctypes.c_int64], ctypes.c_int),
    "pgm_lg_gram_info": ([_P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
                          ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "pgm_lg_colsum": ([_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _P, _P, _P], ctypes.c_int),
    "pgm_lg_gram": ([_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _P, _P, _P], ctypes.c_int),
    "pgm_lg_net_create": ([ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
                           ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_lg_net_destroy": ([_P], ctypes.c_int),
    "pgm_lg_net_info": ([_P, ctypes.POINTER(LgNetInfo), ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "pgm_lg_sample": ([_P, _P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                       ctypes.c_uint64, _P], ctypes.c_int),
    "pgm_lg_logpdf": ([_P, _P, _P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _P, _P, _P],
                      ctypes.c_int),
    "pgm_lg_affine": ([_P, _P, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_int32,
                       ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, _P], ctypes.c_int),
    "pgm_lgs_jobs_create": ([ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                             ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_lgs_jobs_destroy": ([_P], ctypes.c_int),
    "pgm_lgs_jobs_info": ([_P, ctypes.POINTER(LgsInfo), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)],
                          ctypes.c_int),
    "pgm_lgs_pcorr": ([_P, _P, _P, ctypes.c_int32, ctypes.c_int32, _P, _P, _P, _P], ctypes.c_int),
    "pgm_lgs_score": ([_P, _P, _P, ctypes.c_int32, ctypes.c_int32, _P, _P, _P, _P], ctypes.c_int),
    "pgm_lgs_ibeta_half": ([ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_double)], ctypes.c_int),
    "pgm_dbn_plan_create": ([ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8),
                             ctypes.c_int32, ctypes.POINTER(FitFamily), ctypes.c_int32, ctypes.POINTER(FitFamily),
                             ctypes.c_int32, ctypes.POINTER(_P)], ctypes.c_int),
    "pgm_dbn_plan_destroy": ([_P], ctypes.c_int),
    "pgm_dbn_info": ([_P, ctypes.POINTER(DbnInfo), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)],
                     ctypes.c_int),
    "pgm_dbn_run": ([_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, _P, _P, _P, _P,
                     _P, _P, _P, ctypes.c_int64, _P], ctypes.c_int),
    "pgm_dbn_viterbi": ([_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, _P, _P, _P,
                         ctypes.c_int64, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P], ctypes.c_int),
    "pgm_dbn_estep_info": ([_P, ctypes.c_uint32, ctypes.POINTER(DbnEstepInfo)], ctypes.c_int),
    "pgm_dbn_estep": ([_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, _P, _P, _P, _P,
                       _P, _P, _P, ctypes.c_int64, ctypes.c_uint32, _P], ctypes.c_int),
}

EXPORTED = tuple(_SIGS)

_lock = threading.Lock()
_lib = None
_device_ok = None


def load_library():
    """Load libpgmhip.so (no GPU needed). Raises NativeUnavailable if it was not built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NativeUnavailable(
                f"{LIB_PATH} is missing: build it with `python -m pgmpy_amd.build` (hipcc --offload-arch=gfx950)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (argtypes, restype) in _SIGS.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = lib
        return lib


def last_error():
    lib = load_library()
    buf = ctypes.create_string_buffer(1024)
    lib.pgm_last_error(buf, len(buf))
    return buf.value.decode(errors="replace")


def check(rc, what=""):
    if rc == PGM_OK:
        return
    msg = f"{what}: {last_error()}" if what else last_error()
    if rc == PGM_EINVAL:
        raise ValueError(msg)
    if rc == PGM_EINDEX:
        raise IndexError(msg)
    if rc == PGM_ENOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def lib():
    """The library, for compute: additionally requires a visible GPU (no CPU fallback)."""
    global _device_ok
    L = load_library()
    if _device_ok is None:
        import torch

        _device_ok = bool(torch.cuda.is_available())
    if not _device_ok:
        raise NativeUnavailable("no HIP device visible: the gfx950 kernels need an MI355X (no CPU fallback)")
    return L


def stream_handle(stream=None):
    import torch

    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


class _HostBytes:
    """Owner of one pinned host allocation (pgm_host_alloc), exported through __array_interface__:
    numpy arrays made from it (and their views) reference it, so the memory is freed by reference
    counting as soon as the last of them is gone (no cycle back to the HostBuffer)."""

    def __init__(self, ptr, nbytes):
        self._p = ctypes.c_void_p(ptr)
        self.__array_interface__ = {"data": (ptr, False), "shape": (nbytes,), "typestr": "|u1", "version": 3}

    def __del__(self):
        p = getattr(self, "_p", None)
        if p is not None and p.value:
            try:
                load_library().pgm_host_free(p)
            except Exception:
                pass
            self._p = None


class HostBuffer:
    """Pinned, mapped, coherent host memory that kernels read and write directly (pgm_host_alloc):
    `array` (numpy) and `tensor` (a CPU torch view of the same bytes, for descriptor building) share
    it; the memory belongs to the _HostBytes object the arrays are based on and is freed once the
    HostBuffer and every array / tensor viewing it are gone."""

    def __init__(self, shape, dtype):
        import torch

        L = lib()
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) if len(shape) else 1
        p = ctypes.c_void_p()
        nbytes = max(1, n * dtype.itemsize)
        check(L.pgm_host_alloc(ctypes.byref(p), nbytes), "host_alloc")
        raw = np.asarray(_HostBytes(p.value, nbytes))
        self.array = raw[:n * dtype.itemsize].view(dtype).reshape(shape)
        self.tensor = torch.from_numpy(self.array)


def ptr(t):
    """Raw device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def i64arr(vals):
    a = _I64()
    for i, v in enumerate(vals):
        a[i] = int(v)
    return a
