"""Binding of the pgm_gibbs_* entry points (include/pgmhip.h, pgmpy_amd/csrc/pgmgibbs.hip): many Gibbs
chains per launch, one per lane, in the column-major uint8 code matrix.

A factor is ``(columns, cardinalities)`` in the C order of its table: a CPD is ``[node, parents...]``, a
Markov network's factor is given as it stands.  The values share the fit plan's flat layout: factor f
occupies ``[offsets[f], offsets[f] + sizes[f])``.
"""
import ctypes

import numpy as np

from .. import _native as N
from .._plan import MASK64, Plan, codes_window, family_array, flat_tensor

LDS, GLOBAL = N.GIBBS_LDS, N.GIBBS_GLOBAL
PATH_NAMES = {LDS: "LDS", GLOBAL: "GLOBAL"}
MAX_SWEEP = (1 << 32) - 1


class GibbsPlan(Plan):
    _destroy = "pgm_gibbs_plan_destroy"

    def __init__(self, factors, card):
        L = N.load_library()  # building and inspecting a plan needs no device
        self.factors, fams = family_array(factors)
        self.families = self.factors  # table(): a factor's [first column, the others] view
        self.card = [int(k) for k in card]
        self.n_cols = len(self.card)
        self._h = ctypes.c_void_p()
        cards = (ctypes.c_int32 * max(self.n_cols, 1))(*self.card)
        N.check(L.pgm_gibbs_plan_create(fams, len(self.factors), cards, self.n_cols, ctypes.byref(self._h)),
                "gibbs_plan_create")
        n = len(self.factors)
        off, size = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
        inc_off = (ctypes.c_int32 * (self.n_cols + 1))()
        self.info = self.launch_info(0, offsets=off, sizes=size, inc_off=inc_off)
        inc = (ctypes.c_int32 * max(2 * int(self.info.total_incidences), 1))()
        self.launch_info(0, inc=inc)
        self.offsets, self.sizes = list(off), list(size)
        self.inc_off = list(inc_off)
        # per column: [(factor, position of the column in it)], factors ascending
        self.incident = [[(inc[2 * e], inc[2 * e + 1]) for e in range(self.inc_off[c], self.inc_off[c + 1])]
                         for c in range(self.n_cols)]
        self.total_entries = int(self.info.total_entries)

    def launch_info(self, n_chains, offsets=None, sizes=None, inc_off=None, inc=None):
        """GibbsInfo of a launch with n_chains chains (pgm_gibbs_plan_info; no device)."""
        info = N.GibbsInfo()
        N.check(N.load_library().pgm_gibbs_plan_info(self._h, int(n_chains), ctypes.byref(info), offsets, sizes, inc_off,
                                                     inc), "gibbs_plan_info")
        return info

    def start(self, codes, n_chains=None, row0=0, first_chain=0, seed=0):
        """Column c of every chain becomes floor(u * card[c]) from the sweep-0 uniform of (seed, chain, c)."""
        L = N.lib()
        n_cols, ld, n_chains = codes_window(codes, n_chains, row0)
        N.check(L.pgm_gibbs_start(self._h, N.ptr(codes), n_cols, ld, int(row0), n_chains, int(first_chain),
                                  int(seed) & MASK64, N.stream_handle()), "gibbs_start")
        return codes

    def sweep(self, values, codes, n_sweeps, n_chains=None, row0=0, first_chain=0, first_sweep=1, seed=0, clamp=None,
              trace=None, thin=1, uniforms=None):
        """Advance the chains in rows [row0, row0 + n_chains) of the device codes [n_cols, ld] (uint8), in
        place, through sweeps first_sweep .. first_sweep + n_sweeps - 1 of chains [first_chain, ...) of the
        stream of `seed`.  clamp: one uint8 per column (non-zero: the column keeps its code).  trace: a
        uint8 device tensor [n_cols, ld_trace] that receives the state after every thin-th sweep.
        uniforms: an fp64 device tensor [n_sweeps, n_cols, ld] that replaces the generator.  Raises
        ValueError when a conditional's total is not finite or not > 0, IndexError when a code is not a
        state."""
        import torch

        L = N.lib()
        n_cols, ld, n_chains = codes_window(codes, n_chains, row0)
        n_sweeps = int(n_sweeps)
        flat_tensor("values", values, self.total_entries)
        ld_trace = 0
        if trace is not None:
            if trace.dtype != torch.uint8 or trace.dim() != 2 or trace.shape[0] != n_cols or not trace.is_contiguous():
                raise ValueError("trace must be a contiguous [n_cols, ld_trace] uint8 device tensor")
            ld_trace = int(trace.shape[1])
        if uniforms is not None and (uniforms.dtype != torch.float64 or tuple(uniforms.shape) != (n_sweeps, n_cols, ld)
                                     or not uniforms.is_contiguous()):
            raise ValueError("uniforms must be a contiguous fp64 device tensor [n_sweeps, n_cols, ld]")
        m = None
        if clamp is not None:
            m = np.ascontiguousarray(clamp, dtype=np.uint8)
            if m.shape != (self.n_cols,):
                raise ValueError(f"clamp must have one entry per column ({self.n_cols})")
        N.check(L.pgm_gibbs_sweep(self._h, N.ptr(values), N.ptr(codes), n_cols, ld, int(row0), n_chains, int(first_chain),
                                  int(first_sweep), n_sweeps, int(seed) & MASK64,
                                  None if m is None else m.ctypes.data_as(ctypes.c_void_p), N.ptr(trace), ld_trace,
                                  int(thin), N.ptr(uniforms), N.stream_handle()), "gibbs_sweep")
        return codes
