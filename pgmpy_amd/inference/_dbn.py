"""Binding of the pgm_dbn_* entry points (include/pgmhip.h, pgmpy_amd/csrc/pgmdbn.hip): filtering,
smoothing and the log-likelihood of a batch of evidence sequences under a two-slice network in one launch,
and (pgm_dbn_viterbi) their most probable completions.

A plan is made from the slice nodes' cardinalities, a clamped and a queried flag per node and two family
sets, ``(columns, cardinalities)`` as in a fit plan: the slice-0 families over columns ``0 .. n - 1`` and
the transition families, whose node is a column ``n .. 2n - 1`` and whose parents are columns of slice t
(``0 .. n - 1``) or of slice t + 1.  The values of a set lie end to end in the order its families are given.
"""
import ctypes

import numpy as np

from .. import _native as N
from .._plan import Plan, codes_window, family_array, flat_tensor

SCRATCH_BYTES = 1 << 30  # the most scratch one launch of a smoother takes; a larger batch is split by rows


class DbnPlan(Plan):
    _destroy = "pgm_dbn_plan_destroy"

    def __init__(self, card, clamped, queried, families0, families1):
        L = N.load_library()  # building and inspecting a plan needs no device
        n = len(card)
        self.families0, fams0 = family_array(families0)
        self.families1, fams1 = family_array(families1)
        self.card = [int(k) for k in card]
        self.clamped = [bool(c) for c in clamped]
        self.queried = [bool(q) for q in queried]
        c_card = (ctypes.c_int32 * max(n, 1))(*self.card)
        c_clamped = (ctypes.c_uint8 * max(n, 1))(*[int(c) for c in self.clamped])
        c_queried = (ctypes.c_uint8 * max(n, 1))(*[int(q) for q in self.queried])
        self._h = ctypes.c_void_p()
        N.check(L.pgm_dbn_plan_create(c_card, c_clamped, c_queried, n, fams0, len(self.families0), fams1,
                                      len(self.families1), ctypes.byref(self._h)), "dbn_plan_create")
        self.info = N.DbnInfo()
        off0, off1 = (ctypes.c_int64 * max(n, 1))(), (ctypes.c_int64 * max(n, 1))()
        N.check(L.pgm_dbn_info(self._h, ctypes.byref(self.info), off0, off1), "dbn_info")
        self.offsets0, self.offsets1 = list(off0)[:n], list(off1)[:n]
        self.n = n
        self.n_query = int(self.info.n_query)
        # the columns of a queried node in the Q axis
        self.query_slices, q = {}, 0
        for v in range(n):
            if self.queried[v]:
                self.query_slices[v] = slice(q, q + self.card[v])
                q += self.card[v]

    def scratch_bytes(self, n_rows, n_slices):
        return int(n_rows) * int(n_slices) * int(self.info.scratch_per_slice) * 8

    def run(self, codes, values0, values1, n_rows=None, row0=0, want_filter=False, want_smooth=False, want_loglik=True,
            scratch_bytes=SCRATCH_BYTES):
        """Run the rows [row0, row0 + n_rows) of the device codes [(T + 1) n, ld] (uint8).  Returns
        (filter, smooth, loglik, impossible): fp64 device tensors [n_rows, T + 1, Q] (None when not asked
        for), fp64 [n_rows] and uint8 [n_rows].  A smoother whose scratch would pass `scratch_bytes` runs
        in several launches over row windows; a sequence's results do not depend on the split.  Raises
        ValueError when a clamped cell is missing or a code is no state."""
        import torch

        L = N.lib()
        n_cols, ld, n_rows = codes_window(codes, n_rows, row0)
        if n_cols % self.n:
            raise ValueError(f"codes have {n_cols} columns, not a multiple of the {self.n} slice nodes")
        n_slices = n_cols // self.n
        flat_tensor("values0", values0, int(self.info.values0))
        flat_tensor("values1", values1, int(self.info.values1))
        dev, Q = codes.device, self.n_query
        rows = max(n_rows, 0)
        filt = torch.empty((rows, n_slices, Q), dtype=torch.float64, device=dev) if want_filter else None
        smooth = torch.empty((rows, n_slices, Q), dtype=torch.float64, device=dev) if want_smooth else None
        loglik = torch.empty(rows, dtype=torch.float64, device=dev) if want_loglik else None
        impossible = torch.empty(rows, dtype=torch.uint8, device=dev)
        chunk = rows
        if want_smooth and rows:
            chunk = max(1, min(rows, int(scratch_bytes) // max(self.scratch_bytes(1, n_slices), 1)))
        scratch = torch.empty(self.scratch_bytes(chunk, n_slices) // 8, dtype=torch.float64, device=dev) if want_smooth else None
        # an empty (or negative) window still goes to the library once: it checks the arguments
        for r0 in range(0, rows, chunk) if rows else [0]:
            nr = min(chunk, rows - r0) if rows else n_rows

            def at(t, per_row):
                return None if t is None else ctypes.c_void_p(t.data_ptr() + r0 * per_row * t.element_size())

            N.check(L.pgm_dbn_run(self._h, N.ptr(codes), n_cols, ld, int(row0) + r0, nr, n_slices, N.ptr(values0),
                                  N.ptr(values1), at(filt, n_slices * Q), at(smooth, n_slices * Q), at(loglik, 1),
                                  at(impossible, 1), N.ptr(scratch), 0 if scratch is None else scratch.numel() * 8,
                                  N.stream_handle()), "dbn_run")
        return filt, smooth, loglik, impossible

    def estep_info(self, direct=False):
        """pgm_dbn_estep_info_t of an E-step over this plan: the accumulation path (N.DBN_ESTEP_TILE or
        N.DBN_ESTEP_DIRECT), the LDS bytes of a workgroup and the cap of the grid.  Needs no device."""
        L = N.load_library()
        info = N.DbnEstepInfo()
        N.check(L.pgm_dbn_estep_info(self._h, N.DBN_ESTEP_DIRECT if direct else 0, ctypes.byref(info)), "dbn_estep_info")
        return info

    def estep(self, codes, values0, values1, tables0=None, tables1=None, n_rows=None, row0=0, want_loglik=True,
              scratch_bytes=SCRATCH_BYTES, direct=False):
        """The E-step of Baum-Welch (pgm_dbn_estep) over the rows [row0, row0 + n_rows) of the device codes
        [(T + 1) n, ld] (uint8): every sequence adds its expected family counts under the CPD values to the
        fp64 device tables (zeroed flat buffers when None) in the layout of values0 / values1: slice 0 to
        tables0, slices 1 .. T to tables1.  Returns (tables0, tables1, loglik, impossible): loglik fp64
        [n_rows] (None when not asked for), impossible uint8 [n_rows]; an impossible sequence adds nothing.
        A batch whose scratch would pass `scratch_bytes` runs in several launches over row windows.  `direct`
        forces every add to be a global atomic.  Raises ValueError when a clamped cell is missing or a code
        is no state; the tables are then unspecified."""
        import torch

        L = N.lib()
        n_cols, ld, n_rows = codes_window(codes, n_rows, row0)
        if n_cols % self.n:
            raise ValueError(f"codes have {n_cols} columns, not a multiple of the {self.n} slice nodes")
        n_slices = n_cols // self.n
        flat_tensor("values0", values0, int(self.info.values0))
        flat_tensor("values1", values1, int(self.info.values1))
        dev = codes.device
        tables = []
        for name, t, size in (("tables0", tables0, int(self.info.values0)), ("tables1", tables1, int(self.info.values1))):
            if t is None:
                t = torch.zeros(size, dtype=torch.float64, device=dev)
            else:
                flat_tensor(name, t, size)
            tables.append(t)
        rows = max(n_rows, 0)
        loglik = torch.empty(rows, dtype=torch.float64, device=dev) if want_loglik else None
        impossible = torch.empty(rows, dtype=torch.uint8, device=dev)
        chunk = max(1, min(rows, int(scratch_bytes) // max(self.scratch_bytes(1, n_slices), 1))) if rows else 0
        scratch = torch.empty(max(self.scratch_bytes(chunk, n_slices) // 8, 1), dtype=torch.float64, device=dev)
        flags = N.DBN_ESTEP_DIRECT if direct else 0
        # an empty (or negative) window still goes to the library once: it checks the arguments
        for r0 in range(0, rows, chunk) if rows else [0]:
            nr = min(chunk, rows - r0) if rows else n_rows
            N.check(L.pgm_dbn_estep(self._h, N.ptr(codes), n_cols, ld, int(row0) + r0, nr, n_slices, N.ptr(values0),
                                    N.ptr(values1), N.ptr(tables[0]), N.ptr(tables[1]),
                                    None if loglik is None else ctypes.c_void_p(loglik.data_ptr() + r0 * 8),
                                    ctypes.c_void_p(impossible.data_ptr() + r0), N.ptr(scratch), scratch.numel() * 8, flags,
                                    N.stream_handle()), "dbn_estep")
        return tables[0], tables[1], loglik, impossible

    def viterbi_scratch_bytes(self, n_rows, n_slices):
        """Bytes of backpointers one launch of `viterbi` takes: a uint16 per state of every slice but the first."""
        return int(n_rows) * max(int(n_slices) - 1, 0) * int(self.info.n_configs) * 2

    def viterbi(self, codes, values0, values1, n_rows=None, row0=0, scratch_bytes=SCRATCH_BYTES):
        """The most probable completion of the rows [row0, row0 + n_rows) of the device codes [(T + 1) n, ld].
        Returns device tensors (path, logmap, impossible): uint8 [(T + 1) n, n_rows] in the layout of `codes`
        (a complete code matrix; 255 in the free cells of an impossible sequence), fp64 [n_rows] = log max_x
        P(x, e), uint8 [n_rows].  A batch whose backpointers would pass `scratch_bytes` runs in several launches
        over row windows; a sequence's results do not depend on the split.  Raises ValueError when a clamped
        cell is missing or a code is no state."""
        import torch

        L = N.lib()
        n_cols, ld, n_rows = codes_window(codes, n_rows, row0)
        if n_cols % self.n:
            raise ValueError(f"codes have {n_cols} columns, not a multiple of the {self.n} slice nodes")
        n_slices = n_cols // self.n
        flat_tensor("values0", values0, int(self.info.values0))
        flat_tensor("values1", values1, int(self.info.values1))
        dev = codes.device
        rows = max(n_rows, 0)
        ld_out = max(rows, 1)  # an empty window still hands the library a path to check
        path = torch.empty((n_cols, ld_out), dtype=torch.uint8, device=dev)
        logmap = torch.empty(rows, dtype=torch.float64, device=dev)
        impossible = torch.empty(rows, dtype=torch.uint8, device=dev)
        per_row = self.viterbi_scratch_bytes(1, n_slices)
        chunk = max(1, min(rows, int(scratch_bytes) // per_row)) if rows and per_row else rows
        scratch = torch.empty(max(chunk * per_row // 2, 1), dtype=torch.int16, device=dev)
        # an empty (or negative) window still goes to the library once: it checks the arguments
        for r0 in range(0, rows, chunk) if rows else [0]:
            nr = min(chunk, rows - r0) if rows else n_rows
            N.check(L.pgm_dbn_viterbi(self._h, N.ptr(codes), n_cols, ld, int(row0) + r0, nr, n_slices, N.ptr(values0),
                                      N.ptr(values1), N.ptr(path), ld_out, r0, ctypes.c_void_p(logmap.data_ptr() + r0 * 8),
                                      ctypes.c_void_p(impossible.data_ptr() + r0), N.ptr(scratch), scratch.numel() * 2,
                                      N.stream_handle()), "dbn_viterbi")
        return (path if rows else path[:, :0]), logmap, impossible


def flat_values(cpds):
    """The values of CPDs end to end, each in its own [node_card, prod(parent_card)] C order (host)."""
    return np.concatenate([np.asarray(c._values_readonly(), dtype=np.float64).reshape(-1) for c in cpds])
