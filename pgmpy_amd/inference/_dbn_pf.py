"""Binding of the pgm_dbn_pf_* entry points (include/pgmhip.h "dynamic Bayesian networks: the particle filter",
pgmpy_amd/csrc/pgmdbn_pf.hip): a bootstrap particle filter over a batch of evidence sequences in one launch, for
two-slice networks whose joint is too large for the exact plan of ``_dbn.DbnPlan``.

A plan is made from the slice nodes' cardinalities, a queried flag per node and the two family sets of a
``DbnPlan``; any cell may be observed in one sequence and 255 in the next.
"""
import ctypes

from .. import _native as N
from .._plan import Plan, codes_window, family_array, flat_tensor


class DbnPfPlan(Plan):
    _destroy = "pgm_dbn_pf_plan_destroy"

    def __init__(self, card, queried, families0, families1):
        L = N.load_library()  # building and inspecting a plan needs no device
        n = len(card)
        self.families0, fams0 = family_array(families0)
        self.families1, fams1 = family_array(families1)
        self.card = [int(k) for k in card]
        self.queried = [bool(q) for q in queried]
        c_card = (ctypes.c_int32 * max(n, 1))(*self.card)
        c_queried = (ctypes.c_uint8 * max(n, 1))(*[int(q) for q in self.queried])
        self._h = ctypes.c_void_p()
        N.check(L.pgm_dbn_pf_plan_create(c_card, c_queried, n, fams0, len(self.families0), fams1, len(self.families1),
                                         ctypes.byref(self._h)), "dbn_pf_plan_create")
        self.n = n
        order0, order1 = (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)()
        off0, off1 = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
        self.info = N.DbnPfInfo()
        N.check(L.pgm_dbn_pf_plan_info(self._h, N.DBN_PF_MIN_PARTICLES, ctypes.byref(self.info), order0, order1, off0, off1),
                "dbn_pf_plan_info")
        self.order0, self.order1 = list(order0), list(order1)
        self.offsets0, self.offsets1 = list(off0), list(off1)
        self.n_query, self.n_query_nodes = int(self.info.n_query), int(self.info.n_query_nodes)
        self.max_particles = int(self.info.max_particles)
        # the columns of a queried node in the Q axis
        self.query_slices, q = {}, 0
        for v in range(n):
            if self.queried[v]:
                self.query_slices[v] = slice(q, q + self.card[v])
                q += self.card[v]

    def info_at(self, n_particles):
        """pgm_dbn_pf_info_t at `n_particles` per sequence: the block, the LDS bytes, the largest count that fits."""
        info = N.DbnPfInfo()
        N.check(N.load_library().pgm_dbn_pf_plan_info(self._h, int(n_particles), ctypes.byref(info), None, None, None, None),
                "dbn_pf_plan_info")
        return info

    def run(self, codes, values0, values1, n_particles, seed, first_row=0, n_rows=None, row0=0, want_filter=True,
            want_traj=False, strict=True):
        """Filter the rows [row0, row0 + n_rows) of the device codes [T n, ld] (uint8) with `n_particles` particles
        each; row r of the window uses the stream rows first_row + r n_particles + i of `seed`.  Returns device
        tensors (filter [n_rows, T, Q] fp64 or None, loglik [n_rows], ess [n_rows, T], flags [n_rows] uint8:
        N.DBN_PF_IMPOSSIBLE / N.DBN_PF_BAD, ancestors [n_rows, T, N] int16 holding uint16 and traj [n_rows, T,
        queried nodes, N] uint8, or None for both).  A code that is no state raises IndexError unless `strict` is
        False: its sequence is then flagged N.DBN_PF_BAD and NaN, the others are as without it."""
        import torch

        L = N.lib()
        n_cols, ld, n_rows = codes_window(codes, n_rows, row0)
        if n_cols % self.n:
            raise ValueError(f"codes have {n_cols} columns, not a multiple of the {self.n} slice nodes")
        T, P, Q = n_cols // self.n, int(n_particles), self.n_query
        flat_tensor("values0", values0, int(self.info.values0))
        flat_tensor("values1", values1, int(self.info.values1))
        dev, rows = codes.device, max(n_rows, 0)
        filt = torch.empty((rows, T, Q), dtype=torch.float64, device=dev) if want_filter else None
        loglik = torch.empty(rows, dtype=torch.float64, device=dev)
        ess = torch.empty((rows, T), dtype=torch.float64, device=dev)
        flags = torch.empty(rows, dtype=torch.uint8, device=dev)
        anc = torch.empty((rows, T, max(P, 0)), dtype=torch.int16, device=dev) if want_traj else None
        traj = torch.empty((rows, T, self.n_query_nodes, max(P, 0)), dtype=torch.uint8, device=dev) if want_traj else None
        try:
            N.check(L.pgm_dbn_pf_run(self._h, N.ptr(codes), n_cols, ld, int(row0), n_rows, T, N.ptr(values0), N.ptr(values1),
                                     P, int(first_row), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), N.ptr(filt), N.ptr(loglik),
                                     N.ptr(ess), N.ptr(flags), N.ptr(anc), N.ptr(traj), N.stream_handle()), "dbn_pf_run")
        except IndexError:
            if strict:
                raise
        return filt, loglik, ess, flags, anc, traj

    def trace(self, anc, traj, out=None, row0_out=0):
        """The traced trajectories of `run(want_traj=True)`: a uint8 code matrix [T queried nodes, n_rows N] (or the
        rows [row0_out, row0_out + n_rows N) of `out`), column t queried nodes + k the k-th queried node of slice t."""
        import torch

        L = N.lib()
        rows, T, P = (int(x) for x in anc.shape)
        if out is None:
            out = torch.empty((T * self.n_query_nodes, max(rows * P, 1)), dtype=torch.uint8, device=anc.device)
        N.check(L.pgm_dbn_pf_trace(self._h, N.ptr(anc), N.ptr(traj), rows, T, P, N.ptr(out), int(out.shape[1]), int(row0_out),
                                   N.stream_handle()), "dbn_pf_trace")
        return out
