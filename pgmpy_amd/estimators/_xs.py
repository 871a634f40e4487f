"""Binding of the pgm_xs_* entry points (include/pgmhip.h "Exact structure search", pgmpy_amd/csrc/pgmxs.hip): the
highest-scoring DAG over n nodes from a list of scored families, by the subset-lattice dynamic programme.

A family is (node, parent mask, score); nodes are 0 .. n - 1, a mask has bit u set when u is a parent.
"""
import ctypes

import numpy as np

from .. import _native as N
from .._plan import Plan


class XsPlan(Plan):
    _destroy = "pgm_xs_destroy"

    def __init__(self, n, tile_log2=None, high_bits=None):
        L = N.load_library()  # creating and inspecting a handle needs no device
        self.n = int(n)
        self._h = ctypes.c_void_p()
        N.check(L.pgm_xs_create(self.n, ctypes.byref(self._h)), "xs_create")
        if tile_log2 is not None or high_bits is not None:
            info = self.info()
            N.check(L.pgm_xs_set_tiling(self._h, int(info.tile_log2 if tile_log2 is None else tile_log2),
                                        int(info.high_bits if high_bits is None else high_bits)), "xs_set_tiling")

    def info(self):
        info = N.XsInfo()
        N.check(N.load_library().pgm_xs_info(self._h, ctypes.byref(info)), "xs_info")
        return info

    def phase_ms(self):
        """{"scatter", "zeta", "sink"}: the device milliseconds of the phases of the last run (HIP events)."""
        ms = (ctypes.c_double * N.XS_PHASES)()
        N.check(N.load_library().pgm_xs_phase_ms(self._h, ms), "xs_phase_ms")
        return dict(zip(("scatter", "zeta", "sink"), ms))

    @property
    def q_cells(self):
        return self.n << (self.n - 1)

    def run(self, nodes, masks, scores, want_tables=False):
        """{"score", "infeasible", "parents" (a mask per node), "order" (sinks first)} of the families given as three
        equally long sequences; with want_tables also "Q", "A" ([n, 2^(n-1)]), "R", "K" ([2^n]) as numpy arrays.
        Synchronises the stream."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        masks = np.ascontiguousarray(masks, dtype=np.uint32)
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        if not (nodes.ndim == masks.ndim == scores.ndim == 1 and len(nodes) == len(masks) == len(scores)):
            raise ValueError("nodes, masks and scores must be three sequences of one length")
        L = N.lib()
        values = winners = None
        if want_tables:
            import torch

            cells = self.q_cells + (1 << self.n)
            values = torch.empty(cells, dtype=torch.float64, device="cuda")
            winners = torch.empty(cells, dtype=torch.int32, device="cuda")
        out = N.XsResult()
        N.check(L.pgm_xs_run(self._h, nodes.ctypes.data, masks.ctypes.data, scores.ctypes.data, len(nodes),
                             ctypes.byref(out), N.ptr(values), N.ptr(winners), N.stream_handle()), "xs_run")
        res = {"score": float(out.score), "infeasible": bool(out.infeasible), "parents": list(out.parents[:self.n]),
               "order": list(out.order[:self.n])}
        if want_tables:
            v, w = values.cpu().numpy(), winners.cpu().numpy().view(np.uint32)
            rows = 1 << (self.n - 1)
            res.update(Q=v[:self.q_cells].reshape(self.n, rows), A=w[:self.q_cells].reshape(self.n, rows),
                       R=v[self.q_cells:], K=w[self.q_cells:])
        return res
