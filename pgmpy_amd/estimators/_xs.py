"""Binding of the pgm_xs_* entry points (include/pgmhip.h "Exact structure search", pgmpy_amd/csrc/pgmxs.hip): the
highest-scoring DAG over n nodes from a list of scored families, by the subset-lattice dynamic programme, and the
exact posterior of every edge from the same list, by the same lattice in log space.

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
        self._posterior = False  # whether the last completed call was `posterior`
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
        """{"scatter", "zeta", "sink"}: the device milliseconds of the phases of the last run (HIP events); after a
        `posterior`, {"scatter", "alpha", "paths", "edges"}."""
        ms = (ctypes.c_double * N.XS_POST_PHASES)()
        N.check(N.load_library().pgm_xs_phase_ms(self._h, ms), "xs_phase_ms")
        names = ("scatter", "alpha", "paths", "edges") if self._posterior else ("scatter", "zeta", "sink")
        return dict(zip(names, ms))

    @property
    def q_cells(self):
        return self.n << (self.n - 1)

    @staticmethod
    def _families(nodes, masks, scores):
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        masks = np.ascontiguousarray(masks, dtype=np.uint32)
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        if not (nodes.ndim == masks.ndim == scores.ndim == 1 and len(nodes) == len(masks) == len(scores)):
            raise ValueError("nodes, masks and scores must be three sequences of one length")
        return nodes, masks, scores

    def posterior(self, nodes, masks, scores, want_tables=False):
        """{"edge_post" ([n, n]: row = parent, column = child), "log_z" (F[V], B[V]), "mass" ([n]), "infeasible"} of
        the families under the order-modular prior (pgm_xs_posterior); with want_tables also "alpha" ([n, 2^(n-1)]),
        "F", "B" ([2^n]).  Synchronises the stream."""
        nodes, masks, scores = self._families(nodes, masks, scores)
        L = N.lib()
        values = None
        if want_tables:
            import torch

            values = torch.empty(self.q_cells + (2 << self.n), dtype=torch.float64, device="cuda")
        post, log_z, mass = np.empty((self.n, self.n)), np.empty(2), np.empty(self.n)
        infeasible = ctypes.c_int32()
        N.check(L.pgm_xs_posterior(self._h, nodes.ctypes.data, masks.ctypes.data, scores.ctypes.data, len(nodes),
                                   post.ctypes.data, log_z.ctypes.data, mass.ctypes.data, ctypes.byref(infeasible),
                                   N.ptr(values), N.stream_handle()), "xs_posterior")
        self._posterior = True
        res = {"edge_post": post, "log_z": log_z, "mass": mass, "infeasible": bool(infeasible.value)}
        if want_tables:
            v, sets = values.cpu().numpy(), 1 << self.n
            res.update(alpha=v[:self.q_cells].reshape(self.n, sets >> 1), F=v[self.q_cells:self.q_cells + sets],
                       B=v[self.q_cells + sets:])
        return res

    def run(self, nodes, masks, scores, want_tables=False):
        """{"score", "infeasible", "parents" (a mask per node), "order" (sinks first)} of the families given as three
        equally long sequences; with want_tables also "Q", "A" ([n, 2^(n-1)]), "R", "K" ([2^n]) as numpy arrays.
        Synchronises the stream."""
        nodes, masks, scores = self._families(nodes, masks, scores)
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
        self._posterior = False
        res = {"score": float(out.score), "infeasible": bool(out.infeasible), "parents": list(out.parents[:self.n]),
               "order": list(out.order[:self.n])}
        if want_tables:
            v, w = values.cpu().numpy(), winners.cpu().numpy().view(np.uint32)
            rows = 1 << (self.n - 1)
            res.update(Q=v[:self.q_cells].reshape(self.n, rows), A=w[:self.q_cells].reshape(self.n, rows),
                       R=v[self.q_cells:], K=w[self.q_cells:])
        return res
