"""Binding of the pgm_mplp_* entry points (include/pgmhip.h "MAP by max-product linear programming",
pgmpy_amd/csrc/pgmmplp.hip): MPLP on a Markov network for a batch of instances in one launch.

A plan is made from the nodes' cardinalities and the clusters (2 or 3 node indices each), the last `n_triplets`
of them tightening triplets; it is structure only: the node terms and the cluster terms are arguments of a run.
"""
import ctypes

from .. import _native as N
from .._plan import Plan, flat_tensor


class MplpPlan(Plan):
    _destroy = "pgm_mplp_plan_destroy"

    def __init__(self, card, clusters, n_triplets=0):
        L = N.load_library()  # building and inspecting a plan needs no device
        self.card = [int(k) for k in card]
        self.clusters = [tuple(int(v) for v in c) for c in clusters]
        self.n_triplets = int(n_triplets)
        n, m = len(self.card), len(self.clusters)
        c_card = (ctypes.c_int32 * max(n, 1))(*self.card)
        c_nv = (ctypes.c_int32 * max(m, 1))(*[len(c) for c in self.clusters])
        c_vars = (ctypes.c_int32 * max(3 * m, 1))()
        for i, c in enumerate(self.clusters):
            for j, v in enumerate(c[:3]):
                c_vars[3 * i + j] = v
        self._h = ctypes.c_void_p()
        N.check(L.pgm_mplp_plan_create(c_card, n, c_nv, c_vars, m, self.n_triplets, ctypes.byref(self._h)), "mplp_plan_create")
        self.info = N.MplpInfo()
        node_off, cl_off = (ctypes.c_int32 * (n + 1))(), (ctypes.c_int32 * (m + 1))()
        sets, level = (ctypes.c_int32 * max(m, 1))(), (ctypes.c_int32 * max(m, 1))()
        N.check(L.pgm_mplp_plan_info(self._h, ctypes.byref(self.info), node_off, cl_off, sets, level), "mplp_plan_info")
        self.node_offsets, self.cluster_offsets = list(node_off), list(cl_off)
        self.set_counts, self.levels = list(sets)[:m], list(level)[:m]
        self.n_nodes, self.n_unary, self.n_theta = n, int(self.info.n_unary), int(self.info.n_theta)
        self.n_msg, self.state_len, self.n_levels = int(self.info.n_msg), int(self.info.state_len), int(self.info.n_levels)

    def run(self, unaries, theta, n_iter, dual_threshold=0.0, gap_threshold=0.0, state=None, want_state=False):
        """Run every row of the device `unaries` [B, n_unary] (fp64) with the cluster terms `theta` [n_theta] for
        at most `n_iter` iterations, from `state` [B, state_len] when given.  Returns device tensors (codes [B,
        n_nodes] uint8, values [B, 4] fp64: best primal, dual_lp, dual_gap, integrality_gap, iters [B] int32, the
        state [B, state_len] or None)."""
        import torch

        L = N.lib()
        if unaries.dim() != 2 or int(unaries.shape[1]) != self.n_unary:
            raise ValueError(f"unaries must be [B, {self.n_unary}]: one row of node terms per instance")
        B = int(unaries.shape[0])
        flat_tensor("unaries", unaries, B * self.n_unary)
        flat_tensor("theta", theta, self.n_theta)
        if state is not None:
            if state.dim() != 2 or tuple(state.shape) != (B, self.state_len):
                raise ValueError(f"state must be [{B}, {self.state_len}]")
            flat_tensor("state", state, B * self.state_len)
        dev = unaries.device
        codes = torch.empty((B, self.n_nodes), dtype=torch.uint8, device=dev)
        values = torch.empty((B, N.MPLP_VALUES), dtype=torch.float64, device=dev)
        iters = torch.empty(B, dtype=torch.int32, device=dev)
        out = torch.empty((B, self.state_len), dtype=torch.float64, device=dev) if want_state else None
        N.check(L.pgm_mplp_run(self._h, N.ptr(unaries), N.ptr(theta), B, int(n_iter), float(dual_threshold),
                               float(gap_threshold), N.ptr(state), N.ptr(codes), N.ptr(values), N.ptr(iters), N.ptr(out),
                               N.stream_handle()), "mplp_run")
        return codes, values, iters, out
