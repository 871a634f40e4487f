"""Binding of the pgm_lbp_* entry points (include/pgmhip.h "Marginals by loopy belief propagation",
pgmpy_amd/csrc/pgmlbp.hip): sum-product loopy belief propagation on a Markov network for a batch of instances in one
launch.

A plan is made from the nodes' cardinalities, the factor scopes (1 to 3 node indices each) and, for the
deduplication of equal tables, the factor tables on the host; the node terms are an argument of a run.
"""
import ctypes

import numpy as np

from .. import _native as N
from .._plan import Plan, flat_tensor


class LbpPlan(Plan):
    _destroy = "pgm_lbp_plan_destroy"

    def __init__(self, card, scopes, theta=None):
        L = N.load_library()  # building and inspecting a plan needs no device
        self.card = [int(k) for k in card]
        self.scopes = [tuple(int(v) for v in s) for s in scopes]
        n, m = len(self.card), len(self.scopes)
        c_card = (ctypes.c_int32 * max(n, 1))(*self.card)
        c_nv = (ctypes.c_int32 * max(m, 1))(*[len(s) for s in self.scopes])
        c_vars = (ctypes.c_int32 * max(3 * m, 1))()
        for i, s in enumerate(self.scopes):
            for j, v in enumerate(s[:3]):
                c_vars[3 * i + j] = v
        self.theta = None if theta is None else np.ascontiguousarray(theta, dtype=np.float64).reshape(-1)
        c_theta = None if self.theta is None else self.theta.ctypes.data_as(ctypes.c_void_p)
        self._h = ctypes.c_void_p()
        N.check(L.pgm_lbp_plan_create(c_card, n, c_nv, c_vars, m, c_theta, ctypes.byref(self._h)), "lbp_plan_create")
        self.info = N.LbpInfo()
        node_off, f_off = (ctypes.c_int32 * (n + 1))(), (ctypes.c_int32 * (m + 1))()
        msg_off = (ctypes.c_int32 * (sum(len(s) for s in self.scopes) + 1))()
        N.check(L.pgm_lbp_plan_info(self._h, ctypes.byref(self.info), node_off, f_off, msg_off), "lbp_plan_info")
        if self.theta is not None and self.theta.size != self.info.n_theta:
            raise ValueError(f"theta has {self.theta.size} entries, the scopes need {self.info.n_theta}")
        self.node_offsets, self.factor_offsets, self.msg_offsets = list(node_off), list(f_off), list(msg_off)
        self.n_nodes, self.n_unary, self.n_theta = n, int(self.info.n_unary), int(self.info.n_theta)
        self.n_pairs, self.n_msg, self.state_len = int(self.info.n_pairs), int(self.info.n_msg), int(self.info.state_len)
        self.n_tables_unique, self.theta_in_lds = int(self.info.n_tables_unique), int(self.info.theta_in_lds)

    def run(self, unaries, theta, n_iter, tol=0.0, damping=0.0, state=None, want_beliefs=False, want_state=False):
        """Run every row of the device `unaries` [B, n_unary] (fp64) with the factor tables `theta` [n_theta] for at
        most `n_iter` iterations, from the messages `state` [B, state_len] when given.  Returns device tensors
        (marginals [B, n_unary], values [B, 2]: Bethe log Z and last residual, iters [B] int32, the factor beliefs
        [B, n_theta] or None, the state [B, state_len] or None)."""
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
        new = lambda cols: torch.empty((B, cols), dtype=torch.float64, device=dev)
        marginals, values = new(self.n_unary), new(N.LBP_VALUES)
        iters = torch.empty(B, dtype=torch.int32, device=dev)
        beliefs = new(self.n_theta) if want_beliefs else None
        out = new(self.state_len) if want_state else None
        N.check(L.pgm_lbp_run(self._h, N.ptr(unaries), N.ptr(theta), B, int(n_iter), float(tol), float(damping), N.ptr(state),
                              N.ptr(marginals), N.ptr(values), N.ptr(iters), N.ptr(beliefs), N.ptr(out), N.stream_handle()),
                "lbp_run")
        return marginals, values, iters, beliefs, out
