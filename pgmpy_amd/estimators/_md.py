"""Binding of the pgm_md_* entry points (include/pgmhip.h "Junction-tree potentials by mirror descent",
pgmpy_amd/csrc/pgmmd.hip): the clique log-potentials of a junction tree fitted to measured marginals by entropic
mirror descent, a batch of target rows in one launch.

A plan is made from the variables' cardinalities, the cliques and marginals as tuples of variable indices and the
tree's edges as pairs of clique indices; building and inspecting it needs no device.
"""
import ctypes

import numpy as np

from .. import _native as N
from .._plan import Plan, flat_tensor

METRICS = {"L1": N.MD_L1, "L2": N.MD_L2}


def _scopes(scopes):
    """(int32 counts, int32 [n][MD_MAX_VARS] variables) of tuples of variable indices; a longer scope keeps its
    count, which the library rejects."""
    n = len(scopes)
    nv = (ctypes.c_int32 * max(n, 1))(*[len(s) for s in scopes])
    flat = (ctypes.c_int32 * max(N.MD_MAX_VARS * n, 1))()
    for i, s in enumerate(scopes):
        for k, v in enumerate(s[:N.MD_MAX_VARS]):
            flat[N.MD_MAX_VARS * i + k] = v
    return nv, flat


class MdPlan(Plan):
    _destroy = "pgm_md_plan_destroy"

    def __init__(self, card, cliques, edges, marginals):
        L = N.load_library()
        self.card = [int(k) for k in card]
        self.cliques = [tuple(int(v) for v in c) for c in cliques]
        self.edges = [(int(a), int(b)) for a, b in edges]
        self.marginals = [tuple(int(v) for v in m) for m in marginals]
        nc, nm, ne = len(self.cliques), len(self.marginals), len(self.edges)
        c_card = (ctypes.c_int32 * max(len(self.card), 1))(*self.card)
        c_nv, c_vars = _scopes(self.cliques)
        m_nv, m_vars = _scopes(self.marginals)
        c_edges = (ctypes.c_int32 * max(2 * ne, 1))(*[x for e in self.edges for x in e])
        self._h = ctypes.c_void_p()
        N.check(L.pgm_md_plan_create(c_card, len(self.card), c_nv, c_vars, nc, c_edges, ne, m_nv, m_vars, nm,
                                     ctypes.byref(self._h)), "md_plan_create")
        i32 = lambda n: (ctypes.c_int32 * n)()
        outs = [i32(nc + 1), i32(nc), i32(nc), i32(nc + 1), i32(2 * N.MD_MAX_VARS * nc), i32(nm), i32(nm + 1),
                i32(N.MD_MAX_VARS * nm)]
        self.info = N.MdInfo()
        N.check(L.pgm_md_plan_info(self._h, ctypes.byref(self.info), *outs), "md_plan_info")
        (self.clique_offsets, self.parent, self.level, self.sep_offsets, sep_st, self.owner, self.y_offsets,
         m_st) = [list(o) for o in outs]
        self.sep_strides = np.array(sep_st, dtype=np.int64).reshape(nc, 2, N.MD_MAX_VARS)
        self.marginal_strides = np.array(m_st, dtype=np.int64).reshape(nm, N.MD_MAX_VARS)
        self.n_cells, self.n_sep, self.n_y = int(self.info.n_cells), int(self.info.n_sep), int(self.info.n_y)
        self.depth = int(self.info.depth)

    @property
    def tier(self):
        N.check(N.load_library().pgm_md_plan_info(self._h, ctypes.byref(self.info), *[None] * 8), "md_plan_info")
        return int(self.info.tier)

    def set_tier(self, tier):
        """Force N.MD_TIER_LDS or N.MD_TIER_GLOBAL (tests), or go back to N.MD_TIER_AUTO."""
        N.check(N.load_library().pgm_md_set_tier(self._h, int(tier)), "md_set_tier")

    def run(self, targets, totals, theta, metric="L2", iterations=100, stepsize=None):
        """Fit every row of the device `targets` [B, n_y] (fp64; row b sums to totals[b] per marginal) from the
        log-potentials `theta` [B or 1, n_cells].  `stepsize` as MirrorDescentEstimator.estimate reads it: None is the
        line search from 1 / total^2, a float a fixed step of that value (0 and negative ones as they stand; NaN and infinity
        raise ValueError), anything else a fixed step of 1 / total^2.  Returns device
        tensors (theta [B, n_cells], mu [B, n_cells], values [B, 2]: the loss and the final alpha, trials [B, 2]
        int32: trials taken and trials rejected)."""
        import torch

        if metric not in METRICS:
            raise ValueError("Metric must be one of L1 or L2.")
        L = N.lib()
        if targets.dim() != 2 or int(targets.shape[1]) != self.n_y:
            raise ValueError(f"targets must be [B, {self.n_y}]: one row of marginal cells per instance")
        B = int(targets.shape[0])
        if theta.dim() != 2 or int(theta.shape[1]) != self.n_cells or int(theta.shape[0]) not in (1, B):
            raise ValueError(f"theta must be [{B} or 1, {self.n_cells}]")
        flat_tensor("targets", targets, B * self.n_y)
        flat_tensor("totals", totals, B)
        flat_tensor("theta", theta, int(theta.shape[0]) * self.n_cells)
        dev = targets.device
        new = lambda cols: torch.empty((B, cols), dtype=torch.float64, device=dev)
        theta_out, mu, values = new(self.n_cells), new(self.n_cells), new(N.MD_VALUES)
        trials = torch.empty((B, 2), dtype=torch.int32, device=dev)
        scratch = new(int(self.info.state_len)) if self.tier == N.MD_TIER_GLOBAL else None
        fixed = isinstance(stepsize, float)  # the reference's three readings of `stepsize`
        mode = N.MD_STEP_FIXED if fixed else N.MD_STEP_SEARCH if stepsize is None else N.MD_STEP_DEFAULT
        N.check(L.pgm_md_run(self._h, N.ptr(targets), N.ptr(totals), N.ptr(theta), int(theta.shape[0]), B, METRICS[metric],
                             int(iterations), stepsize if fixed else 0.0, mode, N.ptr(scratch), N.ptr(theta_out), N.ptr(mu), N.ptr(values), N.ptr(trials), N.stream_handle()),
                "md_run")
        return theta_out, mu, values, trials
