"""Binding of the pgm_sample_* entry points (include/pgmhip.h, pgmpy_amd/csrc/pgmsample.hip): the running
sums of every CPD column in one launch and every node of every sampled row in one more.

A family is ``(columns, cardinalities)``: the code column and cardinality of the node, then of each
parent in the CPD's order; the families come in a topological order.  The values and the running sums
share the fit plan's flat layout: family f occupies ``[offsets[f], offsets[f] + sizes[f])``, shaped
``[node_card, prod(parent_card)]`` in C order.
"""
import ctypes
from collections import namedtuple

import numpy as np

from .. import _native as N
from .._plan import MASK64, Plan, codes_window, family_array, flat_tensor

FREE, GIVEN, OBSERVED = N.SAMPLE_FREE, N.SAMPLE_GIVEN, N.SAMPLE_OBSERVED

# what SamplePlan.posterior returns: device tensors indexed by evidence row (post, log_evidence, ess: None
# when not asked for); acc holds the uint64 sums as int64 (they stay below 2^62)
Posterior = namedtuple("Posterior", ["acc", "scale", "post", "log_evidence", "ess"])


class SamplePlan(Plan):
    _destroy = "pgm_sample_plan_destroy"

    def __init__(self, families):
        L = N.load_library()  # building and inspecting a plan needs no device
        self.families, fams = family_array(families)
        self._h = ctypes.c_void_p()
        N.check(L.pgm_sample_plan_create(fams, len(self.families), ctypes.byref(self._h)), "sample_plan_create")
        n = len(self.families)
        off, size = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
        self.info = self.launch_info(offsets=off, sizes=size)
        self.offsets, self.sizes = list(off), list(size)
        self.total_bins = int(self.info.total_bins)
        self.n_cols = int(self.info.n_cols)

    def launch_info(self, codes=None, ld=0, row0=0, weights=None, uniforms=None, offsets=None, sizes=None):
        """SampleInfo for a launch (pgm_sample_plan_info; no device).  The pointers are addresses (ints
        or None): only NULL and alignment matter."""
        info = N.SampleInfo()
        P = ctypes.c_void_p
        N.check(N.load_library().pgm_sample_plan_info(self._h, P(codes), int(ld), int(row0), P(weights), P(uniforms),
                                                      ctypes.byref(info), offsets, sizes), "sample_plan_info")
        return info

    def cdf(self, values, out=None):
        """The running sums of every CPD column of the flat fp64 device buffer `values`.  Raises
        ValueError when a column's total is not finite or not > 0."""
        import torch

        L = N.lib()
        flat_tensor("values", values, self.total_bins)
        if out is None:
            out = torch.empty(self.total_bins, dtype=torch.float64, device=values.device)
        N.check(L.pgm_sample_cdf(self._h, N.ptr(values), N.ptr(out), N.stream_handle()), "sample_cdf")
        return out

    def forward(self, cdf, codes, n_rows=None, row0=0, first_row=0, seed=0, modes=None, values=None, weights=None,
                uniforms=None):
        """Draw the rows [row0, row0 + n_rows) of the device codes [n_cols, ld] (uint8) as the rows
        [first_row, first_row + n_rows) of the stream of `seed`.  modes: one of FREE / GIVEN / OBSERVED
        per family (None: all FREE).  weights: an fp64 device tensor of ld entries to fill (needs
        values).  uniforms: an fp64 device tensor [n_cols, ld] that replaces the generator.  Raises
        IndexError when a given code is neither 255 nor a state."""
        import torch

        L = N.lib()
        n_cols, ld, n_rows = codes_window(codes, n_rows, row0)
        for name, t in (("cdf", cdf), ("values", values)):
            if t is not None:
                flat_tensor(name, t, self.total_bins)
        if weights is not None:
            flat_tensor("weights", weights, ld, entries="with one entry per row of codes")
        if uniforms is not None and (uniforms.dtype != torch.float64 or tuple(uniforms.shape) != (n_cols, ld)
                                     or not uniforms.is_contiguous()):
            raise ValueError("uniforms must be a contiguous fp64 device tensor of the shape of codes")
        m = None
        if modes is not None:
            m = np.ascontiguousarray(modes, dtype=np.uint8)
            if m.shape != (len(self.families),):
                raise ValueError(f"modes must have one entry per family ({len(self.families)})")
        N.check(L.pgm_sample_forward(self._h, N.ptr(values), N.ptr(cdf),
                                     None if m is None else m.ctypes.data_as(ctypes.c_void_p), N.ptr(codes), n_cols, ld,
                                     int(row0), n_rows, int(first_row), int(seed) & MASK64, N.ptr(weights),
                                     N.ptr(uniforms), N.stream_handle()), "sample_forward")
        return codes

    def posterior_info(self, targets, n_rows, n_samples, block=0):
        """LwInfo of a posterior call with the FitPlan `targets` (pgm_sample_posterior_info; no device):
        workgroup size, K, LDS bytes, workgroups.  Raises ValueError when no workgroup size fits the LDS
        budget."""
        info = N.LwInfo()
        N.check(N.load_library().pgm_sample_posterior_info(self._h, targets._h, int(n_rows), int(n_samples), int(block),
                                                           ctypes.byref(info)), "sample_posterior_info")
        return info

    def posterior(self, targets, values, cdf, evidence, n_samples, n_rows=None, row0=0, first_row=0, seed=0,
                  modes=None, block=0, post=True, log_evidence=True, ess=True):
        """Likelihood weighting for the evidence rows [row0, row0 + n_rows) of the device codes `evidence`
        [n_cols, ld] (uint8, 255: not observed): n_samples samples per row, histogrammed into the tables of
        the FitPlan `targets` (pgm_sample_posterior).  Sample s of row r is stream row
        first_row + r * n_samples + s of `seed`.  modes as in forward.  block: 0 automatic, 64 / 128 / 256
        forces the workgroup size.  Returns a Posterior of device tensors [n_rows, total_bins] / [n_rows].
        Raises IndexError when an evidence code is neither 255 nor a state (that row's post is NaN)."""
        import torch

        L = N.lib()
        n_cols, ld, n_rows = codes_window(evidence, n_rows, row0)
        flat_tensor("cdf", cdf, self.total_bins)
        flat_tensor("values", values, self.total_bins)
        m = None
        if modes is not None:
            m = np.ascontiguousarray(modes, dtype=np.uint8)
            if m.shape != (len(self.families),):
                raise ValueError(f"modes must have one entry per family ({len(self.families)})")
        rows, bins, dev = max(n_rows, 0), targets.total_bins, evidence.device
        acc = torch.empty((rows, bins), dtype=torch.int64, device=dev)
        scale = torch.empty(rows, dtype=torch.float64, device=dev)
        out_post = torch.empty((rows, bins), dtype=torch.float64, device=dev) if post else None
        out_le = torch.empty(rows, dtype=torch.float64, device=dev) if log_evidence else None
        out_ess = torch.empty(rows, dtype=torch.float64, device=dev) if ess else None
        out = Posterior(acc, scale, out_post, out_le, out_ess)
        try:
            N.check(L.pgm_sample_posterior(self._h, targets._h, N.ptr(values), N.ptr(cdf),
                                           None if m is None else m.ctypes.data_as(ctypes.c_void_p), N.ptr(evidence),
                                           n_cols, ld, int(row0), n_rows, int(n_samples), int(first_row),
                                           int(seed) & MASK64, int(block), N.ptr(acc), N.ptr(scale), N.ptr(out_post),
                                           N.ptr(out_le), N.ptr(out_ess), N.stream_handle()), "sample_posterior")
        except IndexError as e:
            e.posterior = out  # the other rows are complete
            raise
        return out
