"""Binding of the pgm_sample_* entry points (include/pgmhip.h, pgmpy_amd/csrc/pgmsample.hip): the running
sums of every CPD column in one launch and every node of every sampled row in one more.

A family is ``(columns, cardinalities)``: the code column and cardinality of the node, then of each
parent in the CPD's order; the families come in a topological order.  The values and the running sums
share the fit plan's flat layout: family f occupies ``[offsets[f], offsets[f] + sizes[f])``, shaped
``[node_card, prod(parent_card)]`` in C order.
"""
import ctypes

import numpy as np

from .. import _native as N

FREE, GIVEN, OBSERVED = N.SAMPLE_FREE, N.SAMPLE_GIVEN, N.SAMPLE_OBSERVED
MASK64 = (1 << 64) - 1


def family_array(families):
    families = [(list(cols), list(cards)) for cols, cards in families]
    fams = (N.FitFamily * max(len(families), 1))()
    for f, (cols, cards) in enumerate(families):
        if len(cols) != len(cards):
            raise ValueError(f"family {f}: {len(cols)} columns, {len(cards)} cardinalities")
        if not 1 <= len(cols) <= N.PGM_MAX_DIMS:
            raise ValueError(f"family {f} has {len(cols) - 1} parents; at most {N.PGM_MAX_DIMS - 1} are supported")
        fams[f].n_vars = len(cols)
        for v, (c, k) in enumerate(zip(cols, cards)):
            fams[f].col[v], fams[f].card[v] = int(c), int(k)
    return families, fams


class SamplePlan:
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

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                N.load_library().pgm_sample_plan_destroy(h)
            except Exception:
                pass
            self._h = None

    def launch_info(self, codes=None, ld=0, row0=0, weights=None, uniforms=None, offsets=None, sizes=None):
        """SampleInfo for a launch (pgm_sample_plan_info; no device).  The pointers are addresses (ints
        or None): only NULL and alignment matter."""
        info = N.SampleInfo()
        P = ctypes.c_void_p
        N.check(N.load_library().pgm_sample_plan_info(self._h, P(codes), int(ld), int(row0), P(weights), P(uniforms),
                                                      ctypes.byref(info), offsets, sizes), "sample_plan_info")
        return info

    def table(self, flat, f):
        """Family f's [node_card, columns] view of a flat buffer (device tensor or ndarray)."""
        card = self.families[f][1][0]
        return flat[self.offsets[f]:self.offsets[f] + self.sizes[f]].reshape(card, self.sizes[f] // card)

    def cdf(self, values, out=None):
        """The running sums of every CPD column of the flat fp64 device buffer `values`.  Raises
        ValueError when a column's total is not finite or not > 0."""
        import torch

        L = N.lib()
        if values.dtype != torch.float64 or values.numel() < self.total_bins or not values.is_contiguous():
            raise ValueError(f"values must be a contiguous fp64 device tensor of {self.total_bins} entries")
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
        if codes.dtype != torch.uint8 or codes.dim() != 2 or not codes.is_contiguous():
            raise ValueError("codes must be a contiguous [n_cols, ld] uint8 device tensor")
        n_cols, ld = int(codes.shape[0]), int(codes.shape[1])
        n_rows = ld - row0 if n_rows is None else int(n_rows)
        for name, t in (("cdf", cdf), ("values", values)):
            if t is not None and (t.dtype != torch.float64 or t.numel() < self.total_bins or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous fp64 device tensor of {self.total_bins} entries")
        if weights is not None and (weights.dtype != torch.float64 or weights.numel() < ld or not weights.is_contiguous()):
            raise ValueError("weights must be a contiguous fp64 device tensor with one entry per row of codes")
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
