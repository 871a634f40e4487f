"""Binding of the pgm_mnpl_* entry points (include/pgmhip.h "Pseudo-likelihood of a Markov network",
pgmpy_amd/csrc/pgmmnpl.hip): the log pseudo-likelihood of a Markov network and its gradient in the log-potentials,
from the count tables of the nodes' blanket families.

A factor is ``(columns, cardinalities)`` in the C order of its table, as GibbsPlan takes it; theta and the gradient
share the flat layout of the factors: factor f occupies ``[offsets[f], offsets[f] + sizes[f])``.
"""
import ctypes

from .. import _native as N
from .._plan import Plan, family_array, flat_tensor
from ._fit import FitPlan


class MnplPlan(Plan):
    _destroy = "pgm_mnpl_plan_destroy"

    def __init__(self, factors, card):
        L = N.load_library()  # building and inspecting a plan needs no device
        self.factors, fams = family_array(factors)
        self.card = [int(k) for k in card]
        self.n_cols = n = len(self.card)
        m = len(self.factors)
        self._h = ctypes.c_void_p()
        cards = (ctypes.c_int32 * max(n, 1))(*self.card)
        N.check(L.pgm_mnpl_plan_create(fams, m, cards, n, ctypes.byref(self._h)), "mnpl_plan_create")
        self.info = N.MnplInfo()
        N.check(L.pgm_mnpl_plan_info(self._h, ctypes.byref(self.info), None, None, None, None, None, None), "mnpl_plan_info")
        blanket = (N.FitFamily * n)()
        count_off, node_lds = (ctypes.c_int64 * (n + 1))(), (ctypes.c_int64 * n)()
        fac_off, part_off = (ctypes.c_int64 * (m + 1))(), (ctypes.c_int64 * (m + 1))()
        slots = (ctypes.c_int64 * (3 * int(self.info.n_incidences)))()
        N.check(L.pgm_mnpl_plan_info(self._h, None, blanket, count_off, fac_off, part_off, node_lds, slots), "mnpl_plan_info")
        # the blanket family of every node, as FitPlan takes them: (node, blanket columns ascending)
        self.families = [(list(b.col[:b.n_vars]), list(b.card[:b.n_vars])) for b in blanket]
        self.count_offsets, self.node_lds = list(count_off), list(node_lds)
        self.offsets, self.part_offsets = list(fac_off)[:m], list(part_off)
        self.sizes = [fac_off[f + 1] - fac_off[f] for f in range(m)]
        self.slots = [tuple(slots[3 * e:3 * e + 3]) for e in range(int(self.info.n_incidences))]
        self.n_theta, self.n_counts, self.n_parts = int(self.info.n_theta), int(self.info.n_counts), int(self.info.n_parts)
        self._fit = None

    def fit_plan(self):
        """The FitPlan of the blanket families: its int64 tables are what eval reads."""
        if self._fit is None:
            self._fit = FitPlan(self.families)
            if self._fit.offsets != self.count_offsets[:-1] or self._fit.total_bins != self.n_counts:
                raise RuntimeError("the fit plan lays the blanket families out differently from the pseudo-likelihood plan")
        return self._fit

    def eval(self, counts, theta, l2=0.0, want_grad=True, want_node_values=False):
        """(value [1], grad [n_theta] or None, node_values [n_cols] or None), fp64 device tensors, of the log
        pseudo-likelihood less l2 / 2 |theta|^2 at the device `theta` [n_theta], from the int64 device `counts`
        (fit_plan().count(codes)).  Two launches, no synchronisation."""
        import torch

        L = N.lib()
        flat_tensor("counts", counts, self.n_counts, torch.int64, "int64")
        flat_tensor("theta", theta, self.n_theta)
        new = lambda n: torch.empty(n, dtype=torch.float64, device=theta.device)
        value = new(1)
        grad = new(self.n_theta) if want_grad else None
        node_values = new(self.n_cols) if want_node_values else None
        N.check(L.pgm_mnpl_eval(self._h, N.ptr(counts), N.ptr(theta), float(l2), N.ptr(value), N.ptr(grad),
                                N.ptr(node_values), N.stream_handle()), "mnpl_eval")
        return value, grad, node_values
