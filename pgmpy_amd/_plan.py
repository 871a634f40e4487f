"""What the bindings of the plan handles share (estimators/_fit.py FitPlan, sampling/_sample.py SamplePlan,
sampling/_gibbs.py GibbsPlan): the pgm_fit_family array, the handle and its destruction, the flat table
view, and the argument checks of a launch.  Calls on one plan must not overlap (include/pgmhip.h)."""
from . import _native as N

MASK64 = (1 << 64) - 1  # a seed as the library's uint64


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


def codes_window(codes, n, row0):
    """(n_cols, ld, n) of a launch over the rows [row0, row0 + n) of `codes`; n None: up to the last row."""
    import torch

    if codes.dtype != torch.uint8 or codes.dim() != 2 or not codes.is_contiguous():
        raise ValueError("codes must be a contiguous [n_cols, ld] uint8 device tensor")
    n_cols, ld = int(codes.shape[0]), int(codes.shape[1])
    return n_cols, ld, (ld - row0 if n is None else int(n))


def flat_tensor(name, t, n, dtype=None, label="fp64", entries=None):
    """`t` is a contiguous device tensor of `dtype` (fp64) with at least n entries; `label` and `entries`
    word the error ("of n entries" when None)."""
    import torch

    if t.dtype != (dtype or torch.float64) or t.numel() < n or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {label} device tensor {entries or f'of {n} entries'}")


class Plan:
    """A plan handle `_h` of the library; the subclass names its pgm_*_plan_destroy."""
    _destroy = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                getattr(N.load_library(), self._destroy)(h)
            except Exception:
                pass
            self._h = None

    def table(self, flat, f):
        """Family f's [node_card, columns] view of a flat buffer (device tensor or ndarray)."""
        card = self.families[f][1][0]
        return flat[self.offsets[f]:self.offsets[f] + self.sizes[f]].reshape(card, self.sizes[f] // card)
