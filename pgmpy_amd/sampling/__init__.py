"""BayesianModelSampling (mirror of pgmpy/sampling/Sampling.py:17-406) on the device.

The reference draws node by node from numpy's global stream, grouped by the unique parent
configurations of the rows drawn so far.  Here one kernel launch (pgm_sample_forward) draws every node
of every row into column-major uint8 state codes ``[n_nodes, ld]`` — the layout FitPlan.count and the
fused row plan of predict read — from a counter-based stream: the uniform of stream row r and code
column c is a pure function of (seed, r, c) (Philox4x32-10).  Samples equal the reference's
in distribution, not in value.

The plan, the flat CPD values and their running sums are cached on the model and rebuilt when the
model's change counter or any factor's values change.  There is no CPU path: drawing raises
``NativeUnavailable`` without the library or a device; the argument checks run before that.
"""
import os
import threading
import weakref
from collections import namedtuple

import networkx as nx
import numpy as np

from .. import engine as E
from ._sample import FREE, GIVEN, MASK64, OBSERVED, SamplePlan

State = namedtuple("State", ["var", "state"])

MISSING = 255
WEIGHT = "_weight"
REJECTION_FLOOR = 0.01     # the reference's lower bound on the acceptance estimate
REJECTION_EMPTY_BATCHES = 64  # consecutive batches without an accepted row before giving up
REJECTION_MAX_BYTES = 1 << 31  # code bytes of one batch


def fresh_seed():
    return int.from_bytes(os.urandom(8), "little")


def column_order(model):
    """The code column of every node: sorted(model.nodes()), unless the model carries an explicit order
    (simulate's rewritten models keep the original columns and append the nodes they add)."""
    order = model.__dict__.get("_sample_columns")
    return list(order) if order is not None else sorted(model.nodes())


def plan_order(model, col):
    """The order the kernel walks the nodes in: topological, ties broken by code column."""
    return list(nx.lexicographical_topological_sort(model, key=col.__getitem__))


class _Compiled:
    """The sampler's view of a model: columns, families in plan order, the plan (host only)."""

    def __init__(self, model):
        self.nodes = column_order(model)
        self.col = {v: i for i, v in enumerate(self.nodes)}
        if len(self.col) != len(self.nodes) or set(self.nodes) != set(model.nodes()):
            raise ValueError("the sampler's column order must list every node of the model once")
        self.order = plan_order(model, self.col)
        self.family_of = {v: f for f, v in enumerate(self.order)}
        self.cpds = [model.get_cpds(v) for v in self.order]
        for v, c in zip(self.order, self.cpds):
            if c is None:
                raise ValueError(f"No CPD associated with {v}")
            if set(c.variables[1:]) != set(model.get_parents(v)):
                raise ValueError(f"CPD associated with {v} doesn't have proper parents associated with it.")
        self.lock = threading.Lock()  # the plan's mode array on the device is per handle: one launch at a time
        self.card = {v: int(c.cardinality[0]) for v, c in zip(self.order, self.cpds)}
        for v, k in self.card.items():
            if k >= MISSING:
                raise ValueError(f"variable {v} has {k} states; uint8 codes hold at most 254")
        self.plan = SamplePlan([([self.col[u] for u in c.variables], [int(k) for k in c.cardinality])
                                for c in self.cpds])
        self.values = self.cdf = None
        self._targets = {}  # target variable lists -> the FitPlan of their tables (posterior_codes)

    def target_plan(self, targets):
        """The FitPlan whose families are the tables of `targets` (a tuple of tuples of variables), cached."""
        from ..estimators._fit import FitPlan

        plan = self._targets.get(targets)
        if plan is None:
            if len(self._targets) >= 64:
                self._targets.clear()
            plan = self._targets[targets] = FitPlan([([self.col[v] for v in t], [self.card[v] for v in t])
                                                     for t in targets])
        return plan

    def posterior_bin_budget(self):
        """The most target bins a posterior call can take: the LDS budget less the smallest workgroup's codes."""
        from .. import _native as N

        return max((N.LW_LDS_BUDGET - 2048 - 64 * self.plan.n_cols) // 8, 0)

    def tables(self):
        """(values, running sums) on the device; CPDs that are already there (fit) are not copied to
        the host."""
        if self.cdf is None:
            import torch

            if all(c._dev is None for c in self.cpds):  # one upload
                self.values = E.to_device(np.concatenate([np.asarray(c._values_readonly()).ravel() for c in self.cpds]))
            else:
                self.values = torch.cat([c._d().reshape(-1) for c in self.cpds])
            self.cdf = self.plan.cdf(self.values)
        return self.values, self.cdf


_CACHE = weakref.WeakKeyDictionary()  # model -> (key, _Compiled): beside the model, so the model still pickles


def compiled(model):
    """The model's cached _Compiled: rebuilt when the model's change counter (_bump) or any factor's
    values have changed since it was built."""
    from ..factors.discrete.DiscreteFactor import values_epoch

    key = (model.__dict__.get("_epoch", 0), values_epoch())
    hit = _CACHE.get(model)
    if hit is None or hit[0] != key:
        hit = _CACHE[model] = (key, _Compiled(model))
    return hit[1]


class BayesianModelSampling:
    def __init__(self, model):
        from ..models import DiscreteBayesianNetwork

        if not isinstance(model, DiscreteBayesianNetwork):
            raise TypeError(f"Model expected type: DiscreteBayesianNetwork, got type: {type(model)}")
        self.model = model
        self.topological_order = list(nx.topological_sort(model))

    # ------------------------------------------------------------------ device level
    @E.serialized
    def forward_sample_codes(self, size, seed=None, first_row=0, partial_codes=None, modes=None, weights=False):
        """(uint8 device codes [n_nodes, size], nodes[, fp64 device weights]): rows [first_row,
        first_row + size) of the stream of `seed`, columns in sorted(model.nodes()) order.

        partial_codes: {node: a state code or an array of `size` codes (255: draw)} taken as given;
        modes: {node: GIVEN | OBSERVED} for them (default GIVEN; OBSERVED multiplies the row's weight
        by p(code | parents)).  seed=None takes fresh entropy."""
        import torch

        size, first_row = int(size), int(first_row)
        if size < 0 or first_row < 0:
            raise ValueError(f"size and first_row must be non-negative. Got {size}, {first_row}")
        partial_codes = dict(partial_codes or {})
        modes = dict(modes or {})
        for v in list(partial_codes) + list(modes):
            if v not in self.model.nodes():
                raise ValueError(f"Node {v} not in the model")
        for v in modes:
            if v not in partial_codes:
                raise ValueError(f"a mode is given for {v} but no codes")
            if modes[v] not in (FREE, GIVEN, OBSERVED):
                raise ValueError(f"mode of {v} must be FREE (0), GIVEN (1) or OBSERVED (2). Got {modes[v]}")
        c = compiled(self.model)
        fmodes = np.zeros(len(c.order), dtype=np.uint8)
        for v in partial_codes:
            fmodes[c.family_of[v]] = modes.get(v, GIVEN)
        seed = fresh_seed() if seed is None else int(seed) & MASK64
        values, cdf = c.tables()
        codes = torch.empty((len(c.nodes), size), dtype=torch.uint8, device=cdf.device)
        for v, given in partial_codes.items():
            row = codes[c.col[v]]
            if isinstance(given, torch.Tensor):
                if given.numel() != size:
                    raise ValueError(f"partial codes of {v} have {given.numel()} rows, {size} are drawn")
                row.copy_(given.reshape(-1))
            elif np.ndim(given) == 0:
                row.fill_(int(given))
            else:
                g = np.ascontiguousarray(given, dtype=np.uint8).reshape(-1)
                if g.size != size:
                    raise ValueError(f"partial codes of {v} have {g.size} rows, {size} are drawn")
                row.copy_(E.to_device_raw(g))
        w = torch.empty(size, dtype=torch.float64, device=cdf.device) if weights else None
        if size:
            with c.lock:  # the call returns after the launch has finished (it reads the bad-code flag back)
                c.plan.forward(cdf, codes, first_row=first_row, seed=seed, modes=fmodes if partial_codes else None,
                               values=values if weights else None, weights=w)
        return (codes, c.nodes, w) if weights else (codes, c.nodes)

    @E.serialized
    def posterior_codes(self, evidence_codes, targets, n_samples, seed=None, first_row=0, modes=None, block=0):
        """Likelihood weighting for a batch of evidence rows in one fused launch sequence
        (pgm_sample_posterior): no sampled code is written to memory.

        evidence_codes: uint8 device codes [n_nodes, R], columns in sorted(model.nodes()) order, 255 = not
        observed.  targets: a list whose entries are a variable (its marginal) or a list of variables (one
        joint table over them in C order, the first variable slowest).  modes: {node: GIVEN | OBSERVED} for the nodes whose
        evidence counts (default: every node OBSERVED; a 255 cell is drawn whatever the mode).  Sample s of
        row r is stream row first_row + r * n_samples + s of `seed` (None: fresh entropy).

        Returns (Posterior, layout): the Posterior's device tensors are indexed by evidence row, layout is
        [(variables, offset, shape)] per target into the bins axis."""
        n_samples, first_row = int(n_samples), int(first_row)
        c = compiled(self.model)
        targets = [tuple(t) if isinstance(t, list) else (t,) for t in targets]
        if not targets:
            raise ValueError("posterior_codes needs at least one target")
        for t in targets:
            for v in t:
                if v not in c.col:
                    raise ValueError(f"Node {v} not in the model")
            if len(set(t)) != len(t):
                raise ValueError(f"a target lists a variable twice: {list(t)}")
        fmodes = np.full(len(c.order), OBSERVED, dtype=np.uint8)
        if modes is not None:
            fmodes[:] = FREE
            for v, m in dict(modes).items():
                if v not in c.col:
                    raise ValueError(f"Node {v} not in the model")
                if m not in (FREE, GIVEN, OBSERVED):
                    raise ValueError(f"mode of {v} must be FREE (0), GIVEN (1) or OBSERVED (2). Got {m}")
                fmodes[c.family_of[v]] = m
        plan = c.target_plan(tuple(targets))
        seed = fresh_seed() if seed is None else int(seed) & MASK64
        values, cdf = c.tables()
        with c.lock:  # the call returns after the launches have finished (it reads the bad-code flag back)
            out = c.plan.posterior(plan, values, cdf, evidence_codes, n_samples, first_row=first_row, seed=seed,
                                   modes=fmodes, block=block)
        layout = [(list(t), plan.offsets[i], tuple(c.card[v] for v in t)) for i, t in enumerate(targets)]
        return out, layout

    # ------------------------------------------------------------------ helpers
    def _partial(self, partial_samples, size):
        """{node: uint8 codes} of a frame of state names (NaN: draw), with the shape check."""
        if partial_samples is None:
            return {}
        if partial_samples.shape[0] != size:
            raise ValueError(f"partial_samples must have {size} rows (the number of samples). Got {partial_samples.shape[0]}")
        from ..inference.batch import encode_states

        columns = [v for v in partial_samples.columns if v in self.model.nodes()]
        unknown = [v for v in partial_samples.columns if v not in self.model.nodes()]
        if unknown:
            raise ValueError(f"partial_samples has columns that are not nodes of the model: {unknown}")
        states = self.model.states
        codes = encode_states({v: states[v] for v in columns}, partial_samples, columns)
        return {v: codes[j] for j, v in enumerate(columns)}

    def _evidence(self, evidence):
        """{node: state code} of [(var, state name)], with the reference's errors."""
        out = {}
        for var, state in evidence:
            if var not in self.model.nodes():
                raise ValueError(f"Evidence variable {var} not in the model")
            out[var] = self.model.get_cpds(var).get_state_no(var, state)
        return out

    def _frame(self, codes, nodes, include_latents, weights=None):
        """State names of host codes [n_nodes, n], columns in model.nodes() order."""
        import pandas as pd

        states = self.model.states
        pos = {v: i for i, v in enumerate(nodes)}
        keep = [v for v in self.model.nodes() if include_latents or v not in self.model.latents]
        data = {}
        for v in keep:
            lut = np.empty(len(states[v]), dtype=object)  # element-wise: a state name may be a tuple
            lut[:] = list(states[v])
            data[v] = lut[codes[pos[v]]]
        df = pd.DataFrame(data, columns=keep)
        if weights is not None:
            df[WEIGHT] = weights
        return df

    # ------------------------------------------------------------------ the reference's entry points
    def forward_sample(self, size=1, include_latents=False, seed=None, show_progress=True, partial_samples=None,
                       n_jobs=-1):
        """`size` samples of the joint distribution (Sampling.py:30-144): a DataFrame of state names,
        columns in model.nodes() order, latents dropped unless asked for.  partial_samples: a frame of
        state names for some of the variables, taken as given.  show_progress and n_jobs are accepted
        and ignored."""
        from ..inference.batch import download

        partial = self._partial(partial_samples, int(size))
        codes, nodes = self.forward_sample_codes(size, seed=seed, partial_codes=partial)
        return self._frame(download(codes), nodes, include_latents)

    def likelihood_weighted_sample(self, evidence=[], size=1, include_latents=False, seed=None, show_progress=True,
                                   n_jobs=-1):
        """`size` samples that comply with the evidence, each with its likelihood weight in `_weight`
        (Sampling.py:267-406; Koller & Friedman algorithm 12.2)."""
        from ..inference.batch import download

        ev = self._evidence(evidence)
        codes, nodes, w = self.forward_sample_codes(size, seed=seed, partial_codes=ev,
                                                    modes={v: OBSERVED for v in ev}, weights=True)
        return self._frame(download(codes), nodes, include_latents, weights=download(w))

    @E.serialized
    def rejection_sample(self, evidence=[], size=1, include_latents=False, seed=None, show_progress=True,
                         partial_samples=None, _given=None):
        """The first `size` rows of the stream of `seed` that match the evidence (Sampling.py:146-265).
        Batches of the stream are drawn and filtered on the device, each continuing where the last one
        stopped, so the result does not depend on the batch sizes.  Evidence of probability 0 raises
        ValueError after 64 consecutive batches without an accepted row (the reference never returns)."""
        import torch

        from ..inference.batch import download

        size = int(size)
        ev = self._evidence(evidence)
        given = dict(_given or {})
        if partial_samples is not None:  # with evidence its rows are the batch; without, they are the samples
            given.update(self._partial(partial_samples, partial_samples.shape[0] if ev else size))
        if not ev:
            codes, nodes = self.forward_sample_codes(size, seed=seed, partial_codes=given)
            return self._frame(download(codes), nodes, include_latents)
        seed = fresh_seed() if seed is None else int(seed) & MASK64
        n_nodes = max(len(self.model), 1)
        kept, n_kept, pos, prob, empty = [], 0, 0, 1.0, 0
        nodes = None
        while n_kept < size:
            batch = int(((size - n_kept) / prob) * 1.5)
            if partial_samples is not None:  # its rows are the batch
                batch = partial_samples.shape[0]
            batch = max(1, min(batch, REJECTION_MAX_BYTES // n_nodes))
            codes, nodes = self.forward_sample_codes(batch, seed=seed, first_row=pos, partial_codes=given)
            col = {v: i for i, v in enumerate(nodes)}
            ok = torch.ones(batch, dtype=torch.bool, device=codes.device)
            for var, code in ev.items():
                ok &= codes[col[var]] == code
            rows = torch.nonzero(ok).reshape(-1)
            n = int(rows.numel())
            if n:
                kept.append(codes.index_select(1, rows[:size - n_kept]).contiguous())
                empty = 0
            else:
                empty += 1
                if empty >= REJECTION_EMPTY_BATCHES:
                    raise ValueError(f"rejection_sample: no row matched the evidence in {REJECTION_EMPTY_BATCHES} "
                                     f"consecutive batches ({pos + batch} rows): the evidence has probability 0 or close to it")
            n_kept += n
            pos += batch
            prob = max(n / batch, REJECTION_FLOOR)
        if kept:
            out = download(torch.cat(kept, dim=1).contiguous())
        else:
            nodes = compiled(self.model).nodes
            out = np.empty((len(nodes), 0), dtype=np.uint8)
        return self._frame(out, nodes, include_latents)


from .gibbs import GibbsSampling  # noqa: E402  (it builds on the names above)
