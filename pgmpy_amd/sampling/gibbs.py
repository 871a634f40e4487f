"""GibbsSampling (mirror of pgmpy/sampling/Sampling.py:409-631) on the device.

The reference tabulates, per variable, the transition distribution over every joint configuration of all
other variables and walks one chain in a Python loop.  Here the conditional of a variable is the product
of the few factors that contain it, read at the chain's current codes, and one kernel launch
(pgm_gibbs_sweep) advances many chains, one per lane, through many sweeps in the column-major uint8 code
matrix ``[n_nodes, n_chains]`` that FitPlan.count and predict read.  The uniform of chain r, sweep j and
code column c is a pure function of (seed, r, c, j): the forward sampler's Philox stream with the sweep as
its fourth counter word, so a result does not depend on the kernel path or on how the sweeps
are split over launches.

Deviations from the reference: draws equal its in distribution, not in value; a sweep visits the variables
in code-column order (``column_order(model)``), not in ``model.nodes()`` order; no state is carried from
one call to the next (every call starts from its own start state); a network with deterministic CPDs may
not be ergodic under single-site Gibbs, which is not detected.

The plan and the flat device tables are cached per model and rebuilt when the model's change counter or
any factor's values change.  There is no CPU path: drawing raises ``NativeUnavailable`` without the
library or a device; the argument checks run before that.
"""
import threading
import weakref

import numpy as np

from .. import engine as E
from . import MASK64, BayesianModelSampling, State, column_order, compiled, fresh_seed
from ._gibbs import MAX_SWEEP, GibbsPlan

CHAIN = "_chain"
# Variable updates of one launch.  Longer runs are issued as several launches (the split is invisible:
# the stream is a function of the sweep number), so that no single launch holds a shared device for long:
# 2^30 updates are about 10 ms at the rate measured on alarm (109 G updates/s) and about 80 ms at munin's
# (13 G updates/s on the global path; DESIGN.md, Gibbs sampling).
LAUNCH_UPDATES = 1 << 30


class _GibbsCompiled:
    """The Gibbs sampler's view of a model: columns, factors, the plan (host only), the device tables."""

    def __init__(self, model, bayesian):
        self.bayesian = bayesian
        self.lock = threading.Lock()  # the plan's clamp array on the device is per handle: one launch at a time
        self.values = None
        if bayesian:
            self.forward = compiled(model)  # the forward sampler's families are the CPD factors
            self.nodes, self.col = self.forward.nodes, self.forward.col
            self.factors = self.forward.plan.families
            self.card = [self.forward.card[v] for v in self.nodes]
            self.source = self.forward.cpds
        else:
            model.check_model()
            self.nodes = column_order(model)
            self.col = {v: i for i, v in enumerate(self.nodes)}
            if len(self.col) != len(self.nodes) or set(self.nodes) != set(model.nodes()):
                raise ValueError("the sampler's column order must list every node of the model once")
            card = model.get_cardinality()
            self.card = [int(card[v]) for v in self.nodes]
            self.source = list(model.factors)
            self.factors = [([self.col[u] for u in f.variables], [int(k) for k in f.cardinality]) for f in self.source]
        for v, k in zip(self.nodes, self.card):
            if k >= 255:
                raise ValueError(f"variable {v} has {k} states; uint8 codes hold at most 254")
        self.plan = GibbsPlan(self.factors, self.card)

    def tables(self):
        """The flat values on the device; factors that are already there (fit) are not copied to the host."""
        if self.values is None:
            if self.bayesian:
                self.values = self.forward.tables()[0]
            else:
                import torch

                if all(f._dev is None for f in self.source):  # one upload
                    self.values = E.to_device(np.concatenate([np.asarray(f._values_readonly()).ravel() for f in self.source]))
                else:
                    self.values = torch.cat([f._d().reshape(-1) for f in self.source])
        return self.values


_CACHE = weakref.WeakKeyDictionary()  # model -> (key, _GibbsCompiled)


def gibbs_compiled(model, bayesian):
    """The model's cached _GibbsCompiled: rebuilt on the change counters the forward sampler watches (a
    Markov network has no counter of its own: its list of factors is the key)."""
    from ..factors.discrete.DiscreteFactor import values_epoch

    structure = model.__dict__.get("_epoch", 0) if bayesian else tuple(id(f) for f in model.factors)
    key = (structure, values_epoch())
    hit = _CACHE.get(model)
    if hit is None or hit[0] != key:
        hit = _CACHE[model] = (key, _GibbsCompiled(model, bayesian))
    return hit[1]


class GibbsSampling:
    def __init__(self, model=None):
        from ..models import DiscreteBayesianNetwork, DiscreteMarkovNetwork

        if not isinstance(model, (DiscreteBayesianNetwork, DiscreteMarkovNetwork)):
            raise TypeError("Model expected type: DiscreteBayesianNetwork or DiscreteMarkovNetwork, "
                            f"got type: {type(model)}")
        self.model = model
        self.bayesian = isinstance(model, DiscreteBayesianNetwork)
        self.variables = list(model.nodes())
        self.latents = set(model.latents)

    # ------------------------------------------------------------------ helpers
    def _state_no(self, var, state):
        if self.bayesian:
            return self.model.get_cpds(var).get_state_no(var, state)
        return next(f for f in self.model.factors if var in f.scope()).get_state_no(var, state)

    def _evidence(self, evidence):
        """{node: state code} of [(var, state)] or {var: state}, resolved through the model's state names."""
        out = {}
        pairs = evidence.items() if isinstance(evidence, dict) else (evidence or [])
        for var, state in pairs:
            if var not in self.model.nodes():
                raise ValueError(f"Evidence variable {var} not in the model")
            out[var] = int(self._state_no(var, state))
        return out

    def _start(self, start_state):
        """{node: state number} of a dict or a list of State(var, state number), covering every variable."""
        if start_state is None:
            return None
        pairs = list(start_state.items()) if isinstance(start_state, dict) else [tuple(s) for s in start_state]
        out = {}
        for var, state in pairs:
            if var not in self.model.nodes():
                raise ValueError(f"start_state variable {var} not in the model")
            if int(state) != state or int(state) < 0:
                raise ValueError(f"start_state of {var} must be a state number. Got {state}")
            out[var] = int(state)
        missing = [v for v in self.model.nodes() if v not in out]
        if missing:
            raise ValueError(f"start_state must cover every variable of the model; missing: {missing}")
        return out

    @staticmethod
    def _positive(**named):
        for name, x in named.items():
            if int(x) != x or int(x) < 1:
                raise ValueError(f"{name} must be a positive integer. Got {x}")

    def _advance(self, c, codes, first_sweep, n_sweeps, seed, clamp, thin=None):
        """Sweeps first_sweep .. first_sweep + n_sweeps - 1 in launches of at most LAUNCH_UPDATES variable
        updates; with thin, the device records [n_nodes, (n_sweeps // thin) * n_chains] of every thin-th
        sweep."""
        import torch

        n_chains = int(codes.shape[1])
        free = max(1, sum(1 for x in clamp if not x)) if clamp is not None else len(c.nodes)
        step = max(1, LAUNCH_UPDATES // max(1, n_chains * free))
        if thin:
            step = max(thin, step // thin * thin)  # a launch ends on a record
        values = c.tables()
        traces, done = [], 0
        while done < n_sweeps:
            n = min(step, n_sweeps - done)
            trace = None
            if thin and n // thin:
                trace = torch.empty((len(c.nodes), (n // thin) * n_chains), dtype=torch.uint8, device=codes.device)
                traces.append(trace)
            try:
                with c.lock:  # the call returns after the launch has finished (it reads the flags back)
                    c.plan.sweep(values, codes, n, first_sweep=first_sweep + done, seed=seed, clamp=clamp, trace=trace,
                                 thin=thin or 1)
            except ValueError as e:
                if "probability 0" not in str(e):
                    raise
                raise ValueError("GibbsSampling: the start state has probability 0 under the model (a conditional's "
                                 "total is not finite or not > 0); choose a start state the model allows") from e
            done += n
        if not thin:
            return None
        if not traces:
            return torch.empty((len(c.nodes), 0), dtype=torch.uint8, device=codes.device)
        return traces[0] if len(traces) == 1 else torch.cat(traces, dim=1)

    def _begin(self, n_chains, seed, start_codes, ev):
        """(compiled, device codes [n_nodes, n_chains] of the start state, clamp or None)."""
        import torch

        c = gibbs_compiled(self.model, self.bayesian)
        clamp = None
        if ev:
            clamp = np.zeros(len(c.nodes), dtype=np.uint8)
            for v in ev:
                clamp[c.col[v]] = 1
        if start_codes is not None:
            if isinstance(start_codes, torch.Tensor):
                codes = start_codes.to(torch.uint8).contiguous().clone()
            else:
                codes = E.to_device_raw(np.ascontiguousarray(start_codes, dtype=np.uint8))
            if tuple(codes.shape) != (len(c.nodes), n_chains):
                raise ValueError(f"start_codes must be [{len(c.nodes)}, {n_chains}]. Got {list(codes.shape)}")
        elif self.bayesian:
            # rows [0, n_chains) of the forward stream of the seed, the evidence taken as given
            codes, _ = BayesianModelSampling(self.model).forward_sample_codes(n_chains, seed=seed, partial_codes=ev)
            return c, codes, clamp
        else:
            values = c.tables()
            codes = torch.empty((len(c.nodes), n_chains), dtype=torch.uint8, device=values.device)
            c.plan.start(codes, seed=seed)
        for v, code in ev.items():
            codes[c.col[v]].fill_(code)
        return c, codes, clamp

    # ------------------------------------------------------------------ device level
    @E.serialized
    def sample_codes(self, n_chains, n_sweeps, seed=None, start_codes=None, evidence=None, first_sweep=1):
        """(uint8 device codes [n_nodes, n_chains], nodes): the state of every chain after sweeps
        first_sweep .. first_sweep + n_sweeps - 1, columns in column_order(model).  Each chain's state
        after burn-in is one draw, in the matrix FitPlan.count and predict read.

        start_codes=None: a Bayesian network starts from rows [0, n_chains) of the forward stream of
        `seed` with the evidence given; a Markov network starts every column at floor(u * card) from the
        sweep-0 uniform, the evidence written over it.  Evidence columns are clamped.  seed=None takes
        fresh entropy."""
        n_chains, n_sweeps, first_sweep = int(n_chains), int(n_sweeps), int(first_sweep)
        if n_chains < 1:
            raise ValueError(f"n_chains must be a positive integer. Got {n_chains}")
        if n_sweeps < 0 or first_sweep < 1 or first_sweep + n_sweeps - 1 > MAX_SWEEP:
            raise ValueError(f"sweeps [{first_sweep}, + {n_sweeps}) must lie in 1 .. 2^32 - 1")
        ev = self._evidence(evidence)
        seed = fresh_seed() if seed is None else int(seed) & MASK64
        c, codes, clamp = self._begin(n_chains, seed, start_codes, ev)
        self._advance(c, codes, first_sweep, n_sweeps, seed, clamp)
        return codes, c.nodes

    @E.serialized
    def _records(self, start, size, seed, n_chains, burn_in, thin, ev):
        """Host codes [size, n_nodes, n_chains]: the states after burn_in + i * thin sweeps, and the nodes."""
        from ..inference.batch import download

        seed = fresh_seed() if seed is None else int(seed) & MASK64
        start_codes = None
        if start is not None:
            nodes = column_order(self.model)
            start_codes = np.repeat(np.array([[start[v]] for v in nodes], dtype=np.int64), n_chains, axis=1)
            if start_codes.max(initial=0) > 255:
                raise IndexError("start_state: a state number is >= its variable's cardinality")
        c, codes, clamp = self._begin(n_chains, seed, start_codes, ev)
        self._advance(c, codes, 1, burn_in, seed, clamp)
        first = download(codes)
        trace = self._advance(c, codes, 1 + burn_in, (size - 1) * thin, seed, clamp, thin=thin)
        rest = download(trace).reshape(len(c.nodes), size - 1, n_chains).transpose(1, 0, 2)
        return np.concatenate([first[None], rest], axis=0), c.nodes

    # ------------------------------------------------------------------ the reference's entry points
    def sample(self, start_state=None, size=1, seed=None, include_latents=False, *, n_chains=1, burn_in=0, thin=1,
               evidence=None):
        """`size` states of each of `n_chains` chains (Sampling.py:521-585): a DataFrame of integer state
        numbers, columns in model.nodes() order.  Row 0 of a chain is its state after `burn_in` sweeps (for
        the reference's defaults: the start state), row i the state after burn_in + i * thin sweeps.  With
        n_chains > 1 the rows are chain-major and a `_chain` column says which chain a row belongs to.
        start_state: a dict or a list of State(var, state number) covering every variable (None: a random
        start, see sample_codes); evidence: [(var, state)], clamped."""
        import pandas as pd

        self._positive(size=size, thin=thin, n_chains=n_chains)
        if int(burn_in) != burn_in or burn_in < 0:
            raise ValueError(f"burn_in must be a non-negative integer. Got {burn_in}")
        size, thin, n_chains, burn_in = int(size), int(thin), int(n_chains), int(burn_in)
        if burn_in + (size - 1) * thin > MAX_SWEEP:
            raise ValueError("burn_in + (size - 1) * thin must be below 2^32")
        start = self._start(start_state)
        ev = self._evidence(evidence)
        rec, nodes = self._records(start, size, seed, n_chains, burn_in, thin, ev)
        pos = {v: i for i, v in enumerate(nodes)}
        keep = [v for v in self.variables if include_latents or v not in self.latents]
        # chain-major: all rows of chain 0, then of chain 1, ...
        data = {v: rec[:, pos[v], :].T.reshape(-1).astype(np.int64) for v in keep}
        df = pd.DataFrame(data, columns=keep)
        if n_chains > 1:
            df[CHAIN] = np.repeat(np.arange(n_chains, dtype=np.int64), size)
        return df

    def generate_sample(self, start_state=None, size=1, include_latents=False, seed=None):
        """Generator version (Sampling.py:587-631): the list of State(var, state number) after each of
        `size` sweeps of one chain."""
        self._positive(size=size)
        start = self._start(start_state)
        rec, nodes = self._records(start, int(size) + 1, seed, 1, 0, 1, {})
        pos = {v: i for i, v in enumerate(nodes)}
        keep = [v for v in self.variables if include_latents or v not in self.latents]
        for i in range(1, int(size) + 1):
            yield [State(v, int(rec[i, pos[v], 0])) for v in keep]
