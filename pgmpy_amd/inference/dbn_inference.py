"""DBNInference: filtering, smoothing and scoring of evidence sequences under a DynamicBayesianNetwork.

The reference (pgmpy/inference/dbn_inference.py) rebuilds a BeliefPropagation object and calibrates a
junction tree for every slice of ONE sequence.  Here a batch of sequences is one launch of the fused
filter kernel (csrc/pgmdbn.hip; DESIGN.md "Dynamic networks"): sequences are the data-parallel axis, the
joint of a slice's hidden nodes is enumerated in LDS and a message over the interface is carried from
slice to slice.

Results are exact (they equal enumeration of the unrolled network), so they differ from the reference
where it is not: an interface node observed at t >= 1 with an earlier slice queried.

Three levels:
  * the reference's ``forward_inference`` / ``backward_inference`` / ``query``: one sequence given as
    ``{(name, t): state}``, a ``{(name, t): DiscreteFactor}`` back;
  * ``filter_batch`` / ``smooth_batch`` / ``log_likelihood_batch``: a DataFrame with ``(name, t)`` columns,
    NaN or an absent column meaning "not observed";
  * ``filter_codes`` / ``smooth_codes`` / ``log_likelihood_codes``: a resident uint8 code tensor
    ``[(T + 1) n, B]`` (column ``t n + v`` is node v, sorted name order, of slice t; 255: not observed)
    and device tensors back.
The most probable sequence (Viterbi, csrc/pgmdbn.hip k_dbn_viterbi) has the same three levels: ``map_query``,
``viterbi_batch``, ``viterbi_codes``; it maximises over every unobserved cell jointly.
``expected_counts_codes`` (csrc/pgmdbn.hip k_dbn_estep) adds every sequence's expected family counts to fp64
tables on the device: the E-step that ``DynamicBayesianNetwork.fit(estimator="EM")`` iterates on.
There is no CPU path: without a device a compute call raises ``NativeUnavailable``.
"""
import numpy as np

from .. import engine as E
from ..factors.discrete import DiscreteFactor
from ._dbn import SCRATCH_BYTES, DbnPlan, flat_values

MISSING = 255


class DBNResult:
    """What a batched call returns: ``marginal(name)`` [B, T + 1, card] (host), ``log_likelihood`` [B],
    ``impossible`` [B] (bool); ``marginals``, ``loglik`` and ``flags`` are the device tensors."""

    def __init__(self, names, plan, marginals, loglik, flags):
        self._names, self._plan = names, plan
        self.marginals, self.loglik, self.flags = marginals, loglik, flags
        self._host = None

    def marginal(self, name):
        from .batch import download

        if self.marginals is None:
            raise ValueError("this result carries no marginals (log_likelihood_batch)")
        if name not in self._names or self._names.index(name) not in self._plan.query_slices:
            raise ValueError(f"{name} was not among the variables asked for")
        if self._host is None:
            self._host = download(self.marginals.contiguous())
        return self._host[:, :, self._plan.query_slices[self._names.index(name)]]

    @property
    def log_likelihood(self):
        from .batch import download

        return download(self.loglik)

    @property
    def impossible(self):
        from .batch import download

        return download(self.flags).astype(bool)


class ViterbiResult:
    """What ``viterbi_batch`` returns: ``sequences()`` a frame with one ``(name, t)`` column per node and slice
    holding state names (NaN in the unobserved cells of an impossible row), ``log_probability`` [B] =
    log max_x P(x, e) (-inf for an impossible row), ``impossible`` [B] (bool); ``path``, ``logmap`` and ``flags``
    are the device tensors (``path`` is a code matrix in the layout of the input)."""

    def __init__(self, names, state_names, path, logmap, flags):
        self._names, self._state_names = names, state_names
        self.path, self.logmap, self.flags = path, logmap, flags

    def sequences(self):
        import pandas as pd

        from .batch import download

        codes = download(self.path.contiguous())
        n = len(self._names)
        cols, keys = {}, []
        for c in range(codes.shape[0]):
            name = self._names[c % n]
            states = np.asarray(list(self._state_names[name]) + [np.nan], dtype=object)
            col = codes[c].astype(np.int64)
            cols[c] = states[np.where(col == MISSING, len(states) - 1, col)]
            keys.append((name, c // n))
        frame = pd.DataFrame(cols, index=range(codes.shape[1]))
        frame.columns = pd.Index(keys, tupleize_cols=False)
        return frame

    @property
    def log_probability(self):
        from .batch import download

        return download(self.logmap)

    @property
    def impossible(self):
        from .batch import download

        return download(self.flags).astype(bool)


class DBNInference:
    def __init__(self, model):
        from ..models.DynamicBayesianNetwork import DynamicBayesianNetwork

        if not isinstance(model, DynamicBayesianNetwork):
            raise TypeError(f"Model expected type: DynamicBayesianNetwork, got type: {type(model)}")
        model.check_model()
        self.model = model
        self.names = model._slice_order()
        self.index = {name: v for v, name in enumerate(self.names)}
        n = len(self.names)
        pairs = model._both_slices()
        self.cpds0 = [pairs[name][0] for name in self.names]
        self.cpds1 = [pairs[name][1] for name in self.names]
        self.card = [int(c.cardinality[0]) for c in self.cpds0]
        for name, k in zip(self.names, self.card):
            if k >= MISSING:
                raise ValueError(f"variable {name} has {k} states; uint8 codes hold at most 254")
        self.state_names = {name: list(c.state_names[c.variable]) for name, c in zip(self.names, self.cpds0)}
        # a column of the two-slice window: node v of slice h is h n + v
        self.families0 = [([self.index[u] for u, _ in c.variables], [int(k) for k in c.cardinality]) for c in self.cpds0]
        self.families1 = [([self.index[u] + n * h for u, h in c.variables], [int(k) for k in c.cardinality])
                          for c in self.cpds1]
        self._plans = {}
        self._values = None

    # ------------------------------------------------------------------ plans and tables
    def plan(self, observed=(), variables=None):
        """The DbnPlan with the nodes `observed` clamped and `variables` (default: every node) queried."""
        observed, variables = set(observed), set(self.names if variables is None else variables)
        for name in observed | variables:
            if name not in self.index:
                raise ValueError(f"Node {name} not in the model")
        key = (tuple(name in observed for name in self.names), tuple(name in variables for name in self.names))
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) >= 64:
                self._plans.clear()
            plan = self._plans[key] = DbnPlan(self.card, key[0], key[1], self.families0, self.families1)
        return plan

    def _tables(self):
        if self._values is None:
            self._values = (E.to_device(flat_values(self.cpds0)), E.to_device(flat_values(self.cpds1)))
        return self._values

    # ------------------------------------------------------------------ device level
    @E.serialized
    def _run_codes(self, codes, observed, variables, want_filter, want_smooth, scratch_bytes=SCRATCH_BYTES):
        plan = self.plan(observed, variables)
        values0, values1 = self._tables()
        out = plan.run(codes, values0, values1, want_filter=want_filter, want_smooth=want_smooth,
                       scratch_bytes=scratch_bytes)
        return plan, out

    def filter_codes(self, codes, observed=(), variables=None):
        """(filter [B, T + 1, Q], loglik [B], impossible [B]) on the device: P(v_t | e_0:t) of the queried
        nodes, their states end to end in sorted name order (``plan(observed, variables).query_slices``)."""
        _, (filt, _, loglik, flags) = self._run_codes(codes, observed, variables, True, False)
        return filt, loglik, flags

    def smooth_codes(self, codes, observed=(), variables=None, scratch_bytes=SCRATCH_BYTES):
        """(smooth [B, T + 1, Q], loglik [B], impossible [B]) on the device: P(v_t | e_0:T)."""
        _, (_, smooth, loglik, flags) = self._run_codes(codes, observed, variables, False, True, scratch_bytes)
        return smooth, loglik, flags

    def log_likelihood_codes(self, codes, observed=()):
        """(loglik [B], impossible [B]) on the device: log P(e_0:T) per sequence."""
        _, (_, _, loglik, flags) = self._run_codes(codes, observed, [], False, False)
        return loglik, flags

    @E.serialized
    def viterbi_codes(self, codes, observed=(), scratch_bytes=SCRATCH_BYTES):
        """(path [(T + 1) n, B] uint8, logmap [B], impossible [B]) on the device: the jointly most probable
        completion of every sequence, as a code matrix in the layout of `codes` (what ``fit``,
        ``log_probability_codes`` and ``smooth_codes`` read), and log max_x P(x, e_0:T), the joint with the
        evidence.  Ties go to the lowest state index.  An impossible sequence keeps 255 in its unobserved
        cells and gets -inf and the flag."""
        plan = self.plan(observed, [])
        values0, values1 = self._tables()
        return plan.viterbi(codes, values0, values1, scratch_bytes=scratch_bytes)

    @E.serialized
    def expected_counts_codes(self, codes, observed=(), values=None, tables=None, scratch_bytes=SCRATCH_BYTES, direct=False):
        """(tables0, tables1, loglik [B], impossible [B]) on the device: the expected family counts of every
        sequence under the model's CPDs (the E-step of Baum-Welch, csrc/pgmdbn.hip k_dbn_estep), flat fp64
        buffers in the layout of the CPD values: the slice-0 families of ``families0`` end to end, fed by
        slice 0 alone, and the transition families of ``families1``, fed by slices 1 .. T.  An impossible
        sequence adds nothing.  `values` (values0, values1) replaces the model's CPD values, `tables`
        (tables0, tables1) are added to instead of new zeroed ones: what ``fit(estimator="EM")`` iterates on."""
        plan = self.plan(observed, [])
        values0, values1 = self._tables() if values is None else values
        tables0, tables1 = (None, None) if tables is None else tables
        return plan.estep(codes, values0, values1, tables0, tables1, scratch_bytes=scratch_bytes, direct=direct)

    # ------------------------------------------------------------------ frames
    def encode(self, data):
        """(host codes [(T + 1) n, B] of a frame with (name, t) columns, the names observed in every cell)."""
        from .batch import encode_states

        columns = [tuple(c) for c in data.columns]
        for name, t in columns:
            if name not in self.index:
                raise ValueError(f"Node {name} not in the model")
            if not isinstance(t, (int, np.integer)) or t < 0:
                raise ValueError(f"column ({name}, {t}): the time slice must be a non-negative integer")
        n, B = len(self.names), len(data)
        n_slices = 1 + max((int(t) for _, t in columns), default=0)
        codes = np.full((n_slices * n, B), MISSING, dtype=np.uint8)
        if columns:
            flat = data.copy(deep=False)
            flat.columns = list(range(len(columns)))
            enc = encode_states({j: self.state_names[name] for j, (name, _) in enumerate(columns)}, flat)
            for j, (name, t) in enumerate(columns):
                codes[int(t) * n + self.index[name]] = enc[j]
        seen = codes.reshape(n_slices, n, B) != MISSING
        observed = [name for v, name in enumerate(self.names) if B and seen[:, v, :].all()]
        return codes, observed

    def _batch(self, data, variables, want_filter, want_smooth):
        codes, observed = self.encode(data)
        plan, (filt, smooth, loglik, flags) = self._run_codes(E.to_device_raw(codes), observed, variables, want_filter,
                                                              want_smooth)
        return DBNResult(self.names, plan, filt if want_filter else smooth, loglik, flags)

    def filter_batch(self, data, variables=None):
        """P(v_t | e_0:t) for every sequence (row) of `data` and every slice."""
        return self._batch(data, variables, True, False)

    def smooth_batch(self, data, variables=None):
        """P(v_t | e_0:T) for every sequence (row) of `data` and every slice."""
        return self._batch(data, variables, False, True)

    def log_likelihood_batch(self, data):
        """log P(e_0:T) for every sequence (row) of `data`."""
        return self._batch(data, [], False, False)

    def viterbi_batch(self, data):
        """The most probable completion of every sequence (row) of `data`: a ``ViterbiResult``."""
        codes, observed = self.encode(data)
        path, logmap, flags = self.viterbi_codes(E.to_device_raw(codes), observed)
        return ViterbiResult(self.names, self.state_names, path, logmap, flags)

    def map_query(self, variables=None, evidence=None):
        """{(name, t): state name} of one sequence, shaped like ``VariableElimination.map_query``: the jointly
        most probable assignment of ALL the unobserved nodes of slices 0 .. last given the evidence, last being
        the largest slice queried or observed.  `variables` (default: every unobserved node of those slices)
        only selects which entries are returned: this is not marginal MAP over a subset, whose answer may
        differ.  Ties go to the lowest state index.  Impossible evidence raises ValueError.  (The reference's
        DBNInference has no such method.)"""
        from .batch import download

        evidence = {tuple(k): s for k, s in (evidence or {}).items()}
        chosen = None if variables is None else [tuple(v) for v in variables]
        for name, t in list(chosen or []) + list(evidence):
            if name not in self.index:
                raise ValueError(f"Node {name} not in the model")
            if not isinstance(t, (int, np.integer)) or t < 0:
                raise ValueError(f"({name}, {t}): the time slice must be a non-negative integer")
        if chosen is not None and not chosen:
            return {}
        n = len(self.names)
        last = max([t for _, t in chosen or []] + [t for _, t in evidence], default=0)
        codes = np.full(((last + 1) * n, 1), MISSING, dtype=np.uint8)
        for (name, t), state in evidence.items():
            codes[t * n + self.index[name], 0] = self.cpds0[self.index[name]].get_state_no((name, 0), state)
        seen = codes.reshape(last + 1, n) != MISSING
        observed = [name for v, name in enumerate(self.names) if seen[:, v].all()]
        path, _, flags = self.viterbi_codes(E.to_device_raw(codes), observed)
        if download(flags)[0]:
            raise ValueError("map_query: the evidence has probability 0 under the model")
        host = download(path.contiguous())[:, 0]
        if chosen is None:
            chosen = [(name, t) for t in range(last + 1) for name in self.names if (name, t) not in evidence]
        return {(name, t): self.state_names[name][int(host[t * n + self.index[name]])] for name, t in chosen}

    # ------------------------------------------------------------------ the reference's entry points
    def _one(self, variables, evidence, smooth):
        from .batch import download

        variables = [tuple(v) for v in variables]
        evidence = {tuple(k): s for k, s in (evidence or {}).items()}
        for name, t in list(variables) + list(evidence):
            if name not in self.index:
                raise ValueError(f"Node {name} not in the model")
            if not isinstance(t, (int, np.integer)) or t < 0:
                raise ValueError(f"({name}, {t}): the time slice must be a non-negative integer")
        if not variables:
            return {}
        n = len(self.names)
        last = max([t for _, t in variables] + [t for _, t in evidence])
        codes = np.full(((last + 1) * n, 1), MISSING, dtype=np.uint8)
        for (name, t), state in evidence.items():
            codes[t * n + self.index[name], 0] = self.cpds0[self.index[name]].get_state_no((name, 0), state)
        seen = codes.reshape(last + 1, n) != MISSING
        observed = [name for v, name in enumerate(self.names) if seen[:, v].all()]
        plan, (filt, smoothed, _, _) = self._run_codes(E.to_device_raw(codes), observed, {name for name, _ in variables},
                                                       not smooth, smooth)
        host = download(smoothed if smooth else filt)[0]
        out = {}
        for name, t in variables:
            values = host[t, plan.query_slices[self.index[name]]]
            out[(name, t)] = DiscreteFactor([(name, t)], [self.card[self.index[name]]], values,
                                            state_names={(name, t): self.state_names[name]})
        return out

    def forward_inference(self, variables, evidence=None, args=None):
        """{(name, t): P((name, t) | evidence up to t)}.  The sequence runs to the last slice queried or
        observed; slices after the last evidence are prediction."""
        if args == "potential":
            raise NotImplementedError("args='potential' (the interface potentials of the junction trees) is not built")
        return self._one(variables, evidence, smooth=False)

    def backward_inference(self, variables, evidence=None):
        """{(name, t): P((name, t) | all the evidence)}."""
        return self._one(variables, evidence, smooth=True)

    def query(self, variables, evidence=None, args="exact"):
        if args == "exact":
            return self.backward_inference(variables, evidence)
        raise NotImplementedError(f"args={args!r} is not built: only 'exact'")
