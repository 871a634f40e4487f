"""ApproxInference (mirror of pgmpy/inference/ApproxInference.py) on the device.

The reference answers a query by rejection-sampling ``n_samples`` accepted rows (``model.simulate``) and
taking relative frequencies with a pandas groupby.  Here a query is likelihood weighting over
``n_samples`` draws in one fused kernel (pgm_sample_posterior): every sample is drawn, weighted
by the probability of the evidence given its parents and added to the target tables, without a sampled
code ever being written to memory.  ``query_batch`` does that for every row of a frame of evidence at once;
``DiscreteBayesianNetwork.predict(data, algo=ApproxInference)`` is its joint MAP.

Deviations from the reference:

* the estimator is likelihood weighting over ``n_samples`` draws, not the relative frequencies of
  ``n_samples`` accepted rows: equal in distribution in the limit, not in value (the sampler's stance);
* evidence of probability 0 gives NaN (every weight is 0) where the reference never returns;
* ``state_names=None`` means the model's states, all of them, in model order (the reference infers them
  from the samples, in order of appearance, and can miss states).

A ``DynamicBayesianNetwork`` is not taken here (``DBNInference`` filters and smooths it exactly).  There is no
CPU path: a query raises ``NativeUnavailable`` without the library or a device.
"""
import numpy as np

from .. import engine as E


class ApproxInference:
    def __init__(self, model):
        from ..models import DiscreteBayesianNetwork

        if not isinstance(model, DiscreteBayesianNetwork):
            raise ValueError(
                f"model should either be a Bayesian Network or Dynamic Bayesian Network. Got {type(model)}.")
        model.check_model()
        self.model = model

    # ------------------------------------------------------------------ helpers
    def _select(self, variables, values, state_names):
        """A DiscreteFactor over `variables` from `values` [cards of the model's states]; state_names
        selects and orders the states (a name the model does not know gets 0, as the reference's reindex)."""
        from ..factors.discrete import DiscreteFactor

        states = self.model.states
        names = {}
        for axis, v in enumerate(variables):
            own = list(states[v])
            want = own if state_names is None or v not in state_names else list(state_names[v])
            if want != own:
                pos = {s: i for i, s in enumerate(own)}
                idx = np.array([pos.get(s, -1) for s in want], dtype=np.int64)
                taken = np.take(values, np.maximum(idx, 0), axis=axis)
                shape = [1] * values.ndim
                shape[axis] = len(want)
                values = np.where((idx >= 0).reshape(shape), taken, 0.0)
            names[v] = want
        return DiscreteFactor(list(variables), [len(names[v]) for v in variables], values, state_names=names)

    def _with_virtual(self, virtual_evidence):
        """(model, {added node: 0}): each virtual evidence CPD on `var` adds the binary child `__var` with CPD
        [v; 1 - v] that is held at 0, as DiscreteBayesianNetwork.simulate builds it; the added nodes take
        code columns after the model's own."""
        from ..factors.discrete import TabularCPD

        if not virtual_evidence:
            return self.model, {}
        model = self.model.copy()
        columns, held = sorted(self.model.nodes()), {}
        for cpd in virtual_evidence:
            var = cpd.variables[0]
            if var not in self.model.nodes():
                raise ValueError("Evidence provided for variable which is not in the model")
            if len(cpd.variables) > 1:
                raise ValueError("Virtual evidence should be defined on individual variables. Maybe you are looking "
                                 "for soft evidence.")
            if self.model.get_cardinality(var) != cpd.get_cardinality([var])[var]:
                raise ValueError("The number of states/cardinality for the evidence should be same as the number of "
                                 "states/cardinality of the variable in the model")
            new_var = "__" + var
            v = np.asarray(cpd._values_readonly(), dtype=np.float64).reshape(1, -1)
            model.add_edge(var, new_var)
            model.add_cpds(TabularCPD(new_var, 2, np.vstack((v, 1 - v)), evidence=[var],
                                      evidence_card=[int(model.get_cardinality(var))],
                                      state_names={new_var: [0, 1], var: cpd.state_names[var]}))
            held[new_var] = 0
            columns.append(new_var)
        model.__dict__["_sample_columns"] = columns
        return model, held

    @staticmethod
    def _posterior(model, codes, targets, n_samples, seed):
        """posterior_codes on host evidence codes [n_nodes, R]: (host post [R, bins], log_evidence, ess,
        acc, layout)."""
        from ..sampling import BayesianModelSampling
        from .batch import download, upload_codes

        out, layout = BayesianModelSampling(model).posterior_codes(upload_codes(codes), targets, n_samples, seed=seed)
        return download(out.post), download(out.log_evidence), download(out.ess), download(out.acc), layout

    # ------------------------------------------------------------------ the reference's entry points
    @E.serialized
    def get_distribution(self, samples, variables, state_names=None, joint=True):
        """The distribution of `variables` in the frame `samples`: unweighted relative frequencies (rows /
        len(samples); a row with a NaN in a table's variables counts nowhere), counted on the device in one
        pgm_fit_count.  joint=True: one DiscreteFactor over `variables`; else {variable: DiscreteFactor}.
        state_names: {variable: states} to report, in that order (None: the model's)."""
        from ..sampling import compiled
        from .batch import download, encode_states, upload_codes

        variables = list(variables)
        for v in variables:
            if v not in self.model.nodes():
                raise ValueError(f"Node {v} not in the model")
        n = int(samples.shape[0])
        c = compiled(self.model)
        targets = (tuple(variables),) if joint else tuple((v,) for v in variables)
        plan = c.target_plan(targets)
        codes = np.full((len(c.nodes), n), 255, dtype=np.uint8)
        enc = encode_states({v: self.model.states[v] for v in variables}, samples, variables)
        for j, v in enumerate(variables):
            codes[c.col[v]] = enc[j]
        counts = download(plan.count(upload_codes(codes))).astype(np.float64) / n if n else np.full(plan.total_bins, np.nan)
        out = []
        for i, t in enumerate(targets):
            shape = [c.card[v] for v in t]
            out.append(self._select(t, counts[plan.offsets[i]:plan.offsets[i] + plan.sizes[i]].reshape(shape), state_names))
        return out[0] if joint else dict(zip(variables, out))

    def query(self, variables, n_samples=int(1e4), samples=None, evidence=None, virtual_evidence=None, joint=True,
              state_names=None, show_progress=True, seed=None):
        """P(variables | evidence, virtual_evidence) by likelihood weighting over n_samples draws (one
        pgm_sample_posterior call with one evidence row), or the frequencies of `samples` when given.
        joint=True: one DiscreteFactor; else {variable: DiscreteFactor}.  show_progress is accepted and
        ignored."""
        variables = list(variables)
        if samples is not None:
            return self.get_distribution(samples, variables, state_names=state_names, joint=joint)
        from ..sampling import compiled

        for v in variables:
            if v not in self.model.nodes():
                raise ValueError(f"Node {v} not in the model")
        evidence = {} if evidence is None else dict(evidence)
        states = self.model.states
        for var, state in evidence.items():
            if var not in states:
                raise ValueError(f"Evidence variable {var} not in the model")
            if state not in states[var]:
                raise ValueError(f"Evidence state: {state} for {var} doesn't exist")
        model, held = self._with_virtual(virtual_evidence)
        c = compiled(model)
        codes = np.full((len(c.nodes), 1), 255, dtype=np.uint8)
        for var, state in evidence.items():
            codes[c.col[var], 0] = list(states[var]).index(state)
        for var, code in held.items():
            codes[c.col[var], 0] = code
        targets = [variables] if joint else [[v] for v in variables]
        post, _, _, _, layout = self._posterior(model, codes, targets, n_samples, seed)
        out = [self._select(t, post[0, off:off + int(np.prod(shape))].reshape(shape), state_names)
               for t, off, shape in layout]
        return out[0] if joint else dict(zip(variables, out))

    def map_query(self, variables, n_samples=int(1e4), samples=None, evidence=None, virtual_evidence=None,
                  state_names=None, show_progress=True, seed=None):
        """The most probable joint state of `variables`: the argmax of query(joint=True), the lowest flat
        index on ties (np.argmax)."""
        dist = self.query(variables, n_samples=n_samples, samples=samples, evidence=evidence,
                          virtual_evidence=virtual_evidence, joint=True, state_names=state_names,
                          show_progress=show_progress, seed=seed)
        values = np.asarray(dist.values, dtype=np.float64)
        idx = np.unravel_index(int(np.argmax(values)), values.shape)
        return {v: dist.state_names[v][k] for v, k in zip(dist.variables, idx)}

    # ------------------------------------------------------------------ the batched entry
    def _evidence_codes(self, data):
        """(host codes [n_nodes, R] of a frame of evidence rows: NaN or an absent column = 255, compiled)."""
        from ..sampling import compiled
        from .batch import encode_states

        extra = [v for v in data.columns if v not in self.model.nodes()]
        if extra:
            raise ValueError(f"Data has variables which are not in the model: {extra}")
        c = compiled(self.model)
        columns = list(data.columns)
        codes = np.full((len(c.nodes), len(data)), 255, dtype=np.uint8)
        if columns:
            enc = encode_states({v: self.model.states[v] for v in columns}, data, columns)
            for j, v in enumerate(columns):
                codes[c.col[v]] = enc[j]
        return codes, c

    @E.serialized
    def query_batch(self, data, variables=None, n_samples=int(1e4), joint=False, seed=None):
        """One likelihood-weighting query per row of `data`, a frame of evidence (NaN or an absent column:
        not observed), in one pgm_sample_posterior call.  variables default to every variable that is
        missing in some row, in model order.

        joint=False: a frame with the columns f"{var}_{state}" of predict_probability for every variable,
        then `log_evidence` (the estimate of log P(the row's evidence)) and `ess` (the effective sample
        size).  A variable a row observes comes out one-hot.  joint=True: (values [R, cards...] of the
        joint over `variables`, the frame of log_evidence and ess)."""
        import pandas as pd

        codes, c = self._evidence_codes(data)
        if variables is None:
            variables = [v for v in self.model.nodes() if (codes[c.col[v]] == 255).any()]
        variables = list(variables)
        if not variables:
            raise ValueError("No variable missing in data. Nothing to query")
        for v in variables:
            if v not in self.model.nodes():
                raise ValueError(f"Node {v} not in the model")
        targets = [variables] if joint else [[v] for v in variables]
        post, le, ess, _, layout = self._posterior(self.model, codes, targets, n_samples, seed)
        tail = pd.DataFrame({"log_evidence": le, "ess": ess}, index=data.index)
        if joint:
            return post.reshape((len(data),) + layout[0][2]), tail
        cols = {}
        for (v,), off, (card,) in layout:
            for k, s in enumerate(self.model.states[v]):
                cols[f"{v}_{s}"] = post[:, off + k]
        return pd.concat([pd.DataFrame(cols, index=data.index), tail], axis=1)

    @E.serialized
    def predict_frame(self, data, order, n_samples=int(1e4), seed=None):
        """DiscreteBayesianNetwork.predict(algo=ApproxInference): the joint MAP of the variables `order`
        (the columns `data` lacks) per row, from one posterior call with one joint target; ties take the
        lowest flat index.  A row whose samples all have weight 0 gets NaN."""
        from .batch import _append_columns

        codes, c = self._evidence_codes(data)
        bins, budget = int(np.prod([c.card[v] for v in order], dtype=object)), c.posterior_bin_budget()
        if bins > budget or len(order) > 32:
            raise ValueError(f"predict(algo=ApproxInference): the joint table of the {len(order)} missing variables "
                             f"has {bins} states; the kernel's bin budget for this model is {budget} (and 32 variables)")
        _, _, _, acc, layout = self._posterior(self.model, codes, [list(order)], n_samples, seed)
        idx = np.argmax(acc, axis=1).astype(np.int64)
        dead = acc.max(axis=1, initial=0) == 0
        vals = {}
        for v in reversed(list(order)):
            k = c.card[v]
            col = np.array(self.model.states[v], dtype=object)[idx % k]
            col[dead] = np.nan
            vals[v] = col
            idx //= k
        out = _append_columns(data, vals, list(order))
        return out if out.index.is_monotonic_increasing else out.sort_index()
