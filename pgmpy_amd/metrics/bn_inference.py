"""BayesianModelProbability (mirror of pgmpy/metrics/bn_inference.py): the log-density of complete rows
under a discrete Bayesian network, on the device.

The reference walks the nodes; per node it groups the rows by their parent codes (np.unique(axis=0)),
reduces the CPD once per group and picks the node's value row by row in a Python loop.  Here one launch
(pgm_fit_logprob) streams the column-major uint8 codes once: per row it adds log theta_f[x_f | pa_f] over
every family in plan order in fp64, and leaves the total in a fixed-order tree.  The
families, the code columns and the device CPD values are the sampler's cached view of the model
(sampling.compiled), so CPDs that `fit` left on the device are not copied to the host; the log tables are
cached with it and rebuilt when the model or any factor's values change.

Deviations: a model with latent variables raises ValueError (the reference silently drops
latent parents, which is not a probability); a row with a missing cell raises ValueError (marginalising
the missing cells is inference); an array without `ordering` takes its columns in the model's
topological order (the reference's own code for that case fails); every CPD column is divided by its
total before the logarithm, as the reference does for the nodes that have parents (it leaves a root's
values as they are).  There is no CPU path.
"""
import networkx as nx
import numpy as np

from .. import engine as E


class BayesianModelProbability:
    def __init__(self, model):
        from ..models import DiscreteBayesianNetwork

        if not isinstance(model, DiscreteBayesianNetwork):
            raise TypeError(f"Model expected type: DiscreteBayesianNetwork, got type: {type(model)}")
        if len(model.latents) > 0:
            raise ValueError("BayesianModelProbability needs a model without latent variables: the probability of a row "
                             f"that leaves {sorted(map(str, model.latents))} out is a marginal (inference)")
        self.model = model
        self.topological_order = list(nx.topological_sort(model))

    # ------------------------------------------------------------------ device level
    def _tables(self):
        """(compiled model, fit plan over its families, device log tables), cached on the compiled model."""
        from ..estimators._fit import FitPlan
        from ..sampling import compiled

        c = compiled(self.model)
        hit = c.__dict__.get("_logp")
        if hit is None:
            plan = FitPlan(c.plan.families)
            values, cdf = c.tables()
            # Each CPD column divided by its total, as the reference's _reduce_marg does (sampling/base.py:98):
            # a column that a file rounded to a sum of 0.9999999 (alarm's HREKG, HRSAT) is a distribution
            # again.  The total is the last running sum the sampler already holds; the entry -> total index
            # is built once per model.  The quotient is written into the log tables' buffer, then logged in place.
            at = np.empty(plan.total_bins, dtype=np.int64)
            for (_, cards), off, size in zip(plan.families, plan.offsets, plan.sizes):
                ncol = size // cards[0]
                at[off:off + size] = off + size - ncol + np.arange(size, dtype=np.int64) % ncol
            logv = values / cdf[E.to_device_raw(at)]
            hit = c._logp = (plan, plan.log_values(logv, out=logv))
        return (c,) + hit

    @E.serialized
    def log_probability_codes(self, codes, n_rows=None, row0=0):
        """(device logp [ld], device total [1]) of the rows [row0, row0 + n_rows) of the device codes
        [n_nodes, ld] (uint8), columns in sorted(model.nodes()) order: what forward_sample_codes and
        GibbsSampling.sample_codes return.  Nothing is encoded, uploaded or downloaded but the status.
        Raises ValueError when a row holds 255 (missing), IndexError for any other code that is no state."""
        c, plan, logv = self._tables()
        with c.lock:
            logp, total, skipped = plan.logprob(logv, codes, n_rows=n_rows, row0=row0, total=True)
        if skipped:
            raise ValueError(f"{skipped} rows have a missing value: log_probability needs complete rows")
        return logp, total

    def _encode(self, data, ordering):
        import pandas as pd

        from ..inference.batch import ingest_states
        from ..sampling import compiled

        if isinstance(data, pd.DataFrame):
            frame = data
        else:
            data = np.asarray(data, dtype=object) if not isinstance(data, np.ndarray) else data
            if data.ndim != 2:
                raise ValueError(f"data must be a DataFrame or a 2-d array. Got {data.ndim} dimensions")
            ordering = list(self.topological_order if ordering is None else ordering)
            if data.shape[1] != len(ordering):
                raise ValueError(f"data has {data.shape[1]} columns, ordering names {len(ordering)}")
            frame = pd.DataFrame({v: data[:, j] for j, v in enumerate(ordering)}, columns=ordering)
        nodes = compiled(self.model).nodes
        missing = [v for v in nodes if v not in frame.columns]
        if missing:
            raise ValueError(f"data has no column for the variables {sorted(map(str, missing))}")
        return ingest_states(self.model.states, frame, nodes).codes

    def _run(self, data, ordering):
        codes = self._encode(data, ordering)
        if codes.shape[1] == 0:
            return None, None
        return self.log_probability_codes(codes)

    # ------------------------------------------------------------------ the reference's entry points
    def log_probability(self, data, ordering=None):
        """The log-probability of each row: a numpy (n_samples,) array.  `data` is a DataFrame of state
        names (columns in any order), or an array with `ordering` naming its columns (default: the model's
        topological order).  A category that is not a state raises KeyError."""
        from ..inference.batch import download

        logp, _ = self._run(data, ordering)
        return np.zeros(0, dtype=np.float64) if logp is None else download(logp)

    def score(self, data, ordering=None):
        """The total log-probability of the rows: the device's fixed-order sum."""
        from ..inference.batch import download

        _, total = self._run(data, ordering)
        return 0.0 if total is None else float(download(total)[0])
