"""BaseEstimator / ParameterEstimator (mirror of pgmpy/estimators/base.py:14-269).

The reference counts with a pandas groupby per node; here the frame is encoded once into column-major
uint8 state codes on the device (the evidence encoders of pgmpy_amd.inference.batch, against the
estimator's own state names) and the counts come from the fused family-count kernel (pgm_fit_count).
Nothing touches the device before the first count: the constructors only validate.
"""
import numpy as np

from .. import engine as E
from ._fit import FitPlan

WEIGHT = "_weight"


class BaseEstimator(object):
    def __init__(self, data=None, state_names=None):
        self.data = data
        self._encoded = None
        if self.data is not None:
            self.variables = list(data.columns.values)
            if not isinstance(state_names, dict):
                self.state_names = {var: self._collect_state_names(var) for var in self.variables}
            else:
                self.state_names = dict()
                for var in self.variables:
                    if var in state_names:
                        if not set(self._collect_state_names(var)) <= set(state_names[var]):
                            raise ValueError(f"Data contains unexpected states for variable: {var}.")
                        self.state_names[var] = state_names[var]
                    else:
                        self.state_names[var] = self._collect_state_names(var)

    def _collect_state_names(self, variable):
        "Return a list of states that the variable takes in the data."
        return sorted(list(self.data.loc[:, variable].dropna().unique()))

    # ------------------------------------------------------------------ device side
    def _codes(self):
        """(device codes [n_cols, n] uint8, {variable: column}) of every data column but `_weight`,
        encoded once per estimator.  A variable with 255 or more states raises the encoders'
        ValueError (uint8 codes; a deviation from the reference)."""
        if self._encoded is None:
            from ..inference.batch import ingest_states

            E.device()  # NativeUnavailable without a GPU, before any host work
            columns = [v for v in self.variables if v != WEIGHT]
            states = {v: list(self.state_names[v]) for v in columns}
            ev = ingest_states(states, self.data, columns)
            self._encoded = (ev.codes, {v: j for j, v in enumerate(columns)})
        return self._encoded

    def _weights(self, weighted):
        if not weighted:
            return None
        w = np.ascontiguousarray(self.data[WEIGHT].to_numpy(dtype=np.float64))
        return E.to_device_raw(w)

    def _check_weighted(self, weighted):
        if weighted and (WEIGHT not in self.data.columns):
            raise ValueError("data must contain a `_weight` column if weighted=True")

    def _family(self, variable, parents, col_of):
        for v in [variable] + list(parents):
            if v not in col_of:
                raise KeyError(v)
        return ([col_of[v] for v in [variable] + list(parents)],
                [len(self.state_names[v]) for v in [variable] + list(parents)])

    def _count_families(self, families, weighted=False):
        """FitPlan and flat device count tables of [(variable, parents)] families: one launch."""
        self._check_weighted(weighted)
        codes, col_of = self._codes()
        plan = FitPlan([self._family(v, ps, col_of) for v, ps in families])
        return plan, plan.count(codes, weights=self._weights(weighted))

    @E.serialized
    def state_counts(self, variable, parents=[], weighted=False, reindex=True):
        """How often each state of `variable` occurred, per configuration of `parents`
        (base.py:67-176): index = the variable's states, columns = the parents' states (a MultiIndex,
        in the order given).  A row with NaN in any of the family's columns is not counted.
        reindex=False drops the parent configurations that never occurred."""
        import pandas as pd

        from ..inference.batch import download

        parents = list(parents)
        self._check_weighted(weighted)
        plan, tables = self._count_families([(variable, parents)], weighted)
        counts = download(tables).reshape(len(self.state_names[variable]), -1)
        if not weighted and (counts != 0).all():
            pass  # the reference's integer counts survive when no cell had to be filled with 0
        else:
            counts = counts.astype(np.float64)
        index = pd.Index(list(self.state_names[variable]), name=variable)
        if not parents:
            return pd.DataFrame(counts, index=index, columns=[WEIGHT if weighted else "count"])
        columns = pd.MultiIndex.from_product([list(self.state_names[p]) for p in parents], names=parents)
        out = pd.DataFrame(counts, index=index, columns=columns)
        if not reindex:
            out = out.loc[:, (counts != 0).any(axis=0)]
        return out


    # ------------------------------------------------------------------ every pair of columns at once
    def _pair_plan(self, variables, given):
        codes, col_of = self._codes()
        variables = [v for v in self.variables if v != WEIGHT] if variables is None else list(variables)
        for v in variables + ([] if given is None else [given]):
            if v not in col_of:
                raise KeyError(v)
        from ._pairs import PairPlan

        plan = PairPlan([col_of[v] for v in variables], [len(self.state_names[v]) for v in variables])
        stratum = None if given is None else col_of[given]
        n_strata = 1 if given is None else len(self.state_names[given])
        return plan, codes, variables, stratum, n_strata

    @E.serialized
    def pairwise_counts(self, variables=None, given=None):
        """{(u, v): DataFrame} of the contingency table of every pair of `variables` (all columns when
        None; u before v in that order), from one launch of the pairwise-count kernel (pgm_pair_count):
        index = u's states, columns = v's states, and with `given` a MultiIndex (v, given) of columns, as
        state_counts(u, [v, given]) has.  A row with NaN in u, v or `given` is not counted.  Downloads every
        table: meant for small inputs."""
        import pandas as pd

        from ..inference.batch import download

        plan, codes, variables, stratum, n_strata = self._pair_plan(variables, given)
        counts = download(plan.count(codes, stratum=stratum, n_strata=n_strata)).reshape(n_strata, plan.Sp, plan.Sp)
        out = {}
        for i, u in enumerate(variables):
            for j in range(i + 1, len(variables)):
                v = variables[j]
                block = np.asarray(plan.block(counts, i, j, slice(None)))  # [strata, ru, rv]
                index = pd.Index(list(self.state_names[u]), name=u)
                if given is None:
                    out[(u, v)] = pd.DataFrame(block[0], index=index, columns=pd.Index(list(self.state_names[v]), name=v))
                else:
                    columns = pd.MultiIndex.from_product([list(self.state_names[v]), list(self.state_names[given])],
                                                         names=[v, given])
                    out[(u, v)] = pd.DataFrame(block.transpose(1, 2, 0).reshape(block.shape[1], -1), index=index,
                                               columns=columns)
        return out

    @E.serialized
    def pairwise_mutual_information(self, variables=None, given=None, kind="mutual_info"):
        """The symmetric [n, n] matrix (numpy, zero diagonal) of the `kind` of mutual information of every
        pair of `variables` (all columns when None): "mutual_info", "normalized_mutual_info" or
        "adjusted_mutual_info", scikit-learn's definitions.  With `given`, the weight of a pair is
        sum_c p_c w_c over the states c of that column (the TAN weight).  One count launch, one or two
        statistic launches (the expected mutual information only for the adjusted kind) and one download.
        A row with NaN is left out per pair."""
        from ..inference.batch import download
        from . import _pairs as P

        if kind not in P.KINDS:
            P.pair_weights(kind, 0.0, 0.0, 0.0, 0)  # the reference's ValueError
        plan, codes, variables, stratum, n_strata = self._pair_plan(variables, given)
        if plan.n_pairs == 0:
            return np.zeros((len(variables), len(variables)))
        counts = plan.count(codes, stratum=stratum, n_strata=n_strata)
        stats = list(plan.mi(counts))
        if kind == "adjusted_mutual_info":
            stats.append(plan.emi(counts))
        import torch

        flat = download(torch.cat([s.view(torch.int64).reshape(-1) for s in stats]))  # one copy: raw 64-bit words
        parts = flat.reshape(len(stats), n_strata, plan.n_pairs)
        mi, hu, hv = (parts[k].view(np.float64) for k in range(3))
        n = parts[3]
        emi = parts[4].view(np.float64) if len(stats) == 5 else None
        w = P.pair_weights(kind, mi, hu, hv, n, emi)
        values = w[0] if given is None else P.stratified_weight(w, n)
        return P.weight_matrix(len(variables), values)


class ParameterEstimator(BaseEstimator):
    def __init__(self, model, data, **kwargs):
        self.model = model
        super(ParameterEstimator, self).__init__(data, **kwargs)

    def state_counts(self, variable, weighted=False, **kwargs):
        """state_counts with the model's parents of `variable`, sorted (base.py:228-269)."""
        parents = sorted(self.model.get_parents(variable))
        return super(ParameterEstimator, self).state_counts(variable, parents=parents, weighted=weighted, **kwargs)

    # ------------------------------------------------------------------ shared by MLE and Bayes
    def _families(self, nodes):
        return [(node, sorted(self.model.get_parents(node))) for node in nodes]

    def _cpds(self, plan, families, values):
        """One TabularCPD per family, each a view of the flat device buffer `values`."""
        from ..factors.discrete import TabularCPD

        cpds = []
        for f, (node, parents) in enumerate(families):
            scope = [node] + parents
            cards = [len(self.state_names[v]) for v in scope]
            cpds.append(TabularCPD._from_device(node, cards[0], plan.table(values, f), parents, cards[1:],
                                                {v: list(self.state_names[v]) for v in scope}))
        return cpds
