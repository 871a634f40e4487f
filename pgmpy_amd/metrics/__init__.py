"""Model metrics (mirror of pgmpy/metrics/metrics.py).  Built: structure_score.  Not built:
log_likelihood_score, correlation_score, implied_cis, fisher_c, SHD."""
import networkx as nx

__all__ = ["structure_score"]


def structure_score(model, data, scoring_method="bic-d", **kwargs):
    """The structure score of `model` (its graph only) on `data` (metrics.py:222-307): one of k2, bdeu,
    bds, bic-d, aic-d, ll-d; kwargs go to the score's constructor.  The default is "bic-d": the
    reference's default "bic-g" is a Gaussian score, which is not built."""
    import pandas as pd

    from ..estimators import AIC, BIC, K2, BDeu, BDs, LogLikeliHood

    classes = {"k2": K2, "bdeu": BDeu, "bds": BDs, "bic-d": BIC, "aic-d": AIC, "ll-d": LogLikeliHood}
    if not isinstance(model, nx.DiGraph):
        raise ValueError(f"model must be a DiscreteBayesianNetwork or a networkx.DiGraph. Got {type(model)}")
    if not isinstance(data, pd.DataFrame):
        raise ValueError(f"data must be a pandas.DataFrame instance. Got {type(data)}")
    missing = set(model.nodes()) ^ set(data.columns)
    if missing:
        raise ValueError(f"Missing columns in data or variables in the model: {sorted(map(str, missing))}")
    if scoring_method not in classes:
        raise ValueError(f"scoring method not supported: {scoring_method!r} (one of {sorted(classes)})")
    return classes[scoring_method](data, **kwargs).score(model)
