"""Model metrics (mirror of pgmpy/metrics/metrics.py and pgmpy/metrics/bn_inference.py).  Built:
structure_score, log_likelihood_score and BayesianModelProbability (one device pass over the codes,
bn_inference.py), correlation_score and fisher_c (their tests batched through one CITester), SHD.  Not
built: implied_cis (it needs DAG.minimal_dseparator, which is not built), the Gaussian scores of
structure_score."""
import math
from itertools import combinations

import networkx as nx
import numpy as np

from .bn_inference import BayesianModelProbability

__all__ = ["structure_score", "log_likelihood_score", "BayesianModelProbability", "correlation_score", "fisher_c",
           "SHD", "f1_score", "chi2_sf_even"]


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


def _check_model_and_frame(model, data, what):
    import pandas as pd

    from ..models import DiscreteBayesianNetwork

    if not isinstance(model, DiscreteBayesianNetwork):
        raise ValueError(f"{what}: model must be a DiscreteBayesianNetwork. Got {type(model)}")
    if not isinstance(data, pd.DataFrame):
        raise ValueError(f"data must be a pandas.DataFrame instance. Got {type(data)}")
    if set(model.nodes()) != set(data.columns):
        raise ValueError("Missing columns in data. Can't find values for the following variables: "
                         f" {set(model.nodes()) - set(data.columns)}")


def log_likelihood_score(model, data):
    """log P(data | model) (metrics.py:176-219): the reference's checks (the model's type, a DataFrame
    whose columns are the model's nodes, check_model), then BayesianModelProbability(model).score(data):
    one pass over the codes on the device."""
    _check_model_and_frame(model, data, "log_likelihood_score")
    model.check_model()
    return BayesianModelProbability(model).score(data)


def f1_score(y_true, y_pred):
    """The binary F1 of scikit-learn's default (positive class True; 0.0 when there is no true or
    predicted positive), written out so that scikit-learn is no runtime dependency."""
    y_true, y_pred = np.asarray(y_true, dtype=bool), np.asarray(y_pred, dtype=bool)
    tp = int(np.sum(y_true & y_pred))
    fp = int(np.sum(~y_true & y_pred))
    fn = int(np.sum(y_true & ~y_pred))
    return 0.0 if tp == 0 else 2.0 * tp / (2.0 * tp + fp + fn)


def _builtin_lambda(test):
    """scipy's lambda_ name of a built-in test given by name or as the function itself (None: a
    callable of the caller's, tested pair by pair)."""
    from ..estimators import CITests as C

    fn = C.get_callable_ci_test(test)
    if fn in C.BUILTIN_LAMBDA:
        return fn, (C.BUILTIN_LAMBDA[fn] or "cressie-read")
    return fn, None


def correlation_score(model, data, test="chi_square", significance_level=0.05, score=None, return_summary=False):
    """How well the structure's d-connections match the correlations in `data` (metrics.py:59-173).
    Every pair of variables is tested without conditioning (true label: p-value >= significance_level)
    and asked whether it is d-connected in the model (predicted label: NOT d-connected); `score` (default:
    the binary F1, f1_score; any callable taking y_true=, y_pred=) compares the two.  A built-in test
    (by name or as the function) runs every pair in one CITester.tests call; any other callable is called
    pair by pair as test(X=, Y=, Z=[], data=, boolean=True, significance_level=).  return_summary returns
    the frame (var1, var2, stat_test, d_connected), the reference's column names: d_connected holds
    "not d-connected"."""
    import pandas as pd

    from ..estimators.CITests import CITester

    _check_model_and_frame(model, data, "correlation_score")
    fn, lam = _builtin_lambda(test)
    score = f1_score if score is None else score
    if not callable(score):
        raise ValueError(f"score should be a classification metric taking y_true and y_pred. Got {score}")
    pairs = list(combinations(model.nodes(), 2))
    if lam is not None:
        stat_test = CITester(data).independent([(i, j, []) for i, j in pairs], significance_level, lam)
    else:
        stat_test = [fn(X=i, Y=j, Z=[], data=data, boolean=True, significance_level=significance_level)
                     for i, j in pairs]
    trails = model.active_trail_nodes(list(model.nodes()))
    results = pd.DataFrame({"var1": [i for i, _ in pairs], "var2": [j for _, j in pairs],
                            "stat_test": np.asarray(stat_test, dtype=bool),
                            "d_connected": np.asarray([j not in trails[i] for i, j in pairs], dtype=bool)},
                           columns=["var1", "var2", "stat_test", "d_connected"])
    if return_summary:
        return results
    return score(y_true=results["stat_test"].values, y_pred=results["d_connected"].values)


def chi2_sf_even(C, k):
    """The chi-square survival function at `C` with the even degree of freedom 2 k: the closed form
    exp(-C / 2) sum_{i < k} (C / 2)^i / i!.  Each term is exp(i log x - x - log i!) relative to the
    largest one, so nothing overflows for k in the thousands; the terms are formed and added in extended
    precision, from the smallest up."""
    k = int(k)
    if k <= 0:
        return float("nan")
    x = float(C) / 2.0
    if not x > 0.0:
        return 1.0
    i = np.arange(k, dtype=np.longdouble)
    lg = np.concatenate([np.zeros(1, dtype=np.longdouble), np.cumsum(np.log(i[1:]))])  # log i!
    t = i * np.log(np.longdouble(x)) - np.longdouble(x) - lg
    top = t.max()
    s = np.sort(np.exp(t - top)).sum(dtype=np.longdouble)
    return float(min(np.exp(top) * s, np.longdouble(1.0)))


def fisher_c(model, data, ci_test, compute_rmsea=False, show_progress=True):
    """Fisher's C test of the model structure against `data` (metrics.py:379-466): for every non-adjacent
    pair (u, v) the test u _|_ v | parents(u) + parents(v), p-values clipped at 1e-6, C = -2 sum log p,
    and the chi-square survival function at 2 k degrees of freedom (chi2_sf_even: no scipy).  A built-in
    ci_test (by name or as the function) runs every pair through one CITester; any other callable is
    called pair by pair as ci_test(X=, Y=, Z=, data=, boolean=False) and its second result is the p-value.
    Returns the p-value, or (p-value, RMSEA) with compute_rmsea.  show_progress is accepted and ignored."""
    from ..estimators.CITests import CITester
    from ..models import DiscreteBayesianNetwork

    if not isinstance(model, DiscreteBayesianNetwork):
        raise ValueError(f"model must be an instance of DiscreteBayesianNetwork. Got {type(model)}")
    if len(model.latents) > 0:
        raise ValueError("This test can not be performed on models with latent variables.")
    fn, lam = _builtin_lambda(ci_test)
    triples = []
    for u, v in combinations(model.nodes(), 2):
        if not (model.has_edge(u, v) or model.has_edge(v, u)):
            parents = list(model.predecessors(u))
            triples.append((u, v, parents + [z for z in model.predecessors(v) if z not in parents]))
    if lam is not None:
        pvalues = CITester(data).tests(triples, lam)[1] if triples else np.zeros(0)
    else:
        pvalues = np.array([fn(X=u, Y=v, Z=set(Z), data=data, boolean=False)[1] for u, v, Z in triples], dtype=np.float64)
    k = len(triples)
    C = float(-2.0 * np.log(np.clip(pvalues, 1e-6, None)).sum())
    p_value = chi2_sf_even(C, k)
    if not compute_rmsea:
        return p_value
    rmsea = float("nan")
    if len(data) != 1 and k != 0:
        rmsea = math.sqrt(max((C - 2 * k) / (2 * k * (len(data) - 1)), 0))
    return p_value, rmsea


def SHD(true_model, est_model):
    """The structural Hamming distance (metrics.py:469-550): edges to delete, to add and to reverse, each
    counting 1."""
    if set(true_model.nodes()) != set(est_model.nodes()):
        raise ValueError("The graphs must have the same nodes.")
    nodes = list(true_model.nodes())
    pos = {v: i for i, v in enumerate(nodes)}

    def adjacency(g):
        m = np.zeros((len(nodes), len(nodes)), dtype=np.int64)
        for u, v in g.edges():
            m[pos[u], pos[v]] = 1
        return m

    m1, m2 = adjacency(true_model), adjacency(est_model)
    shd = 0
    ds = (m1 + m1.T) - (m2 + m2.T)
    ind = np.where(ds > 0)  # in the true model only: deletions
    m1[ind] = 0
    shd += len(ind[0]) / 2
    ind = np.where(ds < 0)  # in the estimated model only: additions
    m1[ind] = m2[ind]
    shd += len(ind[0]) / 2
    d = np.abs(m1 - m2)  # what is left differs in direction
    shd += np.sum((d + d.T) > 0) / 2
    return int(shd)
