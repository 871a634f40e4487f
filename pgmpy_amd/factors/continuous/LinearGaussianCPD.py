"""LinearGaussianCPD: P(Y | x_1 .. x_k) = N(beta_0 + beta_1 x_1 + ... + beta_k x_k; std), a host class with
pgmpy's names (pgmpy/factors/continuous/LinearGaussianCPD.py).  The numbers live on the host; the kernels
of LinearGaussianBayesianNetwork take them as one coefficient array per call."""
import numpy as np

from ..base import BaseFactor


class LinearGaussianCPD(BaseFactor):
    def __init__(self, variable, beta, std, evidence=[]):
        try:
            hash(variable)
        except TypeError:
            raise ValueError(f"`variable` argument must be hashable, Got {type(variable).__name__}")
        self.variable = variable
        self.beta = np.array(beta)  # beta[0] is the intercept, beta[1 + i] goes with evidence[i]
        self.std = std
        self.evidence = list(evidence)
        self.variables = [variable] + self.evidence

    def copy(self):
        return LinearGaussianCPD(self.variable, self.beta, self.std, list(self.evidence))

    def __str__(self):
        beta, std = self.beta.round(3), round(self.std, 3)
        if not (self.evidence and list(self.beta)):
            return f"P({self.variable}) = N({beta[0]}; {std})"
        terms = [f"{b}*{p}" for b, p in zip(beta[1:], self.evidence)] + [str(beta[0])]
        return f"P({self.variable} | {', '.join(map(str, self.evidence))}) = N({' + '.join(terms)}; {std})"

    def __repr__(self):
        return f"<LinearGaussianCPD: {self} at {hex(id(self))}"

    @staticmethod
    def get_random(variable, evidence, loc=0.0, scale=1.0, seed=None):
        """beta ~ N(loc, scale) per entry, std = |N(loc, scale)|: numpy's default_rng(seed) draws, beta first."""
        rng = np.random.default_rng(seed=seed)
        beta = rng.normal(loc=loc, scale=scale, size=len(evidence) + 1)
        std = abs(rng.normal(loc=loc, scale=scale))
        return LinearGaussianCPD(variable, beta, std, evidence)
