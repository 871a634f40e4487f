"""pgmpy_amd — MI355X-native (gfx950) engine for pgmpy's discrete-factor hot path.

Drop-in mirror of the pgmpy API surface for DiscreteFactor / TabularCPD,
VariableElimination, BeliefPropagation, DiscreteBayesianNetwork.predict /
predict_probability / fit / simulate and BayesianModelSampling; every factor operation runs in
hand-written HIP kernels (pgmpy_amd/csrc/pgmhip.hip, pgmrows.hip, pgmfit.hip, pgmsample.hip) reached
through the C-ABI of include/pgmhip.h.
"""
__version__ = "0.1.0"
ABI_VERSION = 25  # pgm_version() of the library the ctypes mirrors in _native.py are written for
