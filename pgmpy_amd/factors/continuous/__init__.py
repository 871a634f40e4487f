from .LinearGaussianCPD import LinearGaussianCPD

__all__ = ["LinearGaussianCPD"]
