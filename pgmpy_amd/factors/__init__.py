from .base import BaseFactor, factor_divide, factor_product, factor_sum_product
from .continuous import LinearGaussianCPD

__all__ = ["BaseFactor", "factor_product", "factor_sum_product", "factor_divide", "LinearGaussianCPD"]
