"""Graph base classes (mirror of pgmpy/base).  Built: PDAG."""
from .PDAG import PDAG

__all__ = ["PDAG"]
