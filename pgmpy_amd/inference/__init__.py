from .base import Inference
from .ExactInference import BeliefPropagation, BeliefPropagationWithMessagePassing, VariableElimination
from .ApproxInference import ApproxInference

__all__ = ["Inference", "VariableElimination", "BeliefPropagation", "BeliefPropagationWithMessagePassing",
           "ApproxInference"]
