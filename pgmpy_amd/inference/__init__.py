from .base import Inference
from .ExactInference import BeliefPropagation, BeliefPropagationWithMessagePassing, VariableElimination
from .ApproxInference import ApproxInference
from .dbn_inference import DBNInference

__all__ = ["Inference", "VariableElimination", "BeliefPropagation", "BeliefPropagationWithMessagePassing",
           "ApproxInference", "DBNInference"]
