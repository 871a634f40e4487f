from .base import Inference
from .ExactInference import BeliefPropagation, BeliefPropagationWithMessagePassing, VariableElimination
from .ApproxInference import ApproxInference
from .dbn_inference import DBNInference
from .Mplp import Mplp
from .LoopyBeliefPropagation import LoopyBeliefPropagation

__all__ = ["Inference", "VariableElimination", "BeliefPropagation", "BeliefPropagationWithMessagePassing",
           "ApproxInference", "DBNInference", "Mplp", "LoopyBeliefPropagation"]
