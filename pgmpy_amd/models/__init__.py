from .ClusterGraph import ClusterGraph
from .DiscreteBayesianNetwork import DiscreteBayesianNetwork
from .DiscreteMarkovNetwork import DiscreteMarkovNetwork
from .DynamicBayesianNetwork import DynamicBayesianNetwork, DynamicNode
from .FactorGraph import FactorGraph
from .JunctionTree import JunctionTree
from .LinearGaussianBayesianNetwork import LinearGaussianBayesianNetwork
from .NaiveBayes import NaiveBayes

# pgmpy < 1.0 names
BayesianNetwork = DiscreteBayesianNetwork
MarkovNetwork = DiscreteMarkovNetwork

__all__ = ["ClusterGraph", "DiscreteBayesianNetwork", "BayesianNetwork", "DiscreteMarkovNetwork", "MarkovNetwork",
           "DynamicBayesianNetwork", "DynamicNode", "FactorGraph", "JunctionTree", "LinearGaussianBayesianNetwork",
           "NaiveBayes"]
