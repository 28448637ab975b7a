from ._mlp import LayerSizes, ValueBins
from .continuous_policy import ContinuousPolicy
from .diag_gaussian_policy import DiagGaussianPolicy
from .multi_discrete_policy import MultiDiscreteFF
from .discrete_policy import DiscreteFF
from .value_estimator import ValueEstimator
from .hybrid_policy import HybridPolicy
from .ppo_learner import HybridSpace, ObsSizes, PPOLearner, ValueNorm
from .experience_buffer import ExperienceBuffer
from .symmetry import Symmetry
