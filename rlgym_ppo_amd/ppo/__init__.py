from ._mlp import LayerSizes
from .continuous_policy import ContinuousPolicy
from .diag_gaussian_policy import DiagGaussianPolicy
from .multi_discrete_policy import MultiDiscreteFF
from .discrete_policy import DiscreteFF
from .value_estimator import ValueEstimator
from .ppo_learner import ObsSizes, PPOLearner, ValueNorm
from .experience_buffer import ExperienceBuffer
