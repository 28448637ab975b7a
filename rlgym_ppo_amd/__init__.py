"""rlgym_ppo_amd -- MI355X-native hot path of rlgym-ppo (rollout inference -> GAE -> PPO update) behind the
reference's Python API:  `from rlgym_ppo_amd import Learner` mirrors `from rlgym_ppo import Learner`
(reference: rlgym_ppo/__init__.py:1).  Sub-packages mirror the reference's: .ppo, .util, .batched_agents."""

import gc
import os

__version__ = "0.1.0"

# A forked child (multiprocessing's default start method: a Manager, a fork-started worker) inherits the parent's heap, unreachable
# cycles included, but not its GPU: the HIP runtime's threads and queues do not cross a fork.  If the child's collector came across
# an inherited dead cycle that owns a graph, an event or a host window, the destructor would call the HIP runtime in a process where
# it cannot run -- a segmentation fault at whatever allocation happens to start a collection.  Freezing the inherited heap right
# after the fork takes every object that existed then out of the child's collections (what gc.freeze() is for); the parent, which
# owns the resources, collects and releases them as always.
if hasattr(os, "register_at_fork"):
    os.register_at_fork(after_in_child=gc.freeze)


def __getattr__(name):  # lazy: importing the package must not spawn anything or touch the GPU
    if name == "Learner":
        from .learner import Learner
        return Learner
    raise AttributeError(name)
