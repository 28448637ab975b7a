"""What the environment receives from a policy head that samples unbounded actions (the diagonal-Gaussian head): a thin wrapper
that clips the actions in step() and delegates everything else.  The experience buffer keeps the UNCLIPPED samples -- the ratio is
about the sample, as in Stable-Baselines3.  One mechanism for both collection modes and no change to the wire format: Learner
wraps `env_create_function` in a ClippedEnvFactory, so the environment is built wrapped wherever it is built (inside the worker
process in process mode, in the learner process around the vector environment in vector mode).  Both classes pickle (the spawn
path) as long as the wrapped factory does."""
import math

import numpy as np
import torch


def check_clip(clip):
    """None, or (lo, hi) finite with lo < hi -> None or (float, float)."""
    if clip is None:
        return None
    try:
        lo, hi = (float(x) for x in clip)
    except (TypeError, ValueError):
        raise ValueError(f"continuous_action_clip must be None or a pair (lo, hi), got {clip!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError(f"continuous_action_clip needs finite lo < hi, got {clip!r}")
    return lo, hi


class ActionClipEnv:
    """env with step(clip(actions, lo, hi)); every other attribute (spaces, reset, action_masks, close, ...) is the environment's."""

    def __init__(self, env, lo, hi):
        self._env, self._lo, self._hi = env, np.float32(lo), np.float32(hi)

    def step(self, actions):
        if isinstance(actions, torch.Tensor):   # a device-resident vector environment: out of place, dtype and device kept
            return self._env.step(torch.clamp(actions, float(self._lo), float(self._hi)))
        return self._env.step(np.clip(np.asarray(actions, dtype=np.float32), self._lo, self._hi))

    def __getattr__(self, name):   # (only reached for what the wrapper does not define itself)
        if name.startswith("__") or name in ("_env", "_lo", "_hi"):   # copy / pickle probe before __init__ has run
            raise AttributeError(name)
        return getattr(self._env, name)

    def __getstate__(self):
        return {"_env": self._env, "_lo": self._lo, "_hi": self._hi}

    def __setstate__(self, state):
        self.__dict__.update(state)


class ClippedEnvFactory:
    """() -> ActionClipEnv(build_env_fn(), lo, hi)."""

    def __init__(self, build_env_fn, lo, hi):
        self.build_env_fn, self.lo, self.hi = build_env_fn, float(lo), float(hi)

    def __call__(self):
        return ActionClipEnv(self.build_env_fn(), self.lo, self.hi)
