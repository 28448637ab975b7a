"""Small discrete environments WITH action_masks() for process-mode collection (importable by worker processes): the mask is a
deterministic function of the raw observation the agents act on next -- `mask_of` -- so a test can recompute the mask of every
stored state (with standardize_obs=False).  Every mask row has at least one valid action (ZeroRowEnv apart, which exists to
break that rule once)."""
import numpy as np

import synthetic_env


def mask_of(obs, n_actions):
    """obs [n, d] (or [d]) float32 -> bool [n, n_actions] (or [n_actions]): action c is valid unless floor(4 |obs[c % d]|) is a
    multiple of 3; action floor(10 |obs[0]|) % n_actions is always valid."""
    o = np.asarray(obs, dtype=np.float32)
    rows = o.reshape(1, -1) if o.ndim == 1 else o
    cols = np.arange(n_actions) % rows.shape[1]
    m = (np.floor(np.abs(rows[:, cols]) * np.float32(4.0)).astype(np.int64) % 3) != 0
    sure = np.floor(np.abs(rows[:, 0]) * np.float32(10.0)).astype(np.int64) % n_actions
    m[np.arange(rows.shape[0]), sure] = True
    return m[0] if o.ndim == 1 else m


class _Masked:
    """Mixin: remembers the observation the agents act on next and answers action_masks() for it."""

    def reset(self):
        self._last = super().reset()
        return self._last

    def step(self, actions):
        out = super().step(actions)
        self._last = out[0]
        return out

    def action_masks(self):
        return mask_of(self._last, self.action_space.n)


class MaskedWireEnv(_Masked, synthetic_env.SyntheticEnv):
    pass


class MaskedSingleEnv(_Masked, synthetic_env.SyntheticSingleEnv):
    pass


class MaskedVaryingEnv(_Masked, synthetic_env.SyntheticVaryingEnv):
    pass


class ZeroRowEnv(MaskedWireEnv):
    """Reports a mask row without a valid action (agent 1) for the observation after its third step."""

    def action_masks(self):
        m = super().action_masks()
        if self.t == 3:
            m[1, :] = False
        return m


def make_masked_wire_env():      # two agents, 13 features, 7 actions
    return MaskedWireEnv(obs_dim=13, n_actions=7, n_agents=2, ep_len=5, seed=2)


def make_masked_single_env():    # one agent, rank-1 observations (and a [n_actions] mask)
    return MaskedSingleEnv()


def make_masked_varying_env():   # team size 2 -> 3 -> 1 -> ... across resets
    return MaskedVaryingEnv()


def make_zero_row_env():
    return ZeroRowEnv(obs_dim=13, n_actions=7, n_agents=2, ep_len=5, seed=2)


def make_masked_env_90():        # the end-to-end test: 90 actions (three mask words)
    return MaskedWireEnv(obs_dim=31, n_actions=90, n_agents=2, ep_len=9, seed=7)
