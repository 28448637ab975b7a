"""Small MultiDiscrete environments WITH action_masks() for process-mode collection (importable by worker processes), modelled on
masked_wire_env.py and multidiscrete_env.py: a mask row has one entry per LOGIT, [n_agents, S = sum(nvec)], head h owning columns
[s_h, s_h + b_h), and is a deterministic function of the raw observation the agents act on next -- `mask_of` -- so a test can
recompute the mask of every stored state (with standardize_obs=False).  Every head of every row keeps a valid bin (EmptyHeadEnv
apart, which exists to break that rule once).  An action outside nvec is reported through the reward, as in multidiscrete_env.py."""
import numpy as np

import multidiscrete_env as E

NVEC = E.NVEC            # (2, 7, 3, 11, 2): S = 25, one mask word
OBS_DIM = E.OBS_DIM


def starts(nvec):
    return [int(s) for s in np.cumsum((0,) + tuple(nvec))[:-1]]


def mask_of(obs, nvec=NVEC):
    """obs [n, d] (or [d]) float32 -> bool [n, S] (or [S]): logit c is valid unless floor(4 |obs[c % d]|) is a multiple of 3; in head
    h the bin floor(10 |obs[h]|) % b_h is always valid."""
    o = np.asarray(obs, dtype=np.float32)
    rows = o.reshape(1, -1) if o.ndim == 1 else o
    S = int(sum(nvec))
    cols = np.arange(S) % rows.shape[1]
    m = (np.floor(np.abs(rows[:, cols]) * np.float32(4.0)).astype(np.int64) % 3) != 0
    for h, (s, b) in enumerate(zip(starts(nvec), nvec)):
        sure = np.floor(np.abs(rows[:, h % rows.shape[1]]) * np.float32(10.0)).astype(np.int64) % int(b)
        m[np.arange(rows.shape[0]), s + sure] = True
    return m[0] if o.ndim == 1 else m


def head_valid_actions(mask, actions, nvec=NVEC):
    """bool [n]: every component of every action row [n, H] is a valid bin of its head under mask [n, S]."""
    a = np.asarray(actions).reshape(len(mask), len(nvec)).astype(np.int64)
    ok = np.ones(len(mask), bool)
    for h, (s, b) in enumerate(zip(starts(nvec), nvec)):
        ok &= (a[:, h] >= 0) & (a[:, h] < b)
        ok &= mask[np.arange(len(mask)), s + np.clip(a[:, h], 0, b - 1)]
    return ok


class MaskedNvecEnv(E.NvecEnv):
    """NvecEnv (two agents, episodes of 9 steps) that remembers the observation the agents act on next and answers action_masks()
    for it."""

    def reset(self):
        self._last = super().reset()
        return self._last

    def step(self, actions):
        out = super().step(actions)
        self._last = out[0]
        return out

    def action_masks(self):
        return mask_of(self._last)


class MaskedNvecSingleEnv(MaskedNvecEnv):
    """One agent, rank-1 observations and a rank-1 [S] mask."""

    def __init__(self, seed=0):
        super().__init__(seed)
        self.n_agents = 1

    def _obs(self):
        return super()._obs()[0]

    def step(self, actions):
        obs, rew, done, trunc, info = super().step(actions)
        return obs, rew[0], done, trunc, info


class EmptyHeadEnv(MaskedNvecEnv):
    """Reports a mask whose head 1 (bins 2 .. 8) is empty for agent 1, for the observation after its third step."""

    def action_masks(self):
        m = super().action_masks()
        if self.t == 3:
            m[1, 2:9] = False
        return m


class NarrowMaskEnv(MaskedNvecEnv):
    """Answers one entry per COMPONENT (5) instead of one per logit (25): the width the learner must refuse."""

    def action_masks(self):
        return np.ones((self.n_agents, len(NVEC)), bool)


def make_masked_nvec_env():
    return MaskedNvecEnv()


def make_masked_nvec_single_env():
    return MaskedNvecSingleEnv()


def make_empty_head_env():
    return EmptyHeadEnv()


def make_narrow_mask_env():
    return NarrowMaskEnv()
