"""Small gym-free environments with a MultiDiscrete((2, 7, 3, 11, 2)) action space (tests/test_gpu_multidiscrete_learner.py): one for
the process-per-environment workers, one vectorised.  An action outside nvec cannot be reported from a worker process by an
exception the learner would see, so it is reported through the reward: every such step pays OUT_OF_RANGE_REWARD."""
import numpy as np

NVEC = (2, 7, 3, 11, 2)
OBS_DIM = 23
OUT_OF_RANGE_REWARD = 1000.0


class MultiDiscrete:
    def __init__(self, nvec):
        self.nvec = np.asarray(nvec, np.int64)
        self.shape = self.nvec.shape

    def seed(self, s):
        pass


class _Space:
    def __init__(self, shape):
        self.shape = shape


def _penalty(actions, n_agents):
    a = np.asarray(actions, np.float64).reshape(n_agents, -1)
    ok = a.shape[1] == len(NVEC) and (a == np.floor(a)).all() and (a >= 0).all() and (a < np.asarray(NVEC)).all()
    return 0.0 if ok else OUT_OF_RANGE_REWARD


class NvecEnv:
    """Two agents, episodes of 9 steps; the reward favours high indices (so it depends on the actions) and is far below the penalty."""

    def __init__(self, seed=0):
        self.n_agents, self.ep_len, self.t = 2, 9, 0
        self.rs = np.random.RandomState(seed)
        self.observation_space = _Space((OBS_DIM,))
        self.action_space = MultiDiscrete(NVEC)

    def _obs(self):
        return (self.rs.randn(self.n_agents, OBS_DIM) * 2 + 0.5).astype(np.float32)

    def reset(self):
        self.t = 0
        return self._obs()

    def step(self, actions):
        self.t += 1
        pen = _penalty(actions, self.n_agents)
        a = np.asarray(actions, np.float64).reshape(self.n_agents, -1)
        rew = [float(np.tanh(a[i].sum() * 0.05) + self.rs.randn() * 0.1 + pen) for i in range(self.n_agents)]
        done = self.t >= self.ep_len
        return self._obs(), rew, done, (not done) and self.t % 4 == 0, {"state": None}

    def close(self):
        pass


class NvecVectorEnv:
    """Twelve agents in lockstep with auto-reset (the interface of batched_agents/vector_agent_manager.py); keeps the largest
    index seen per head."""

    def __init__(self, seed=0, nvec=NVEC):
        self.n_agents = 12
        self.rs = np.random.RandomState(seed)
        self.observation_space = _Space((OBS_DIM,))
        self.action_space = MultiDiscrete(nvec)
        self.ep_len = 5 + (np.arange(self.n_agents) * 7) % 6
        self.t = np.zeros(self.n_agents, np.int64)
        self.seen_max = np.full(len(NVEC), -1, np.int64)
        self.out_of_range_steps = 0

    def _obs(self):
        return (self.rs.randn(self.n_agents, OBS_DIM) * 2 + 0.5).astype(np.float32)

    def reset(self):
        self.t[:] = 0
        return self._obs()

    def step(self, actions):
        a = np.asarray(actions, np.float64).reshape(self.n_agents, -1)
        pen = _penalty(a, self.n_agents)
        self.out_of_range_steps += int(pen != 0)
        if a.shape[1] == len(NVEC):
            self.seen_max = np.maximum(self.seen_max, a.max(0).astype(np.int64))
        self.t += 1
        rew = (np.tanh(a.sum(1) * 0.05) + self.rs.randn(self.n_agents) * 0.1 + pen).astype(np.float32)
        done = self.t >= self.ep_len
        self.t[done] = 0
        return self._obs(), rew, done.astype(np.float32), np.zeros(self.n_agents, np.float32), {"state": None}

    def close(self):
        pass


def make_env():
    return NvecEnv()


def make_vector_env():
    return NvecVectorEnv()
