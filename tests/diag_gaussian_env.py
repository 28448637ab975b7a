"""Continuous synthetic environments that REPORT what they were handed: the reward of an agent's step is max_j |action_j| as the
environment received it (no noise), so a test that only sees the experience buffer -- process-mode workers live in other processes
-- can tell whether an action outside the clip range ever reached an environment, while the buffer's own `actions` hold what the
policy sampled.  Observations do not depend on the actions."""
import numpy as np

import synthetic_env

OBS_DIM, K = 13, 3


class EchoEnv(synthetic_env.SyntheticEnv):
    def __init__(self):
        super().__init__(obs_dim=OBS_DIM, n_actions=K, n_agents=2, ep_len=6, seed=4, kind="continuous")

    def step(self, actions):
        out = list(super().step(actions))
        out[1] = [float(np.abs(np.asarray(actions, np.float64)[i]).max()) for i in range(self.n_agents)]
        return tuple(out)


def make_echo_env():
    return EchoEnv()


class EchoVectorEnv(synthetic_env.SyntheticVectorEnv):
    def __init__(self):
        super().__init__(obs_dim=OBS_DIM, n_actions=K, n_agents=16, seed=0, kind="continuous")

    def step(self, actions):
        out = list(super().step(actions))
        out[1] = np.abs(np.asarray(actions, np.float32).reshape(self.n_agents, -1)).max(1).astype(np.float32)
        return tuple(out)


def make_echo_vector_env():
    return EchoVectorEnv()


class CounterVectorEnv:
    """A vectorised echo environment whose whole state is ONE step counter: the observations, done and truncated flags of step t are
    a function of t alone (the reward echoes max |action| as above), and reset() returns the observation of the current t without
    touching it.  An environment built with start = t0 is therefore exactly where one built with start = 0 is after t0 steps --
    what a test needs to continue a run in a second Learner (an environment is not checkpoint state)."""

    def __init__(self, start=0, n_agents=16):
        self.n_agents, self.t = n_agents, int(start)
        self.observation_space = synthetic_env._Space(shape=(OBS_DIM,))
        self.action_space = synthetic_env.Box(shape=(K,))

    def _obs(self):
        return (np.random.RandomState(1000 + self.t).randn(self.n_agents, OBS_DIM) * 2 + 0.5).astype(np.float32)

    def reset(self):
        return self._obs()

    def step(self, actions):
        rew = np.abs(np.asarray(actions, np.float32).reshape(self.n_agents, -1)).max(1).astype(np.float32)
        self.t += 1
        who = np.arange(self.n_agents)
        done = (self.t + who) % 9 == 0
        trunc = ~done & ((self.t + 2 * who) % 11 == 0)
        return self._obs(), rew, done.astype(np.float32), trunc.astype(np.float32), {"state": None}

    def close(self):
        pass
