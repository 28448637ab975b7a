"""Small synthetic vector environments with critic_observations() (Learner(critic_observations=True)), a numpy one and a device-resident
one, modelled on tests/synthetic_env.py / tests/device_vector_env.py.

CriticVectorEnv: its whole state is ONE step counter (tests/diag_gaussian_env.py::CounterVectorEnv): observations, critic
observations and the done / truncated flags of step t are functions of t alone, rewards depend on the actions, and reset() returns
the observation of the current t without touching it -- so an environment built with start = t0 is where one built with start = 0 is
after t0 steps (what a test needs to continue a run in a second Learner), and two policies that disagree on a near-tie still see the
same observation stream.
  alias=True:  critic_observations() is the observation itself -- a run with critic_observations=True must then be the run without it,
               bit for bit;
  alias=False: the observation (width 13) ++ 16 deterministic features of the step counter and the agent index (critic width 29):
               what a simulator knows and the robot does not.

CriticDeviceTwin: the same environment behind the device interface (it copies through the host internally: the environment's own wait,
which the interface allows), so the same interaction sequence can be collected through all three collect paths."""
import numpy as np

from device_vector_env import DeviceTwin
from synthetic_env import Discrete, _Space

OBS, EXTRA, N_ACTIONS = 13, 16, 6
CRITIC_OBS = OBS + EXTRA


class NoCriticEnv:
    """The environment WITHOUT critic_observations()."""

    def __init__(self, start=0, n_agents=8, alias=False):
        self.n_agents, self.t, self.alias = n_agents, int(start), alias
        self.observation_space = _Space(shape=(OBS,))
        self.action_space = Discrete(n=N_ACTIONS)
        self.critic_calls = 0

    def obs_at(self, t):
        return (np.random.RandomState(1000 + t).randn(self.n_agents, OBS) * 2 + 0.5).astype(np.float32)

    def reset(self):
        return self.obs_at(self.t)

    def step(self, actions):
        a = np.asarray(actions, np.float32).reshape(self.n_agents, -1)
        rew = (a.sum(1) * np.float32(0.125) - np.float32(0.25)).astype(np.float32)
        self.t += 1
        who = np.arange(self.n_agents)
        done = (self.t + who) % 9 == 0
        trunc = ~done & ((self.t + 2 * who) % 11 == 0)
        return self.obs_at(self.t), rew, done.astype(np.float32), trunc.astype(np.float32), {"state": None}

    def close(self):
        pass


class CriticVectorEnv(NoCriticEnv):
    def critic_obs_at(self, t):
        if self.alias:
            return self.obs_at(t)
        j, who = np.arange(EXTRA, dtype=np.float32), np.arange(self.n_agents, dtype=np.float32)
        extra = np.sin(np.float32(0.37) * np.float32(t) + np.float32(0.11) * j[None, :] + who[:, None]) * np.float32(3.0) + who[:, None] * np.float32(0.25)
        return np.concatenate([self.obs_at(t), extra.astype(np.float32)], axis=1)

    def critic_observations(self):
        """For the observation the agents act on next: the one reset() / the last step() returned."""
        self.critic_calls += 1
        return self.critic_obs_at(self.t)


class CriticDeviceTwin(DeviceTwin):
    def critic_observations(self):
        return self._up(self._env.critic_observations(), np.float32)


def make(alias, device=False, start=0, **kw):
    def build():
        env = CriticVectorEnv(start=start, alias=alias, **kw)
        return CriticDeviceTwin(env) if device else env
    return build
