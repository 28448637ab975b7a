"""Vector environments behind the DEVICE interface of VectorAgentManager (reset() / step() answer GPU tensors), for
tests/test_gpu_device_env.py and tools/device_env_cost.py.

DeviceTwin(host_env): any numpy vector environment behind the device interface.  It copies through the host internally -- the
environment's own wait, which the interface allows -- so the same interaction sequence can be collected through both interfaces.

IntegerEnv: ONE environment written once over a tiny backend (numpy on the host, torch on the device).  Its state is integers
and every float it emits is one IEEE operation on small integers (an exact division by 4, an exact multiplication by 0.125), so
the two backends agree bit for bit; the torch backend never reads the device.  Rewards depend on the actions, episode lengths differ
per agent, every third agent meets a time limit every 4 steps, the others terminate."""
import numpy as np
import torch

from synthetic_env import Box, Discrete, SyntheticVectorEnv, _Space


class DeviceTwin(object):
    def __init__(self, host_env, device="cuda:0"):
        self._env, self._dev = host_env, torch.device(device)

    def _up(self, x, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype))).to(self._dev)

    def reset(self):
        return self._up(self._env.reset())

    def step(self, actions):
        assert isinstance(actions, torch.Tensor) and actions.is_cuda and actions.dtype == torch.float32
        out = self._env.step(actions.cpu().numpy())
        info = out[-1]
        if isinstance(info, dict) and "final_observation" in info:
            info = dict(info, final_observation=self._up(info["final_observation"]))
        return (self._up(out[0]), self._up(out[1], np.float32)) + tuple(self._up(f) for f in out[2:-1]) + (info,)

    def __getattr__(self, name):
        if name.startswith("__") or name in ("_env", "_dev"):
            raise AttributeError(name)
        got = getattr(self._env, name)          # (an environment without action_masks() stays one without)
        if name == "action_masks":
            return lambda: self._up(np.asarray(got()) != 0)
        return got


class IntegerEnv(object):
    """device=None: numpy arrays (the host interface); a torch device: tensors on it (the device interface)."""

    def __init__(self, n_agents=64, obs_dim=107, n_actions=90, device=None, masks=False, final_obs=False, flags="float32"):
        self.n, self.d, self.A, self.dev, self.final_obs, self.flags = n_agents, obs_dim, n_actions, device, final_obs, flags
        self.observation_space = _Space(shape=(obs_dim,))
        self.action_space = Discrete(n=n_actions)
        self.a = self._arange(n_agents)
        self.j = self._arange(obs_dim)
        self.c = self._arange(n_actions)
        self.ep_len = 3 + (self.a * 5) % 7
        self.t = self.a * 0
        self.g = 0                               # steps so far: a host integer in both backends
        if masks:
            self.action_masks = self._masks

    def _arange(self, n):
        return np.arange(n, dtype=np.int64) if self.dev is None else torch.arange(n, dtype=torch.int64, device=self.dev)

    def _f32(self, x):
        return x.astype(np.float32) if self.dev is None else x.to(torch.float32)

    def _obs(self, t):
        k = (self.a[:, None] * 31 + self.j[None, :] * 17 + t[:, None] * 7 + self.g * 3) % 23 - 11
        return self._f32(k) / 4.0                # one exact division

    def _masks(self):
        return (self.c[None, :] + self.t[:, None] + self.a[:, None]) % 3 != 0

    def reset(self):
        self.t, self.g = self.a * 0, 0
        return self._obs(self.t)

    def step(self, actions):
        if self.dev is None:
            act = np.asarray(actions, np.float32).reshape(self.n, -1)[:, 0].astype(np.int64)
        else:
            assert isinstance(actions, torch.Tensor) and actions.is_cuda and actions.dtype == torch.float32
            act = actions.reshape(self.n, -1)[:, 0].to(torch.int64)
        self.t = self.t + 1
        self.g += 1
        rew = self._f32((act + self.t) % 9 - 4) * 0.125     # one exact multiplication
        done = self.t >= self.ep_len
        trunc = (~done) & (self.t % 4 == 0) & (self.a % 3 == 0)
        info = {"state": None}
        if self.final_obs:
            info["final_observation"] = self._obs(self.t)
        self.t = self.t * (~(done | trunc))
        if self.flags == "float32":
            done, trunc = self._f32(done), self._f32(trunc)
        return self._obs(self.t), rew, done, trunc, info

    def close(self):
        pass


def make_integer_device_env():
    return IntegerEnv(device=torch.device("cuda:0"))


def make_integer_host_env():
    return IntegerEnv()


class MaskedSyntheticVectorEnv(SyntheticVectorEnv):
    """SyntheticVectorEnv with action_masks(): a third of the actions invalid, moving with the agents' step counters."""

    def action_masks(self):
        c = np.arange(self.action_space.n)
        return (c[None, :] + self.t[:, None] + np.arange(self.n_agents)[:, None]) % 3 != 0


__all__ = ["Box", "DeviceTwin", "IntegerEnv", "MaskedSyntheticVectorEnv", "make_integer_device_env", "make_integer_host_env"]
