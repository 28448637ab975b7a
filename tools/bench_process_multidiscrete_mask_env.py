"""bench_process_env.BenchProcessEnv with a MultiDiscrete(NVEC) action space, with and without action_masks(): pre-drawn masks, one
entry per logit, two-thirds valid, every head of every row with a valid bin, one per pre-drawn observation -- the synthetic
environment of tools/multidiscrete_process_mask_cost.py's process_collect leg.  Imported by the worker processes."""
import numpy as np

import bench_process_env as B

NVEC = (5, 5, 3, 3, 3, 2, 2, 2)   # not the reference's fixed bins: masked and unmasked runs both take the general kernels
S = sum(NVEC)


class MultiDiscrete:
    def __init__(self, nvec):
        self.nvec = np.asarray(nvec, np.int64)
        self.shape = self.nvec.shape

    def seed(self, s):
        pass


class NvecBenchProcessEnv(B.BenchProcessEnv):
    def __init__(self, seed=0):
        super().__init__(seed)
        self.action_space = MultiDiscrete(NVEC)


class MaskedNvecBenchProcessEnv(NvecBenchProcessEnv):
    def __init__(self, seed=0):
        super().__init__(seed)
        rs = np.random.RandomState(seed + 1)
        self._masks = rs.rand(64, B.AGENTS, S) < 2.0 / 3.0
        s = 0
        for b in NVEC:   # every head of every row has a valid bin
            self._masks[:, :, s] |= ~self._masks[:, :, s:s + b].any(axis=2)
            s += b

    def action_masks(self):
        return self._masks[self._i % 64]


def make_env():
    return NvecBenchProcessEnv()


def make_masked_env():
    return MaskedNvecBenchProcessEnv()
