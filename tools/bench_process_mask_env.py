"""bench_process_env.BenchProcessEnv with action_masks(): pre-drawn masks, two-thirds valid, one per pre-drawn observation -- the
synthetic environment of tools/process_mask_cost.py's masked process_collect leg.  Imported by the worker processes."""
import numpy as np

import bench_process_env as B


class MaskedBenchProcessEnv(B.BenchProcessEnv):
    def __init__(self, seed=0):
        super().__init__(seed)
        rs = np.random.RandomState(seed + 1)
        self._masks = rs.rand(64, B.AGENTS, B.ACT) < 2.0 / 3.0
        self._masks[:, :, 0] |= ~self._masks.any(axis=2)   # every row has a valid action

    def action_masks(self):
        return self._masks[self._i % 64]


def make_env():
    return B.BenchProcessEnv()


def make_masked_env():
    return MaskedBenchProcessEnv()
