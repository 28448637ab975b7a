"""Host-side pieces of the device-resident vector-environment interface: the tensor branch of the action clip, the detection
helpers of VectorAgentManager, and the new entry points in the header, the export map and the ctypes table."""
import fnmatch
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rlppo_rollout_record", "rlppo_obs_scalars", "rlppo_rollout_to_trajectory_major")


class _Echo:
    def __init__(self):
        self.seen = None

    def step(self, actions):
        self.seen = actions
        return actions


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_action_clip_tensor_branch_is_out_of_place_and_keeps_the_dtype(dtype):
    from rlgym_ppo_amd.util.action_clip import ActionClipEnv
    env = _Echo()
    a = torch.tensor([[-3.0, 0.25, 1.5], [0.999, -1.0, float("inf")]], dtype=dtype)
    before = a.clone()
    out = ActionClipEnv(env, -1.0, 1.0).step(a)
    assert isinstance(out, torch.Tensor) and out.dtype == dtype and out.device == a.device
    assert out.data_ptr() != a.data_ptr() and torch.equal(a, before)
    assert torch.equal(out, torch.tensor([[-1.0, 0.25, 1.0], [0.999, -1.0, 1.0]], dtype=dtype))


def test_action_clip_numpy_branch_is_unchanged():
    from rlgym_ppo_amd.util.action_clip import ActionClipEnv
    env = _Echo()
    out = ActionClipEnv(env, -0.5, 0.5).step([[-3.0, 0.25], [0.75, -0.5]])
    assert isinstance(out, np.ndarray) and out.dtype == np.float32
    assert np.array_equal(out, np.asarray([[-0.5, 0.25], [0.5, -0.5]], np.float32))


def test_detection_helpers():
    from rlgym_ppo_amd.batched_agents.vector_agent_manager import check_same_device, device_env_of
    assert device_env_of(np.zeros((2, 3), np.float32)) is None
    assert device_env_of([[0.0, 1.0]]) is None
    assert device_env_of(torch.zeros(2, 3)) is None            # a CPU tensor speaks the host interface
    check_same_device(torch.device("cuda", 0), "cuda:0")
    check_same_device(torch.device("cuda", 1), torch.device("cuda", 1))
    check_same_device(torch.device("cuda", 0), "cuda")         # (no index: the current device)
    with pytest.raises(ValueError, match=r"cuda:1.*cuda:0"):
        check_same_device(torch.device("cuda", 1), "cuda:0")
    with pytest.raises(ValueError, match=r"cpu.*cuda:0"):
        check_same_device(torch.device("cpu"), "cuda:0")


def test_cpu_tensor_reset_with_a_device_step_is_refused_by_name():
    from rlgym_ppo_amd.batched_agents.vector_agent_manager import _HostInterfaceGuard

    class FakeCuda(torch.Tensor):
        is_cuda = True
        device = "cuda:0"

    class Env:
        n = 3

        def step(self, actions):
            return (self.obs,)
    env = Env()
    guard = _HostInterfaceGuard(env)
    env.obs = torch.zeros(2, 2)
    assert guard.step(None)[0] is env.obs and guard.n == 3
    env.obs = torch.zeros(2, 2).as_subclass(FakeCuda)
    with pytest.raises(ValueError, match="reset\\(\\) returned a CPU tensor"):
        guard.step(None)


def test_new_entry_points_are_declared_exported_and_bound():
    from rlgym_ppo_amd import _native
    header = open(os.path.join(ROOT, "include", "rlppo.h")).read()
    exports = open(os.path.join(ROOT, "rlgym_ppo_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)[0].split()
    for name in NEW:
        assert re.search(r"^int %s\(void \*stream," % name, header, re.M), name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
        assert name in _native.SIGNATURES
    assert "#define RLPPO_ABI_VERSION 8" in header and _native.ABI_VERSION == 8
    assert re.search(r"7 = rlppo_rollout_record launches", header)
    L = _native.lib()   # resolves every symbol of the table
    assert all(hasattr(L, name) for name in NEW) and L.rlppo_dbg_counter(7) >= 0
