"""Bootstrapping truncated trajectories from V(next state), the parts that need no GPU: the exported symbol and its binding, the
argument checks of rlppo_gae_boot (before any HIP call), the Learner keyword, and the check the GPU tests' yardstick rests on --
that the CPU oracle applied per trajectory reproduces the oracle on the whole array when every segment's bootstrap value is
V[next]."""
import ctypes
import inspect

import numpy as np
import pytest

import gae_bootstrap_yardstick as Y
from oracle import gae as ogae


def test_symbol_is_exported_and_bound_and_abi_stays_8():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    assert hasattr(L, "rlppo_gae_boot")
    res, args = N.SIGNATURES["rlppo_gae_boot"]
    plain = N.SIGNATURES["rlppo_gae"]
    assert res == plain[0] and args == plain[1][:5] + [ctypes.c_void_p] + plain[1][5:]   # rlppo_gae + boot_values after values
    assert N.ABI_VERSION == 8 and L.rlppo_abi_version() == 8
    header = open(N.HERE + "/../include/rlppo.h").read()
    assert "int rlppo_gae_boot(" in header and "boot_values" in header


def test_gae_boot_rejects_bad_arguments_before_any_launch():
    """Placeholder pointers, no GPU: the checks run before the first HIP call."""
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    n = 5000
    ws_bytes = L.rlppo_gae_workspace_bytes(n)
    fake = [ctypes.c_void_p(0x100000 + 0x10000 * k) for k in range(9)]   # 16-byte aligned, distinct, never dereferenced
    rews, dones, trunc, values, boot, vt, adv, ret, ws = fake

    def call(boot=boot, ws_bytes=ws_bytes, n=n):
        rc = L.rlppo_gae_boot(None, rews, dones, trunc, values, boot, n, 0.99, 0.95, 1.0, vt, adv, ret, ws, ws_bytes)
        return rc, L.rlppo_last_error().decode()

    rc, msg = call(boot=ctypes.c_void_p(boot.value + 4))
    assert rc == 1001 and "16-byte aligned" in msg, (rc, msg)
    rc, msg = call(ws_bytes=ws_bytes - 512)
    assert rc == 1002 and "workspace" in msg, (rc, msg)
    rc, msg = call(ws_bytes=0)
    assert rc == 1002, (rc, msg)
    rc, msg = call(n=-1)
    assert rc == 1001, (rc, msg)
    assert call(n=0)[0] == 0                                              # nothing to do, nothing launched


def test_python_surface_accepts_the_keywords():
    from rlgym_ppo_amd import Learner
    from rlgym_ppo_amd.util import torch_functions as TF
    p = inspect.signature(Learner.__init__).parameters["gae_bootstrap_truncated"]
    assert p.default is False
    assert inspect.signature(TF.compute_gae).parameters["next_values"].default is None
    for fn in (TF.gae_device, TF.gae_device_deferred):
        assert inspect.signature(fn).parameters["boot_values"].default is None
    # the reference's signature stays a prefix
    assert list(inspect.signature(TF.compute_gae).parameters)[:7] == ["rews", "dones", "truncated", "values", "gamma", "lmbda", "return_std"]


@pytest.mark.parametrize("n", [1, 7, 2049, 5003])
@pytest.mark.parametrize("std", [None, 1.3])
def test_per_segment_yardstick_reproduces_the_whole_array_oracle(n, std):
    rews, dones, trunc, values, _ = Y.make_case(n, seed=n)
    boot = values[1:].copy()                                             # b = V[next] at every segment end
    seg = Y.per_segment(rews, dones, trunc, values, boot, 0.99, 0.95, std)
    whole = ogae.gae(rews, dones, trunc, values, 0.99, 0.95, std, "f64")
    for a, b in zip(seg, whole):
        assert np.array_equal(a, b)
    # and a bootstrap value that differs moves exactly the advantages of the segments that end truncated and not done
    boot2 = boot + 1.0
    seg2 = Y.per_segment(rews, dones, trunc, values, boot2, 0.99, 0.95, std)
    assert np.array_equal(seg2[2], whole[2])                             # returns are not bootstrapped
    idx = Y.boot_steps(dones, trunc)
    assert idx.size and np.all(seg2[1][idx] != whole[1][idx])
    only_done = np.flatnonzero(dones != 0)
    assert np.array_equal(seg2[1][only_done], whole[1][only_done])       # done wins over truncated
