"""The V-trace option without a GPU: where its keywords sit, and the argument errors rlppo_gae_vtrace reports before any HIP call."""
import ctypes
import inspect

import numpy as np
import pytest


def test_keywords_and_defaults():
    from rlgym_ppo_amd import Learner
    from rlgym_ppo_amd.util import torch_functions as TF
    params = inspect.signature(Learner.__init__).parameters
    names = list(params)
    i = names.index("gae_vtrace")
    assert names[i:i + 3] == ["gae_vtrace", "gae_vtrace_rho_bar", "gae_vtrace_c_bar"]
    assert [params[k].default for k in names[i:i + 3]] == [False, 1.0, 1.0]
    for fn in (TF.gae_device, TF.gae_device_deferred):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "vtrace" and p["vtrace"].default is None


@pytest.mark.parametrize("change, names", [(dict(rews=None), "rews"), (dict(logp_new=None), "logp_new"), (dict(advantages=None), "advantages"),
                                           (dict(rho_bar=0.0), "rho_bar"), (dict(c_bar=float("nan")), "c_bar"), (dict(n=-1), "n=")])
def test_argument_errors_name_the_argument(change, names):
    from rlgym_ppo_amd import _native as N
    lib = N.lib()
    buf = np.zeros(64, np.float32)          # host memory: a call that got as far as a launch would be a defect of the checks
    p = ctypes.c_void_p(buf.ctypes.data)
    a = dict(stream=None, rews=p, dones=p, truncated=p, values=p, boot_values=None, value_scale=None, logp_new=p, logp_old=p, n=8,
             gamma=0.99, lmbda=0.95, rho_bar=1.0, c_bar=1.0, return_std=float("nan"), value_targets=p, advantages=p, workspace=p, ws_bytes=0)
    a.update(change)
    assert lib.rlppo_gae_vtrace(*a.values()) == 1001
    assert names.encode() in lib.rlppo_last_error()
