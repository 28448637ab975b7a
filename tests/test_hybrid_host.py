"""CPU checks of the hybrid head (include/rlppo.h, "[hybrid]"): every argument refusal at the C boundary before any HIP call, and the
value errors of HybridSpace, PPOLearner, Learner and the column-wise action clip.  No GPU, no compute call."""
import ctypes

import numpy as np
import pytest
import torch

from test_diag_gaussian_host import _Agent, _args, _learner

NVEC = [3, 2]
POL = [107, 256, 256, 2 + 5]   # k = 2 means + 3 + 2 logits


def hybrid(N, L, a, nvec=NVEC, n_heads=None, nbytes=None, scratch=0x2002000):
    nv = None if nvec is None else N.dims_array(nvec)
    nbytes = L.rlppo_diag_scratch_bytes(1500, 2) if nbytes is None else nbytes
    rc = L.rlppo_ppo_minibatch_hybrid(None, ctypes.byref(a), nv, len(nvec or []) if n_heads is None else n_heads, 0x2000000, 0x2001000, scratch, nbytes)
    return rc, L.rlppo_last_error().decode()


@pytest.mark.parametrize("what, kw, call, words", [
    ("k = 0", dict(act_dim=2), {}, ("act_dim=2", "k=0")),
    ("empty nvec", dict(act_dim=4), dict(nvec=[], n_heads=0), ("n_heads", "0 heads")),
    ("NULL nvec", dict(act_dim=4), dict(nvec=None, n_heads=2), ("nvec is NULL",)),
    ("act_dim mismatch", dict(act_dim=5), {}, ("act_dim=5", "7 outputs")),
    ("bins beyond the limit", dict(act_dim=4), dict(nvec=[3, 65]), ("nvec[1]=65", "RLPPO_MD_MAX_BINS")),
    ("scratch too small", dict(act_dim=4), dict(nbytes=6 * 2 * 8 - 1), ("scratch", str(6 * 2 * 8))),
    ("scratch misaligned", dict(act_dim=4), dict(scratch=0x2002004), ("scratch", "aligned")),
    ("another head", dict(act_dim=1, head=0), {}, ("head 0", "ppo_minibatch_hybrid")),
])
def test_minibatch_hybrid_refusals_come_before_any_hip_call(what, kw, call, words):
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    rc, msg = hybrid(N, L, _args(N, L, **{"head": N.HEAD_HYBRID, "pol": POL, **kw}), **call)
    assert rc == 1001 and all(w in msg for w in words), (what, rc, msg)


def test_other_entry_points_refuse_head_4_by_name_and_masks_are_refused():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    assert N.HEAD_HYBRID == 4
    a = _args(N, L, head=4, act_dim=4, pol=POL)
    for rc in (L.rlppo_ppo_minibatch(None, ctypes.byref(a)), L.rlppo_ppo_minibatch_nvec(None, ctypes.byref(a), N.dims_array(NVEC), 2),
               L.rlppo_ppo_minibatch_diag(None, ctypes.byref(a), 0x2000000, 0x2001000, 0x2002000, 96)):
        msg = L.rlppo_last_error().decode()
        assert rc == 1001 and "head 4" in msg and "rlppo_ppo_minibatch_hybrid" in msg, (rc, msg)
    a.action_mask, a.mask_words = 0x3000000, 1
    rc, msg = hybrid(N, L, a)
    assert rc == 1001 and "action_mask" in msg and "hybrid" in msg, (rc, msg)
    a = _args(N, L, head=4, act_dim=4, pol=POL)
    a.mb = 0   # an empty pass is no error and no launch
    assert hybrid(N, L, a)[0] == 0
    # the rollout step and the kernels on their own: k, nvec and the row width, before any HIP call
    dims = N.dims_array(POL)
    act = lambda k, nvec: (L.rlppo_hybrid_act(None, dims, 3, 0x1000, 0x2000, 112, 16, k, N.dims_array(nvec), len(nvec), 0x3000, 0x4000, 0x5000,
                                              0x6000, 0x7000, 0x8000, 1 << 20, None), L.rlppo_last_error().decode())
    for k, nvec, word in ((0, [3, 2], "k=0"), (2, [3, 3], "output width 7"), (N.DIAG_MAX_K + 1, [3, 2], "RLPPO_DIAG_MAX_K"), (2, [], "0 heads")):
        rc, msg = act(k, nvec)
        assert rc == 1001 and word in msg, (rc, msg)
    rc = L.rlppo_dbg_hybrid_loss(None, 0x1000, 6, 2, N.dims_array(NVEC), 2, 0x2000, 0x3000, 0x4000, 16, 0.2, 0.0, 1.0, 0x5000, 0x6000, 0x7000, 16, 0x8000, 0)
    assert rc == 1001 and "ld=6" in L.rlppo_last_error().decode()


def test_hybrid_space_and_learner_value_errors(monkeypatch, tmp_path):
    from rlgym_ppo_amd import ppo
    s = ppo.HybridSpace(2, [3, 2])
    assert s == (2, (3, 2)) and s.k == 2 and s.nvec == (3, 2)
    for k, nvec in ((0, [2]), (257, [2]), (1.5, [2]), (2, []), (2, [0]), (2, [65])):
        with pytest.raises(ValueError):
            ppo.HybridSpace(k, nvec)
    # policy_type 4 and a HybridSpace go together; a bare nvec stays the multi-discrete policy's (both refused before the GPU is needed)
    common = ((256,), (256,), (0.1, 1.0), 64, 1, 3e-4, 3e-4, 0.2, 0.005, 64, "cuda:0")
    for space, ptype, word in ((s, 3, "HybridSpace"), (7, 4, "HybridSpace"), ([3, 2], 4, "HybridSpace"), ([3, 2], 3, "policy_type 1")):
        with pytest.raises(ValueError, match=word):
            ppo.PPOLearner(11, space, ptype, *common)
    with pytest.raises(ValueError, match="'hybrid' needs multi_discrete_bins"):
        _learner(monkeypatch, tmp_path, continuous_head="hybrid", vector_env=True)
    with pytest.raises(ValueError, match="'hybrid' needs vector_env=True.*process-mode"):
        _learner(monkeypatch, tmp_path, continuous_head="hybrid", multi_discrete_bins=[3, 2])
    with pytest.raises(ValueError, match="symmetry"):
        _learner(monkeypatch, tmp_path, continuous_head="hybrid", multi_discrete_bins=[2], vector_env=True, symmetry=object())
    from rlgym_ppo_amd import learner as LM
    monkeypatch.setattr(LM, "VectorAgentManager", _Agent)   # reports an action width of 3
    with pytest.raises(ValueError, match="action width of 3.*3 entries"):
        _learner(monkeypatch, tmp_path, continuous_head="hybrid", multi_discrete_bins=[2, 2, 2], vector_env=True)


def test_action_clip_by_columns():
    from rlgym_ppo_amd.util.action_clip import ActionClipEnv, ClippedEnvFactory

    class Env:
        def step(self, actions):
            return actions
    a = np.array([[-3.0, 0.5, 2.0, 1.0], [4.0, -0.2, 0.0, 2.0]], np.float32)
    want = np.array([[-1.0, 0.5, 2.0, 1.0], [1.0, -0.2, 0.0, 2.0]], np.float32)
    for columns in (2, -2):   # the first two; all but the last two
        env = ClippedEnvFactory(Env, -1.0, 1.0, columns)()
        assert np.array_equal(env.step(a), want) and a[0, 0] == -3.0   # out of place
        assert torch.equal(env.step(torch.as_tensor(a)), torch.as_tensor(want))
    assert np.array_equal(ActionClipEnv(Env(), -1.0, 1.0).step(a), np.clip(a, -1, 1))   # the default: every column, as before
