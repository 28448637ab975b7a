"""Invalid-action masking in process-mode collection: masks travel from a worker's environment (the opt-in trailer of
comm_consts.py) through both learner-side loops -- the Python loop and the C++ one (csrc/collector.cpp) -- to
`BatchedAgentManager.action_mask_rows`.  Real worker processes; ONE worker, so that arrival order is fixed and the two loops must
agree value for value.  standardize_obs=False: every stored state is the raw observation, so its mask can be recomputed.  CPU only."""
import numpy as np
import pytest
import torch

import masked_wire_env
import synthetic_env

CALLS = (40, 17, 1, 33)


class _MaskedPolicy:
    """Accepts action_mask=, insists on one mask row per observation and picks the lowest valid action."""

    def __init__(self):
        self.calls = 0

    def get_action(self, obs, action_mask=None):
        obs = np.asarray(obs, np.float32)
        assert action_mask is not None, "a masked run hands every call its masks"
        m = np.asarray(action_mask) != 0
        assert m.ndim == 2 and m.shape[0] == obs.shape[0] and m.any(axis=1).all()
        self.calls += 1
        return torch.as_tensor(m.argmax(axis=1).astype(np.int64)), torch.as_tensor(-np.abs(obs[:, 0]).astype(np.float32))


class _PlainPolicy:
    """The reference's signature: it would fail on an action_mask keyword."""

    def get_action(self, obs):
        obs = np.asarray(obs, np.float32)
        return torch.as_tensor((np.abs(obs[:, :5]).sum(1) * 7).astype(np.int64) % 7), torch.as_tensor(-np.abs(obs[:, 0]).astype(np.float32))


def _run(native, env_fn, policy, calls=CALLS, n_proc=1):
    from rlgym_ppo_amd.batched_agents import BatchedAgentManager
    mgr = BatchedAgentManager(policy, min_inference_size=1, seed=5, standardize_obs=False)
    mgr.native_collect = native
    try:
        shapes = mgr.init_processes(n_proc, env_fn, collect_metrics_fn=synthetic_env.step_count_metrics if "varying" in env_fn.__name__ else None,
                                    shm_buffer_size=4096)
        out = []
        for k in calls:
            exp, metrics, n, _ = mgr.collect_timesteps(k)
            out.append((exp, metrics, n, None if mgr.action_mask_rows is None else np.array(mgr.action_mask_rows, copy=True)))
        if n_proc > 0:
            assert (mgr._native is not None) == native, "the loop that ran is not the one the test asked for"
        return shapes, out, dict(avg=mgr.average_reward, total=mgr.cumulative_timesteps, masked=mgr.masked)
    finally:
        mgr.cleanup()


def _check_masks(out, n_actions):
    """Row-aligned with the states across the call boundaries: every mask is the environment's mask function of its stored state,
    and every stored action is valid (the lowest valid one) under it."""
    rows = 0
    for (states, actions, *_), _, n, masks in out:
        assert masks is not None and masks.dtype == bool and masks.shape == (len(states), n_actions)
        assert np.array_equal(masks, masked_wire_env.mask_of(states, n_actions))
        a = np.asarray(actions).reshape(-1).astype(np.int64)
        assert masks[np.arange(len(a)), a].all() and np.array_equal(a, masks.argmax(axis=1))
        rows += len(states)
    assert rows > 0


@pytest.mark.parametrize("case", ["two_agents", "single_agent_rank1", "varying_team"])
def test_native_loop_equals_the_python_loop_masks_included(case):
    env_fn, A = {"two_agents": (masked_wire_env.make_masked_wire_env, 7), "single_agent_rank1": (masked_wire_env.make_masked_single_env, 5),
                 "varying_team": (masked_wire_env.make_masked_varying_env, 7)}[case]
    (s0, o0, t0), (s1, o1, t1) = _run(False, env_fn, _MaskedPolicy()), _run(True, env_fn, _MaskedPolicy())
    assert s0 == s1 and t0 == t1 and t0["masked"]
    for (ea, ma, na, ka), (eb, mb, nb, kb) in zip(o0, o1):
        assert na == nb and len(ma) == len(mb)
        for x, y in zip(ma, mb):
            assert np.array_equal(x, y)
        assert len(ea) == len(eb) == 7                        # collect_timesteps keeps its 7-tuple
        for x, y, name in zip(ea, eb, ("states", "actions", "log_probs", "rewards", "next_states", "dones", "truncated")):
            assert x.shape == y.shape and np.array_equal(x, y), name
        assert ka.dtype == kb.dtype == bool and ka.shape == kb.shape and np.array_equal(ka, kb)
    _check_masks(o0, A)
    _check_masks(o1, A)
    if case == "varying_team":   # the flush at a team-size change really happened
        nxt = np.concatenate([o[0][4] for o in o1])
        assert (np.abs(nxt).sum(1) == 0).any()


def test_local_worker_carries_masks_too():
    pol = _MaskedPolicy()
    shapes, out, state = _run(False, masked_wire_env.make_masked_wire_env, pol, calls=(40, 17), n_proc=0)
    assert shapes == (13, 7, 0) and state["masked"] and pol.calls > 0
    _check_masks(out, 7)


@pytest.mark.parametrize("native", [False, True])
def test_an_unmasked_environment_is_never_handed_the_keyword(native):
    shapes, out, state = _run(native, synthetic_env.make_wire_env, _PlainPolicy())
    assert shapes == (13, 7, 0) and not state["masked"]
    assert all(masks is None for *_, masks in out) and sum(n for _, _, n, _ in out) >= sum(CALLS)


@pytest.mark.parametrize("native", [False, True])
def test_a_mask_row_without_a_valid_action_raises_on_the_learner(native):
    from rlgym_ppo_amd.batched_agents import BatchedAgentManager
    pol = _MaskedPolicy()
    mgr = BatchedAgentManager(pol, min_inference_size=1, seed=5, standardize_obs=False)
    mgr.native_collect = native
    try:
        mgr.init_processes(1, masked_wire_env.make_zero_row_env, shm_buffer_size=4096)
        with pytest.raises(ValueError, match=r"worker 0, agent 1 has no valid action"):
            mgr.collect_timesteps(40)
        assert (mgr._native is not None) == native
        assert pol.calls == 3   # the three steps before it were served; no action was sent for the bad observation
    finally:
        mgr.cleanup()


def test_masked_collector_entry_points_report_errors():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    assert L.rlppo_collector_set_masked(None, 7) == 1001 and b"collector_set_masked" in L.rlppo_last_error()
    assert L.rlppo_collector_ready_masks(None, None, 0) == 1001 and b"collector_ready_masks" in L.rlppo_last_error()
    assert L.rlppo_collector_emit_masks(None, None) == 1001 and b"collector_emit_masks" in L.rlppo_last_error()
    assert L.rlppo_collector_set_mask(None, 0, None, 0) == 1001 and b"collector_set_mask" in L.rlppo_last_error()
